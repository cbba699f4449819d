"""A strength number that needs no opponent: how often a player keeps the game-theoretic outcome in the last plies of its own games.
Plays N self-play games of a checkpoint (or a random-init net) with exact endgames OFF (and, with --proof-backup, a second wave of the
same seeds with proof backup ON: az_engine_set_proof_backup), then solves every recorded position with at
most --max-empties empty cells (engine.solve_batch) together with the position its played move led to: the move KEEPS the outcome
when the successor's outcome is the position's.  Reported per empties count: plies, the share that kept the outcome, and the share
of the positions' outcomes that were still open (not lost for the mover).
usage: python tools/endgame_accuracy.py [--out profiles/r27_exact_endgame.txt] [--checkpoint PATH] [--games 1024] [--sims 100]
       [--board-size 8] [--max-empties 10] [--proof-backup]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_amd import _lib  # noqa: E402
from alphazero_amd import engine as E  # noqa: E402
from alphazero_amd.games.othello import OthelloNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r27_exact_endgame.txt")
    ap.add_argument("--checkpoint", default=None, help="a torch state_dict of OthelloNet (default: random init, torch.manual_seed(0))")
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--board-size", type=int, default=8)
    ap.add_argument("--max-empties", type=int, default=10)
    ap.add_argument("--proof-backup", action="store_true", help="a second leg of the same seeds with proof backup on, for comparison")
    a = ap.parse_args()
    n = a.board_size
    torch.manual_seed(0)
    net = OthelloNet(n=n).eval()
    if a.checkpoint:
        net.load_state_dict(torch.load(a.checkpoint, map_location="cpu"))
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    hip = E.HipNet(0, n, n, sd, max_batch=a.games)
    lines = []
    for proof in ((False, True) if a.proof_backup else (False,)):
        lines += leg(a, n, hip, proof)
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


def leg(a, n, hip, proof):
    """one wave with proof backup on or off -> the report's lines"""
    eng = E.SelfPlayEngine(0, n, n, n_slots=a.games, n_sim=a.sims, net=hip, seed=3)
    eng.set_proof_backup(proof)
    smp = eng.run(a.games)
    st = eng.stats()
    assert st["games_done"] == a.games and st["error_flags"] == 0
    eng.close()
    # a sample's state is player * grid: the mover's own frame, so the position is (state, +1) and outcomes come back in that frame
    state, meta = smp["state"].contiguous(), smp["meta"]
    empties = (state == 0).flatten(1).sum(1)
    late = torch.nonzero(empties <= a.max_empties).flatten()
    grids = state[late].contiguous()
    ones = torch.ones(len(late), dtype=torch.int8, device=grids.device)
    acts = meta[late, 3].to(torch.int32).contiguous()
    nxt, nxt_p, status = E.play_batch(0, n, n, grids, ones, acts)
    assert int((status != 0).sum()) == 0
    w0, _ = E.solve_batch(0, n, n, grids, ones, a.max_empties)
    w1, _ = E.solve_batch(0, n, n, nxt, nxt_p, a.max_empties)
    assert int((w0 == _lib.UNSOLVED).sum()) == 0 and int((w1 == _lib.UNSOLVED).sum()) == 0
    kept = (w0 == w1).cpu().numpy()
    open_ = (w0 >= 0).cpu().numpy()
    em = empties[late].cpu().numpy()
    lines = [f"endgame accuracy: Othello {n}x{n}, {a.games} self-play games, exact endgames off, proof backup {'ON' if proof else 'off'}, at {a.sims} simulations, "
             f"{'checkpoint ' + a.checkpoint if a.checkpoint else 'random-init OthelloNet'}; {torch.cuda.get_device_name(0)}",
             f"{'empties':>8} {'plies':>8} {'kept outcome':>13} {'outcome open':>13}"]
    for e in range(1, a.max_empties + 1):
        sel = em == e
        if sel.any():
            lines.append(f"{e:>8} {int(sel.sum()):>8} {kept[sel].mean() * 100:>12.2f}% {open_[sel].mean() * 100:>12.2f}%")
    lines.append(f"{'all':>8} {len(em):>8} {kept.mean() * 100:>12.2f}% {open_.mean() * 100:>12.2f}%")
    return lines


if __name__ == "__main__":
    main()
