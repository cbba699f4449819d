"""What the Gumbel root search costs and buys (Othello 8x8, random-init OthelloNet on the HIP network), plain PUCT root against
gumbel = 16 at n_sim 16, 32 and 100:
  a. one game's MCT.search from a fresh root: us per simulation, ms per move;
  b. a 64-game BatchedAlphaZeroPlayer.get_moves: ms per call;
  c. a 4096-slot self-play wave (SelfPlayEngine.run of 4096 games): games/s and examples/s.
At equal n_sim the two searches launch the same sequence (k_step_gumbel for k_step); the mode exists for c. at n_sim 16 and 32
against plain at 100: fewer simulations per move, not a faster kernel.  Wall-clock medians of repeats after a warm-up; every timed
call blocks until its results are there.  --trace runs the one-game leg at n_sim 100 alone (for rocprofv3 --kernel-trace --stats).
usage: python tools/gumbel_bench.py [--out profiles/r13_gumbel.txt] [--repeats 9] [--wave-repeats 2] [--trace]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_amd import engine as E  # noqa: E402
from alphazero_amd.games.othello import OthelloBoard, OthelloNet  # noqa: E402
from alphazero_amd.mcts import MCT  # noqa: E402
from alphazero_amd.players import BatchedAlphaZeroPlayer  # noqa: E402

LINES = []
M = 16


def say(s):
    print(s, flush=True)
    LINES.append(s)


def spread(xs, scale, unit):
    return f"median {statistics.median(xs) * scale:9.3f} {unit}  (min {min(xs) * scale:.3f}, max {max(xs) * scale:.3f}, {len(xs)} repeats)"


def opt(gumbel):
    return {"gumbel": M} if gumbel else {}


def one_game(net, gumbel, n_sim, repeats):
    mct = MCT(eval_method="neural", nn=net, seed=1, **opt(gumbel))
    b = OthelloBoard(n=8)
    ts = []
    for i in range(repeats + 3):
        mct._root_key = None  # the next search starts the tree afresh from the board: the same work each time
        t = time.perf_counter()
        mct.search(b, n_sim=n_sim)
        if i >= 3:
            ts.append(time.perf_counter() - t)
    assert mct._engine.stats()["graph_replays"] > 0
    mct._engine.close()
    return ts


def batched_player(net, gumbel, n_sim, repeats, games=64):
    player = BatchedAlphaZeroPlayer(n_sim=n_sim, nn=net, n_slots=games, seed=2, **opt(gumbel))
    boards = [OthelloBoard(n=8) for _ in range(games)]
    rng = np.random.default_rng(5)
    for b in boards:  # 64 different early positions
        for _ in range(int(rng.integers(0, 8))):
            moves = b.get_moves()
            b.play_move(moves[int(rng.integers(len(moves)))])
    ts = []
    for i in range(repeats + 3):
        player.reset()  # every call searches from fresh roots: the same work each time
        t = time.perf_counter()
        player.get_moves(boards, temps=0)
        if i >= 3:
            ts.append(time.perf_counter() - t)
    player.close()
    return ts


def wave(hip, gumbel, n_sim, repeats, games=4096):
    """-> [(games/s, examples/s)] of whole self-play waves; the first one (plain launches, graph capture) is not timed"""
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=games, n_sim=n_sim, net=hip, seed=3)
    if gumbel:
        eng.set_gumbel(M)
    out = []
    for i in range(repeats + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.run(games, first_game_id=i * games)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        st = eng.stats()
        assert st["games_done"] == games and st["error_flags"] == 0
        if i >= 1:
            out.append((games / dt, st["samples"] / dt))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--wave-repeats", type=int, default=2)
    ap.add_argument("--trace", action="store_true", help="one-game leg at 100 simulations only (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--no-wave", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    net = OthelloNet(8, device="cuda")
    net.eval()
    say(f"python tools/gumbel_bench.py{' --trace' if a.trace else ''}: Othello 8x8, random-init OthelloNet, gumbel m = {M}, "
        f"{torch.cuda.get_device_name(0)}")
    med = statistics.median
    sims = [100] if a.trace else [16, 32, 100]
    for n_sim in sims:
        res = {}
        for gumbel in (False, True, False, True):  # alternated: the second pair shows the spread of a repeat
            ts = one_game(net, gumbel, n_sim, a.repeats)
            res.setdefault(gumbel, []).append(med(ts))
            say(f"a. 1 game, MCT.search, n_sim {n_sim:3d}, {'gumbel' if gumbel else 'plain '} : {spread([t / n_sim for t in ts], 1e6, 'us per simulation')}  "
                f"{med(ts) * 1e3:7.3f} ms per move")
        say(f"   n_sim {n_sim:3d}: gumbel / plain = {med(res[True]) / med(res[False]):.3f} (plain runs {res[False][0] * 1e3:.3f} and {res[False][1] * 1e3:.3f} ms)")
    if a.trace:
        return
    for n_sim in sims:
        res = {}
        for gumbel in (False, True):
            ts = batched_player(net, gumbel, n_sim, a.repeats)
            res[gumbel] = med(ts)
            say(f"b. 64-game BatchedAlphaZeroPlayer.get_moves, n_sim {n_sim:3d}, {'gumbel' if gumbel else 'plain '} : {spread(ts, 1e3, 'ms per call')}")
        say(f"   n_sim {n_sim:3d}: gumbel / plain = {res[True] / res[False]:.3f}")
    if not a.no_wave:
        hip = net.to_hip(max_batch=4096)
        got = {}
        for n_sim in sims:
            for gumbel in (False, True):
                r = wave(hip, gumbel, n_sim, a.wave_repeats)
                got[gumbel, n_sim] = (med([x[0] for x in r]), med([x[1] for x in r]))
                say(f"c. 4096-slot wave, n_sim {n_sim:3d}, {'gumbel' if gumbel else 'plain '} : " +
                    ", ".join(f"{g:8.1f} games/s {x:10.1f} examples/s" for g, x in r))
        for n_sim in sims:
            say(f"   n_sim {n_sim:3d}: gumbel / plain games/s = {got[True, n_sim][0] / got[False, n_sim][0]:.3f}")
        for n_sim in (16, 32):
            say(f"   gumbel at n_sim {n_sim} against plain at 100: {got[True, n_sim][0] / got[False, 100][0]:.2f}x the games/s, "
                f"{got[True, n_sim][1] / got[False, 100][1]:.2f}x the examples/s (fewer simulations per move, not a faster kernel)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
