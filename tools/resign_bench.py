"""What resignation in self-play costs and buys (Othello 8x8, 4096 slots, n_sim 100, random-init OthelloNet on the HIP
network):
  a. a record-only wave (holdout 1.0, consecutive 2, min_ply as given) gives the game log; resign.calibrate at the target false-positive
     rate gives the threshold; its samples are compared with a mode-off wave's;
  b. the mode off against the mode on at that threshold (holdout 0.1, consecutive 2), alternated A B A B in one session: games/s,
     samples/s, mean plies per game, the share of games resigned and the holdout's false-positive rate.
A random-initialised network's values are small: the rule may trigger rarely.  Whether shorter games train a stronger network is not
measured here.  Wall-clock times of calls that block until their results are there; the first wave of an engine (plain launches, graph
capture) is not timed.
usage: python tools/resign_bench.py [--out profiles/r31_resign.txt] [--repeats 2] [--target 0.05] [--holdout 0.1] [--min-ply 8]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_amd import engine as E  # noqa: E402
from alphazero_amd import resign as R  # noqa: E402
from alphazero_amd.games.othello import OthelloNet  # noqa: E402

LINES = []
GAMES, N_SIM, SEED, K = 4096, 100, 3, 2


def say(s):
    print(s, flush=True)
    LINES.append(s)


def wave(eng, first):
    torch.cuda.synchronize()
    t = time.perf_counter()
    smp = eng.run(GAMES, first_game_id=first)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    st = eng.stats()
    assert st["games_done"] == GAMES and st["error_flags"] == 0
    return smp, st, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--target", type=float, default=0.05)
    ap.add_argument("--holdout", type=float, default=0.1)
    ap.add_argument("--min-ply", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    net = OthelloNet(8, device="cuda")
    net.eval()
    hip = net.to_hip(max_batch=GAMES)
    say(f"python tools/resign_bench.py: Othello 8x8, {GAMES} slots, n_sim {N_SIM}, random-init OthelloNet, {torch.cuda.get_device_name(0)}")
    engines = {leg: E.SelfPlayEngine(0, 8, 8, n_slots=GAMES, n_sim=N_SIM, net=hip, seed=SEED) for leg in ("off", "on")}
    record = {"threshold": -0.5, "consecutive": K, "min_ply": a.min_ply, "holdout": 1.0}
    engines["on"].set_resign(record)
    off_smp, _, _ = wave(engines["off"], 0)  # untimed first waves: the same games, with the log and without
    rec_smp, st, _ = wave(engines["on"], 0)
    def ordered(smp):  # rows land in the order the slot groups' games finish: compare by (game id, ply)
        order = torch.argsort(smp["meta"][:, 0].long() * 4096 + smp["meta"][:, 1].long())
        return {k: v[order] for k, v in smp.items()}
    off_smp, rec_smp = ordered(off_smp), ordered(rec_smp)
    same = all(torch.equal(off_smp[k], rec_smp[k]) for k in off_smp)
    log = engines["on"].game_log()
    low, winner = log["low"].cpu().numpy(), log["winner"].cpu().numpy()
    thr = R.calibrate(low, winner, a.target, record["threshold"])
    sides = np.concatenate([low[winner >= 0, 0], low[winner <= 0, 1]])
    qs = np.quantile(np.minimum(low[:, 0], low[:, 1]), [0.05, 0.25, 0.5, 0.75, 0.95])
    say(f"a. record-only wave (consecutive {K}, min_ply {a.min_ply}): samples equal to the mode-off wave array by array: {same}; "
        f"{st['plies'] / GAMES:.2f} plies per game; winners +1 / 0 / -1: {int((winner == 1).sum())} / {int((winner == 0).sum())} / {int((winner == -1).sum())}")
    say(f"   a game's lower low, quantiles 5 / 25 / 50 / 75 / 95 %: {', '.join(f'{q:+.4f}' for q in qs)}; {len(sides)} non-losing sides, "
        f"{int((sides < thr).sum())} of them below the calibrated threshold")
    say(f"   calibrate(target {a.target}) -> threshold {thr:+.6f}; games with a side below it: {int(((low < thr).any(axis=1)).sum())} of {GAMES}")
    on = {"threshold": thr, "consecutive": K, "min_ply": a.min_ply, "holdout": a.holdout}
    engines["on"].set_resign(on)
    res = {"off": [], "on": []}
    for i in range(a.repeats):
        for leg in ("off", "on"):  # alternated
            _, st, dt = wave(engines[leg], (i + 1) * GAMES)
            rs = engines[leg].resign_stats()
            res[leg].append((GAMES / dt, st["samples"] / dt))
            tail = ""
            if leg == "on":
                fp = rs["holdout_false_positives"] / max(1, rs["holdout_games"])
                tail = (f"; resigned {rs['resigned']} ({100.0 * rs['resigned'] / GAMES:.1f} %), held out {rs['holdout_games']}, triggered "
                        f"{rs['holdout_triggered']}, false positives {rs['holdout_false_positives']} ({100.0 * fp:.1f} % of the held-out games)")
            say(f"b. wave {i + 1}, resignation {leg:3s}, {engines[leg].groups()} slot groups: {GAMES / dt:8.1f} games/s {st['samples'] / dt:10.1f} samples/s "
                f"{st['plies'] / GAMES:6.2f} plies per game{tail}")
    g = {leg: float(np.mean([x[0] for x in res[leg]])) for leg in res}
    s = {leg: float(np.mean([x[1] for x in res[leg]])) for leg in res}
    say(f"   on / off: games/s {g['on'] / g['off']:.3f}, samples/s {s['on'] / s['off']:.3f} (means of {a.repeats} waves per leg)")
    for eng in engines.values():
        eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
