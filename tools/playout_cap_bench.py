"""What playout cap randomization costs and buys (Othello 8x8, 4096 slots, n_sim 100, random-init OthelloNet on the
HIP network): the mode off against (n_fast, p_full) = (25, 0.25) and (16, 0.25), alternated A B C A B C in one session.
  a. a 4096-game self-play wave (SelfPlayEngine.run): games/s, samples/s, full / fast plies, network rows per enqueued lock-step;
  b. one search of 4096 fresh roots (set_roots, search): the lock-step time of the first n_fast steps -- search(n_fast), every slot
     walks -- against the rest -- (search(n_sim) - search(n_fast)) / (n_sim - n_fast), where only the slots whose ply-0 coin is full
     walk; the mode-off leg is timed at the same two lengths;
  c. the network's stage times (HipNet.time_stage: trunk, fc1, fc2, heads, whole forward) at the tail's row count and at the batch
     cap the host launches with: what the tail steps could cost if the dispatch followed the device row counter.
Wall-clock times of calls that block until their results are there; the first wave and the first two searches of an engine (plain
launches, graph capture) are not timed.
usage: python tools/playout_cap_bench.py [--out profiles/r18_playout_cap.txt] [--wave-repeats 1] [--search-repeats 5] [--caps 25:0.25,16:0.25]"""
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

LINES = []
GAMES, N_SIM, SEED = 4096, 100, 3


def say(s):
    print(s, flush=True)
    LINES.append(s)


def name(cap):
    return "cap off        " if cap is None else f"cap ({cap[0]:2d}, {cap[1]:.2f})"


def engine(hip, cap):
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=GAMES, n_sim=N_SIM, net=hip, seed=SEED)
    eng.set_playout_cap(cap)
    return eng


def wave(hip, cap, repeats):
    """-> [(games/s, samples/s, full plies, fast plies, rows per enqueued lock-step)] of whole waves after an untimed first one"""
    eng = engine(hip, cap)
    out = []
    for i in range(repeats + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.run(GAMES, first_game_id=i * GAMES)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        st, cs = eng.stats(), eng.playout_cap_stats()
        assert st["games_done"] == GAMES and st["error_flags"] == 0
        if i >= 1:
            out.append((GAMES / dt, st["samples"] / dt, cs["full_plies"], cs["fast_plies"], st["net_evals"] / float(max(1, st["lockstep_iters"]))))
    groups = eng.groups()
    eng.close()
    return out, groups


def searches(hip, cap, lengths, repeats):
    """-> {n: [seconds]} of search(n) on 4096 fresh roots (the start position, game ids 0 .. 4095, ply 0)"""
    eng = engine(hip, cap)
    b = OthelloBoard(n=8)
    grids, players = np.tile(b.grid.astype(np.int8)[None], (GAMES, 1, 1)), np.full(GAMES, b.player, np.int8)
    out = {}
    for n in lengths:
        ts = []
        for i in range(repeats + 2):
            eng.set_roots(grids, players)
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.search(n)
            if i >= 2:
                ts.append(time.perf_counter() - t)
        out[n] = ts
    assert eng.stats()["graph_replays"] > 0 and eng.stats()["error_flags"] == 0
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--wave-repeats", type=int, default=1)
    ap.add_argument("--search-repeats", type=int, default=5)
    ap.add_argument("--caps", default="25:0.25,16:0.25")
    a = ap.parse_args()
    caps = [(int(c.split(":")[0]), float(c.split(":")[1])) for c in a.caps.split(",")]
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    net = OthelloNet(8, device="cuda")
    net.eval()
    hip = net.to_hip(max_batch=GAMES)
    med = statistics.median
    say(f"python tools/playout_cap_bench.py: Othello 8x8, {GAMES} slots, n_sim {N_SIM}, random-init OthelloNet, {torch.cuda.get_device_name(0)}")
    legs = [None] + caps
    got = {}
    for cap in legs + legs:  # alternated: the second round shows the spread of a repeat
        r, groups = wave(hip, cap, a.wave_repeats)
        got.setdefault(cap, []).extend(r)
        for g, s, full, fast, rows in r:
            say(f"a. wave of {GAMES} games, {name(cap)}, {groups} slot groups: {g:8.1f} games/s {s:10.1f} samples/s; {full} full + {fast} fast plies; "
                f"{rows:7.1f} network rows per enqueued lock-step")
    off_g, off_s, off_rows = med([x[0] for x in got[None]]), med([x[1] for x in got[None]]), med([x[4] for x in got[None]])
    say(f"   cap off runs: {', '.join(f'{x[0]:.1f}' for x in got[None])} games/s")
    for cap in caps:
        g, s, rows = med([x[0] for x in got[cap]]), med([x[1] for x in got[cap]]), med([x[4] for x in got[cap]])
        pred = (cap[1] * N_SIM + (1.0 - cap[1]) * cap[0]) / N_SIM
        say(f"   {name(cap)} / off: games/s {g / off_g:.3f}, samples/s {s / off_s:.3f}, network rows {rows / off_rows:.3f} (predicted {pred:.3f})")
    for cap in caps:
        n_fast = cap[0]
        res = {leg: searches(hip, leg, (n_fast, N_SIM), a.search_repeats) for leg in (None, cap)}
        for leg in (None, cap):
            head = med(res[leg][n_fast]) / n_fast
            tail = (med(res[leg][N_SIM]) - med(res[leg][n_fast])) / (N_SIM - n_fast)
            say(f"b. search of {GAMES} fresh roots, {name(leg)}: the first {n_fast} lock-steps {head * 1e6:7.1f} us each, the other {N_SIM - n_fast} "
                f"{tail * 1e6:7.1f} us each (search({n_fast}) {med(res[leg][n_fast]) * 1e3:.3f} ms, search({N_SIM}) {med(res[leg][N_SIM]) * 1e3:.3f} ms)")
        full0 = sum(E.SelfPlayEngine.playout_cap_full(SEED, g, 0, cap[1]) for g in range(GAMES))
        say(f"   {name(cap)}: {full0} of the {GAMES} roots are full plies: the tail steps carry {full0} rows under a launch cap of {GAMES}")
    rows = sorted({int(GAMES * p) for _, p in caps} | {int(GAMES // 2 * p) for _, p in caps} | {GAMES // 2, GAMES})
    for B in rows:
        ts = [hip.time_stage(s, B, 20) * 1e3 for s in (0, 1, 2, 3, -1)]
        say(f"c. network stages at {B:4d} rows: trunk {ts[0]:6.1f}, fc1 {ts[1]:6.1f}, fc2 {ts[2]:6.1f}, heads {ts[3]:6.1f}, whole forward {ts[4]:6.1f} us "
            f"({hip.stage_kernel(0, B)}, {hip.stage_kernel(1, B)}, {hip.stage_kernel(2, B)}, {hip.stage_kernel(3, B)})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
