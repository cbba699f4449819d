"""What forced playouts and policy target pruning cost (Othello 8x8, 4096 slots, n_sim 100, random-init OthelloNet on
the HIP network): the mode off against k = 2, with the playout cap off and with the cap at (25, 0.25), alternated A B A B in one session.
  a. a 4096-game self-play wave (SelfPlayEngine.run): games/s, samples/s, the share of root selections that had a forced child
     (forced_picks over the simulations walked on full plies) and the share of recorded playouts that were pruned (pruned_playouts
     over the visits of the recorded rows);
  b. the lock-step kernel alone: one search of 4096 fresh roots with the fake evaluator, whose network stand-in is one small kernel, so
     that the time per lock-step is k_step's / k_step_forced's (and k_step_cap's / k_step_cap_forced's) plus the same constant; the
     same search with the HIP network beside it.
Wall-clock times of calls that block until their results are there; the first wave and the first two searches of an engine (plain
launches, graph capture) are not timed.  Whether the pruned targets train a stronger network is not measured here.
usage: python tools/forced_playouts_bench.py [--out profiles/r20_forced_playouts.txt] [--wave-repeats 1] [--search-repeats 5] [--k 2]"""
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
GAMES, N_SIM, SEED, CAP = 4096, 100, 3, (25, 0.25)


def say(s):
    print(s, flush=True)
    LINES.append(s)


def name(cap, k):
    return ("cap off       " if cap is None else f"cap ({cap[0]:2d}, {cap[1]:.2f})") + (", forced off" if k is None else f", forced k={k:g}")


def engine(hip, cap, k):
    if hip is None:
        eng = E.SelfPlayEngine(0, 8, 8, n_slots=GAMES, n_sim=N_SIM, evaluator=E.EVAL_FAKE, seed=SEED)
    else:
        eng = E.SelfPlayEngine(0, 8, 8, n_slots=GAMES, n_sim=N_SIM, net=hip, seed=SEED)
    eng.set_playout_cap(cap)
    eng.set_forced_playouts(k)
    return eng


def wave(hip, cap, k, repeats):
    """-> [(games/s, samples/s, forced share, pruned share, forced picks, pruned playouts)] of whole waves after an untimed first one"""
    eng = engine(hip, cap, k)
    out = []
    for i in range(repeats + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        smp = eng.run(GAMES, first_game_id=i * GAMES)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        st, fs, cs = eng.stats(), eng.forced_playouts_stats(), eng.playout_cap_stats()
        assert st["games_done"] == GAMES and st["error_flags"] == 0
        if i >= 1:
            full_plies = cs["full_plies"] if cap is not None else st["plies"]
            visits = int(smp["visits"].sum().item())
            out.append((GAMES / dt, st["samples"] / dt, fs["forced_picks"] / float(max(1, full_plies * N_SIM)), fs["pruned_playouts"] / float(max(1, visits)),
                        fs["forced_picks"], fs["pruned_playouts"]))
    groups = eng.groups()
    eng.close()
    return out, groups


def searches(hip, cap, k, repeats):
    """-> [seconds] of search(N_SIM) on 4096 fresh roots (the start position, game ids 0 .. 4095, ply 0)"""
    eng = engine(hip, cap, k)
    b = OthelloBoard(n=8)
    grids, players = np.tile(b.grid.astype(np.int8)[None], (GAMES, 1, 1)), np.full(GAMES, b.player, np.int8)
    ts = []
    for i in range(repeats + 2):
        eng.set_roots(grids, players)
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.search(N_SIM)
        if i >= 2:
            ts.append(time.perf_counter() - t)
    assert eng.stats()["graph_replays"] > 0 and eng.stats()["error_flags"] == 0
    eng.close()
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--wave-repeats", type=int, default=1)
    ap.add_argument("--search-repeats", type=int, default=5)
    ap.add_argument("--k", type=float, default=2.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    net = OthelloNet(8, device="cuda")
    net.eval()
    hip = net.to_hip(max_batch=GAMES)
    med = statistics.median
    say(f"python tools/forced_playouts_bench.py: Othello 8x8, {GAMES} slots, n_sim {N_SIM}, random-init OthelloNet, {torch.cuda.get_device_name(0)}")
    for cap in (None, CAP):
        got = {}
        for k in (None, a.k, None, a.k):  # alternated: the second round shows the spread of a repeat
            r, groups = wave(hip, cap, k, a.wave_repeats)
            got.setdefault(k, []).extend(r)
            for g, s, fshare, pshare, picks, pruned in r:
                say(f"a. wave of {GAMES} games, {name(cap, k)}, {groups} slot groups: {g:8.1f} games/s {s:10.1f} samples/s; "
                    f"forced root selections {picks} ({fshare:.4f} of the full plies' simulations), pruned playouts {pruned} ({pshare:.2e} of the recorded visits)")
        off_g, off_s = med([x[0] for x in got[None]]), med([x[1] for x in got[None]])
        on_g, on_s = med([x[0] for x in got[a.k]]), med([x[1] for x in got[a.k]])
        say(f"   {name(cap, None)} runs: {', '.join(f'{x[0]:.1f}' for x in got[None])} games/s; k={a.k:g} runs: {', '.join(f'{x[0]:.1f}' for x in got[a.k])} games/s; "
            f"on / off: games/s {on_g / off_g:.3f}, samples/s {on_s / off_s:.3f}")
    for net_name, h in (("fake evaluator", None), ("HIP network", hip)):
        for cap in (None, CAP):
            res = {}
            for k in (None, a.k, None, a.k):
                res.setdefault(k, []).extend(searches(h, cap, k, a.search_repeats))
            off, on = med(res[None]) / (N_SIM + 1), med(res[a.k]) / (N_SIM + 1)
            say(f"b. search of {GAMES} fresh roots, {net_name}, {name(cap, None)[:14]}: {off * 1e6:7.1f} us per lock-step with the mode off "
                f"(min {min(res[None]) / (N_SIM + 1) * 1e6:.1f}, max {max(res[None]) / (N_SIM + 1) * 1e6:.1f}), {on * 1e6:7.1f} us with k={a.k:g} "
                f"(min {min(res[a.k]) / (N_SIM + 1) * 1e6:.1f}, max {max(res[a.k]) / (N_SIM + 1) * 1e6:.1f}): {(on - off) * 1e6:+.1f} us per launch")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
