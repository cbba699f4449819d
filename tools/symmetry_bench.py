"""What evaluating every leaf over the board's symmetries costs, in three regimes (Othello 8x8, 100 simulations, random-init OthelloNet):
  1. one game's search (one slot): us per simulation;
  2. a 64-game BatchedAlphaZeroPlayer.get_moves: ms per call (search of every board + one root readout, trees restarted per call);
  3. a 4096-slot self-play wave (4096 games to the end): games/s.
Each with the symmetries off, with symmetry="random" (one of the 8 orientations drawn per evaluation: the rows of the plain search)
and with symmetry="all" (8 twins per leaf), plus one game with leaf_batch=8 alone and with "random".  Wall-clock medians of repeats
after a warm-up; every timed call blocks until its results are there.  --off-only measures the off figures alone and touches nothing
the symmetry modes added, so the same file runs on a tree without them (the off path is meant to be unchanged: compare the two).
usage: python tools/symmetry_bench.py [--off-only] [--out profiles/r11_symmetry_random.txt] [--repeats 15]"""
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
from alphazero_amd.players import BatchedAlphaZeroPlayer  # noqa: E402

SIMS = 100
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def spread(xs, scale, unit):
    return f"median {statistics.median(xs) * scale:9.3f} {unit}  (min {min(xs) * scale:.3f}, max {max(xs) * scale:.3f}, {len(xs)} repeats)"


def twins(sym):
    """network rows per leaf: the ensemble evaluates every twin, the random mode one of them"""
    return 8 if sym == "all" else 1


def one_game(net, sym, repeats, leaf_batch=1):
    hip = net.to_hip(max_batch=twins(sym) * leaf_batch)
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=1, n_sim=SIMS, net=hip, seed=1)
    if sym:
        eng.set_symmetry(sym)
    if leaf_batch > 1:
        eng.set_leaf_batch(leaf_batch)
    b = OthelloBoard(n=8)
    grid, player = b.grid.astype(np.int8)[None], np.array([b.player], np.int8)
    ts = []
    for i in range(repeats + 3):  # the first searches are plain launches and the graph capture
        eng.set_roots(grid, player)
        t = time.perf_counter()
        eng.search(SIMS)
        if i >= 3:
            ts.append((time.perf_counter() - t) / SIMS)
    assert eng.stats()["graph_replays"] > 0
    eng.close()
    return ts


def batched_player(net, sym, repeats, games=64):
    kw = {"symmetry": sym} if sym else {}
    player = BatchedAlphaZeroPlayer(n_sim=SIMS, nn=net, n_slots=games, seed=2, **kw)
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


def wave(net, sym, repeats, games=4096):
    hip = net.to_hip(max_batch=twins(sym) * games)
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=games, n_sim=SIMS, net=hip, seed=3)
    if sym:
        eng.set_symmetry(sym)
    ts = []
    for i in range(repeats + 1):
        t = time.perf_counter()
        E.check(E.lib().az_engine_run(eng.h, i * games, games))  # the wave alone: no copy of the samples
        if i >= 1:
            ts.append(time.perf_counter() - t)
    st = eng.stats()
    assert st["games_done"] == games and st["error_flags"] == 0
    eng.close()
    return [games / t for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--wave-repeats", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    net = OthelloNet(8, device="cuda")
    net.eval()
    modes = [("off", None)] + ([] if a.off_only else [("random", "random"), ("all", "all")])
    say(f"python tools/symmetry_bench.py{' --off-only' if a.off_only else ''}: Othello 8x8, {SIMS} simulations, random-init OthelloNet, "
        f"{torch.cuda.get_device_name(0)}")
    res = {}
    for name, sym in modes:
        res[name, 1] = one_game(net, sym, a.repeats)
        say(f"1 game, one search, symmetry {name:6s}       : {spread(res[name, 1], 1e6, 'us per simulation')}")
    for name, sym in modes:
        res[name, 2] = batched_player(net, sym, a.repeats)
        say(f"64-game BatchedAlphaZeroPlayer.get_moves, {name:6s}: {spread(res[name, 2], 1e3, 'ms per call')}")
    for name, sym in modes:
        res[name, 3] = wave(net, sym, a.wave_repeats)
        say(f"4096-slot self-play wave, symmetry {name:6s}   : {spread(res[name, 3], 1.0, 'games/s')}")
    if not a.off_only:
        med = statistics.median
        for name, sym in modes[:2]:
            res[name, 4] = one_game(net, sym, a.repeats, leaf_batch=8)
            say(f"1 game, leaf_batch 8, symmetry {name:6s}     : {spread(res[name, 4], 1e6, 'us per simulation')}")
        say(f"random / off: one game {med(res['random', 1]) / med(res['off', 1]):.2f}x the time per simulation "
            f"(+{(med(res['random', 1]) - med(res['off', 1])) * 1e6:.1f} us; leaf_batch 8: +{(med(res['random', 4]) - med(res['off', 4])) * 1e6:.1f} us), "
            f"64 games {med(res['random', 2]) / med(res['off', 2]):.2f}x the time per call, "
            f"4096-slot wave {(1 - med(res['random', 3]) / med(res['off', 3])) * 100:.1f} % fewer games/s "
            f"({med(res['random', 3]) / med(res['all', 3]):.2f}x the ensemble's)")
        say(f"all / off: one game {med(res['all', 1]) / med(res['off', 1]):.2f}x the time per simulation "
            f"(+{(med(res['all', 1]) - med(res['off', 1])) * 1e6:.1f} us), 64 games {med(res['all', 2]) / med(res['off', 2]):.2f}x the time per call, "
            f"4096-slot wave {med(res['off', 3]) / med(res['all', 3]):.2f}x fewer games/s")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
