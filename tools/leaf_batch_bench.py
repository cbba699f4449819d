"""What searching several leaves per lock-step (leaf_batch = K, virtual loss) buys where one simulation per lock-step leaves the chip
empty (Othello 8x8, random-init OthelloNet on the HIP network):
  a. one game's MCT.search from a fresh root, n_sim 100 and 800, K = 1, 2, 4, 8, 16: us per simulation, ms per move, and the share
     of simulations that collided with a pending leaf of their own lock-step;
  b. a 64-game BatchedAlphaZeroPlayer.get_moves at 100 simulations, K = 1, 2, 4 (64 K rows cross the 256-row knee at K = 4).
Wall-clock medians of repeats after a warm-up (the first searches are plain launches and the graph capture); every timed call blocks
until its results are there.  --k1-only measures the K = 1 legs alone and touches nothing the option added, so the same file runs on
a tree without it (K = 1 is meant to be unchanged: compare the two).
usage: python tools/leaf_batch_bench.py [--k1-only] [--out profiles/r10_leaf_batch.txt] [--repeats 15]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_amd.games.othello import OthelloBoard, OthelloNet  # noqa: E402
from alphazero_amd.mcts import MCT  # noqa: E402
from alphazero_amd.players import BatchedAlphaZeroPlayer  # noqa: E402

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def spread(xs, scale, unit):
    return f"median {statistics.median(xs) * scale:9.3f} {unit}  (min {min(xs) * scale:.3f}, max {max(xs) * scale:.3f}, {len(xs)} repeats)"


def one_game(net, k, n_sim, repeats):
    """MCT.search of the start position from a fresh root each time -> (seconds per search, collision share)"""
    mct = MCT(eval_method="neural", nn=net, seed=1, **({"leaf_batch": k} if k > 1 else {}))
    b = OthelloBoard(n=8)
    ts, c0 = [], 0
    for i in range(repeats + 3):
        mct._root_key = None  # the next search starts the tree afresh from the board: the same work each time
        if i == 3 and k > 1:
            c0 = mct._engine.collisions()
        t = time.perf_counter()
        mct.search(b, n_sim=n_sim)
        if i >= 3:
            ts.append(time.perf_counter() - t)
    share = (mct._engine.collisions() - c0) / (repeats * n_sim) if k > 1 else 0.0
    assert mct._engine.stats()["graph_replays"] > 0
    mct._engine.close()
    return ts, share


def batched_player(net, k, repeats, games=64, n_sim=100):
    player = BatchedAlphaZeroPlayer(n_sim=n_sim, nn=net, n_slots=games, seed=2, **({"leaf_batch": k} if k > 1 else {}))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k1-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--trace", action="store_true", help="one-game leg at 100 simulations, K = 1 and 8 only (for rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    net = OthelloNet(8, device="cuda")
    net.eval()
    say(f"python tools/leaf_batch_bench.py{' --k1-only' if a.k1_only else ''}{' --trace' if a.trace else ''}: Othello 8x8, random-init OthelloNet, "
        f"{torch.cuda.get_device_name(0)}")
    ks = [1] if a.k1_only else ([1, 8] if a.trace else [1, 2, 4, 8, 16])
    med = statistics.median
    one = {}
    for n_sim in ([100] if a.trace else [100, 800]):
        for k in ks:
            ts, share = one_game(net, k, n_sim, a.repeats)
            one[k, n_sim] = med(ts)
            say(f"a. 1 game, MCT.search, n_sim {n_sim:3d}, K {k:2d} : {spread([t / n_sim for t in ts], 1e6, 'us per simulation')}  "
                f"{med(ts) * 1e3:7.3f} ms per move, collisions {share:.4f}")
        for k in ks[1:]:
            say(f"   n_sim {n_sim:3d}: K {k:2d} takes {one[1, n_sim] / one[k, n_sim]:.2f}x fewer us per simulation than K 1")
    if a.trace:
        return
    many = {}
    for k in [1] if a.k1_only else [1, 2, 4]:
        ts = batched_player(net, k, a.repeats)
        many[k] = med(ts)
        say(f"b. 64-game BatchedAlphaZeroPlayer.get_moves, n_sim 100, K {k:2d} : {spread(ts, 1e3, 'ms per call')}")
    for k in list(many)[1:]:
        say(f"   64 games: K {k:2d} takes {many[1] / many[k]:.2f}x less time per call than K 1")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
