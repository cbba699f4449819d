"""What the Gumbel root search costs and buys (Othello 8x8, random-init OthelloNet on the HIP network), plain PUCT root against
gumbel = 16 at n_sim 16, 32 and 100:
  a. one game's MCT.search from a fresh root: us per simulation, ms per move;
  b. a 64-game BatchedAlphaZeroPlayer.get_moves: ms per call;
  c. a 4096-slot self-play wave (SelfPlayEngine.run of 4096 games): games/s and examples/s.
At equal n_sim the two searches launch the same sequence (k_step_gumbel for k_step); the mode exists for c. at n_sim 16 and 32
against plain at 100: fewer simulations per move, not a faster kernel.  Wall-clock medians of repeats after a warm-up; every timed
call blocks until its results are there.  --trace runs the one-game leg at n_sim 100 alone (for rocprofv3 --kernel-trace --stats).
--batch 1,4,16 adds a column per gumbel_batch K (K Sequential Halving leaves per network call; 1 is the leg
above): every K > 1 leg is set against K = 1, with the share of simulations that collided on a pending leaf, and for the wave the
network rows per enqueued lock-step against the K * slots the call could carry (what the idle tail of Lmax costs).
--full 0,1 adds, for every K, the leg with gumbel_full on (the paper's v_mix and its deterministic selection below
the root), set against the leg of the same K with it off.  With --full 1 alone --trace runs the full kernels.
usage: python tools/gumbel_bench.py [--out profiles/r13_gumbel.txt] [--repeats 9] [--wave-repeats 2] [--trace] [--sims 16,32,100]
       [--batch 1,4,16] [--full 0,1]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_amd import engine as E  # noqa: E402
from alphazero_amd import gumbel as G  # noqa: E402
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


def kof(gumbel):
    """the gumbel_batch K of a Gumbel leg: K itself, or (K, "full") for the leg with gumbel_full on"""
    return int(gumbel[0] if isinstance(gumbel, tuple) else gumbel)


def opt(gumbel):
    """gumbel: False (the plain search), the gumbel_batch K of the Gumbel leg, or (K, "full") with gumbel_full on"""
    return {"gumbel": M, "gumbel_batch": kof(gumbel), "gumbel_full": isinstance(gumbel, tuple)} if gumbel else {}


def name(gumbel):
    return "plain          " if not gumbel else f"gumbel K{kof(gumbel):2d}{' full' if isinstance(gumbel, tuple) else '     '}"


COLL = {}  # (leg, gumbel, n_sim) -> collisions / simulations of the timed calls


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
    COLL["a", gumbel, n_sim] = mct._engine.collisions() / float((repeats + 3) * n_sim)
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
    COLL["b", gumbel, n_sim] = player._engine.collisions() / float((repeats + 3) * n_sim * games)
    player.close()
    return ts


def wave(hip, gumbel, n_sim, repeats, games=4096):
    """-> [(games/s, examples/s)] of whole self-play waves; the first one (plain launches, graph capture) is not timed"""
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=games, n_sim=n_sim, net=hip, seed=3)
    if gumbel:
        eng.set_gumbel(M)
        eng.set_gumbel_batch(kof(gumbel))
        eng.set_gumbel_full(isinstance(gumbel, tuple))
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
    # the last wave: simulations that collided, and the network rows per enqueued lock-step (root-prior passes included in the rows)
    COLL["c", gumbel, n_sim] = eng.collisions() / float((repeats + 1) * max(1, st["samples"]) * n_sim)
    COLL["rows", gumbel, n_sim] = st["net_evals"] / float(max(1, st["lockstep_iters"]))
    if gumbel and kof(gumbel) > 1:
        # the searched roots' child counts (pi' has full support over the legal moves) and with them the lock-steps a slot's own plan
        # fills of the Lmax the host enqueues: what the idle tail costs
        nch = (eng.samples()["pi"] > 0).sum(1).cpu().numpy()
        plan = {c: len(G.lockstep_plan(n_sim, min(M, int(c)), kof(gumbel))) for c in np.unique(nch)}
        COLL["plan", gumbel, n_sim] = (float(np.mean([plan[c] for c in nch])), G.locksteps(n_sim, M, kof(gumbel)),
                                      [int(((nch >= lo) & (nch <= hi)).sum()) for lo, hi in ((1, 1), (2, 3), (4, 7), (8, 15), (16, 64))])
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--wave-repeats", type=int, default=2)
    ap.add_argument("--trace", action="store_true", help="one-game leg at 100 simulations only (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--no-wave", action="store_true")
    ap.add_argument("--sims", default="16,32,100")
    ap.add_argument("--batch", default="1", help="gumbel_batch values of the Gumbel legs, e.g. 1,4,16")
    ap.add_argument("--full", default="0", help="gumbel_full values of the Gumbel legs: 0, 0,1 (every K with it off and on) or 1")
    a = ap.parse_args()
    Ks = [int(k) for k in a.batch.split(",")]
    assert Ks and Ks[0] == 1 and all(1 <= k <= 16 for k in Ks), "--batch starts with 1 (the yardstick of the K > 1 legs)"
    assert a.full in ("0", "0,1", "1"), "--full is 0, 0,1 or 1"
    full = [(k, "full") for k in Ks] if a.full != "0" else []
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    net = OthelloNet(8, device="cuda")
    net.eval()
    say(f"python tools/gumbel_bench.py{' --trace' if a.trace else ''}: Othello 8x8, random-init OthelloNet, gumbel m = {M}, "
        f"{torch.cuda.get_device_name(0)}")
    med = statistics.median
    sims = [100] if a.trace else [int(x) for x in a.sims.split(",")]
    legs = ([False] + Ks if a.full != "1" else []) + full
    for n_sim in sims:
        res = {}
        for gumbel in legs + legs:  # alternated: the second round shows the spread of a repeat
            ts = one_game(net, gumbel, n_sim, a.repeats)
            res.setdefault(gumbel, []).append(med(ts))
            say(f"a. 1 game, MCT.search, n_sim {n_sim:3d}, {name(gumbel)} : {spread([t / n_sim for t in ts], 1e6, 'us per simulation')}  "
                f"{med(ts) * 1e3:7.3f} ms per move")
        if a.full != "1":
            say(f"   n_sim {n_sim:3d}: gumbel / plain = {med(res[1]) / med(res[False]):.3f} (plain runs {res[False][0] * 1e3:.3f} and {res[False][1] * 1e3:.3f} ms)")
            for k in Ks[1:]:
                say(f"   n_sim {n_sim:3d}: K {k:2d} / K 1 = {med(res[k]) / med(res[1]):.3f} (K 1 runs {res[1][0] * 1e3:.3f} and {res[1][1] * 1e3:.3f} ms), "
                    f"{G.locksteps(n_sim, M, k)} lock-steps for {n_sim}, collisions {COLL['a', k, n_sim]:.3f} of the simulations")
            for f in full:
                say(f"   n_sim {n_sim:3d}: K {f[0]:2d} full / K {f[0]:2d} = {med(res[f]) / med(res[f[0]]):.3f} (full off runs {res[f[0]][0] * 1e3:.3f} and "
                    f"{res[f[0]][1] * 1e3:.3f} ms), collisions {COLL['a', f, n_sim]:.3f} of the simulations")
    if a.trace:
        return
    for n_sim in sims:
        res = {}
        for gumbel in legs:
            ts = batched_player(net, gumbel, n_sim, a.repeats)
            res[gumbel] = med(ts)
            say(f"b. 64-game BatchedAlphaZeroPlayer.get_moves, n_sim {n_sim:3d}, {name(gumbel)} : {spread(ts, 1e3, 'ms per call')}")
        if a.full != "1":
            say(f"   n_sim {n_sim:3d}: gumbel / plain = {res[1] / res[False]:.3f}")
            for k in Ks[1:]:
                say(f"   n_sim {n_sim:3d}: K {k:2d} / K 1 = {res[k] / res[1]:.3f}, collisions {COLL['b', k, n_sim]:.3f} of the simulations")
            for f in full:
                say(f"   n_sim {n_sim:3d}: K {f[0]:2d} full / K {f[0]:2d} = {res[f] / res[f[0]]:.3f}, collisions {COLL['b', f, n_sim]:.3f} of the simulations")
    if not a.no_wave:
        hip = net.to_hip(max_batch=4096 * max(Ks))
        got = {}
        for n_sim in sims:
            for gumbel in legs:
                r = wave(hip, gumbel, n_sim, a.wave_repeats)
                got[gumbel, n_sim] = (med([x[0] for x in r]), med([x[1] for x in r]))
                say(f"c. 4096-slot wave, n_sim {n_sim:3d}, {name(gumbel)} : " +
                    ", ".join(f"{g:8.1f} games/s {x:10.1f} examples/s" for g, x in r) +
                    f"; {COLL['rows', gumbel, n_sim]:9.1f} network rows per enqueued lock-step of {4096 * (kof(gumbel) if gumbel else 1)}")
                if ("plan", gumbel, n_sim) in COLL:
                    mean, lmax, hist = COLL["plan", gumbel, n_sim]
                    say(f"   roots by child count 1 / 2-3 / 4-7 / 8-15 / 16+: {hist}; their own plans fill {mean:.2f} of the {lmax} lock-steps enqueued")
        for n_sim in sims if a.full != "1" else []:
            say(f"   n_sim {n_sim:3d}: gumbel / plain games/s = {got[1, n_sim][0] / got[False, n_sim][0]:.3f}")
            for k in Ks[1:]:
                say(f"   n_sim {n_sim:3d}: K {k:2d} / K 1 games/s = {got[k, n_sim][0] / got[1, n_sim][0]:.3f}, Lmax {G.locksteps(n_sim, M, k)} against "
                    f"{n_sim} lock-steps, collisions {COLL['c', k, n_sim]:.3f} of the simulations")
            for f in full:
                say(f"   n_sim {n_sim:3d}: K {f[0]:2d} full / K {f[0]:2d} games/s = {got[f, n_sim][0] / got[f[0], n_sim][0]:.3f}, examples/s "
                    f"{got[f, n_sim][1] / got[f[0], n_sim][1]:.3f}, collisions {COLL['c', f, n_sim]:.3f} of the simulations")
        if 100 in sims and a.full != "1":
            for n_sim in (x for x in sims if x < 100):
                for k in Ks:
                    say(f"   gumbel K {k:2d} at n_sim {n_sim} against plain at 100: {got[k, n_sim][0] / got[False, 100][0]:.2f}x the games/s, "
                        f"{got[k, n_sim][1] / got[False, 100][1]:.2f}x the examples/s (fewer simulations per move, not a faster kernel)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
