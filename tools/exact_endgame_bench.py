"""What exact endgames cost and buy in the self-play wave (az_engine_set_exact_endgame), at the headline shape:
Othello 8x8, random-init OthelloNet on the HIP network, 4096 slots, 100 simulations.  On one box the legs E = 0 (off) / 4 / 6 / 8 are
run in turn, --rounds times over, so that drift of the box hits every leg alike.  Per leg:
  games/s               whole SelfPlayEngine.run waves, wall clock, the first wave of a leg (plain launches, graph capture) not timed;
  rows saved            1 - (network rows per ply of the leg) / (network rows per ply with the mode off): a solved leaf takes no row;
  solver nodes / leaf   az_engine_exact_endgame_stats: positions the solver entered per solved leaf.
The lock-step waits for its slowest solve, so whether E gains or loses games/s is a measurement, not a promise.
k_step against k_step_exact, us per launch: --trace E runs that one leg alone and writes nothing, for
    rocprofv3 --kernel-trace --stats -- python tools/exact_endgame_bench.py --trace 6
whose per-kernel means go into the record by hand (--kernel-us "k_step=..,k_step_exact=..").
usage: python tools/exact_endgame_bench.py [--out profiles/r27_exact_endgame.txt] [--legs 0,4,6,8] [--rounds 2] [--waves 2]
       [--games 4096] [--sims 100] [--trace E] [--kernel-us TEXT]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_amd import engine as E  # noqa: E402
from alphazero_amd.games.othello import OthelloNet  # noqa: E402

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def hip_net(games):
    torch.manual_seed(0)
    net = OthelloNet(n=8).eval()
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    return E.HipNet(0, 8, 8, sd, max_batch=games)


def leg(hip, e, games, sims, waves, first_id):
    """-> [(games/s, rows per ply, solved leaves per ply, solver nodes per solved leaf)] of `waves` timed waves"""
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=games, n_sim=sims, net=hip, seed=3)
    eng.set_exact_endgame(e or None)
    out = []
    for i in range(waves + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.run(games, first_game_id=first_id + i * games)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        st, xs, cs = eng.stats(), eng.exact_endgame_stats(), eng.eval_cache_stats()
        assert st["games_done"] == games and st["error_flags"] == 0
        if i >= 1:
            rows = st["net_evals"] - cs["cache_hits"]
            out.append((games / dt, rows / st["plies"], xs["solved_leaves"] / st["plies"],
                        xs["solver_nodes"] / max(1, xs["solved_leaves"])))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r27_exact_endgame.txt")
    ap.add_argument("--legs", default="0,4,6,8")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--waves", type=int, default=2)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--trace", type=int, default=None)
    ap.add_argument("--kernel-us", default="")
    a = ap.parse_args()
    hip = hip_net(a.games)
    if a.trace is not None:
        leg(hip, a.trace, a.games, a.sims, 1, 0)
        return
    legs = [int(x) for x in a.legs.split(",")]
    res = {e: [] for e in legs}
    say(f"exact endgames in the self-play wave: Othello 8x8, {a.games} slots, {a.sims} simulations, random-init OthelloNet; "
        f"{torch.cuda.get_device_name(0)}")
    say(f"legs E = {legs} in turn, {a.rounds} rounds of {a.waves} timed waves each (one untimed wave first)")
    for r in range(a.rounds):
        for e in legs:
            got = leg(hip, e, a.games, a.sims, a.waves, (r * len(legs) + legs.index(e)) * (a.waves + 1) * a.games)
            res[e] += got
            say(f"  round {r} E={e}: " + "  ".join(f"{g:8.1f} games/s" for g, _, _, _ in got))
    base_rows = statistics.mean(x[1] for x in res[0]) if 0 in res else None
    say("")
    say(f"{'E':>3} {'games/s median':>15} {'min':>9} {'max':>9} {'vs off':>8} {'rows/ply':>10} {'rows saved':>11} {'solved/ply':>11} {'nodes/leaf':>11}")
    base = statistics.median(x[0] for x in res[0]) if 0 in res else None
    for e in legs:
        g = [x[0] for x in res[e]]
        rows = statistics.mean(x[1] for x in res[e])
        say(f"{e:>3} {statistics.median(g):>15.1f} {min(g):>9.1f} {max(g):>9.1f} "
            f"{(statistics.median(g) / base - 1) * 100 if base else float('nan'):>+7.2f}% {rows:>10.2f} "
            f"{(1 - rows / base_rows) * 100 if base_rows else float('nan'):>10.2f}% {statistics.mean(x[2] for x in res[e]):>11.3f} "
            f"{statistics.mean(x[3] for x in res[e]):>11.1f}")
    say("")
    say("step kernels, us per launch (rocprofv3 --kernel-trace --stats on --trace legs): " + (a.kernel_us or "not yet measured on the GPU"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
