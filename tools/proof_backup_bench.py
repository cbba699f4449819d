"""What proof backup costs and buys in the self-play wave (az_engine_set_proof_backup), at the headline shape:
Othello 8x8, random-init OthelloNet on the HIP network, 4096 slots, 100 simulations.  On one box the legs
    off | proof (proof backup alone) | E4 (exact endgames at E = 4) | E4+proof
are run in turn, --rounds times over, so that drift of the box hits every leg alike.  Per leg:
  games/s          whole SelfPlayEngine.run waves, wall clock, the first wave of a leg (plain launches, graph capture) not timed;
  rows/ply         network rows per ply (net_evals - cache_hits): a walk that ends on a proven node takes none;
  proven/ply       az_engine_proof_backup_stats: interior nodes marked per ply;  stops/ply: walks ended on a proven node per ply;
  pruned           the share of plies whose policy counts the proofs changed.
The step kernel's time per launch: --trace LEG runs that one leg alone and writes nothing, for
    rocprofv3 --kernel-trace --stats -- python tools/proof_backup_bench.py --trace proof
whose per-kernel mean and maximum go into the record by hand (--kernel-us "k_step=..,k_step_proof=..").
usage: python tools/proof_backup_bench.py [--out profiles/r28_proof_backup.txt] [--legs off,proof,E4,E4+proof] [--rounds 2]
       [--waves 2] [--games 4096] [--sims 100] [--trace LEG] [--kernel-us TEXT]"""
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
LEGS = {"off": (0, False), "proof": (0, True), "E4": (4, False), "E4+proof": (4, True)}


def say(s):
    print(s, flush=True)
    LINES.append(s)


def hip_net(games):
    torch.manual_seed(0)
    net = OthelloNet(n=8).eval()
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    return E.HipNet(0, 8, 8, sd, max_batch=games)


def leg(hip, name, games, sims, waves, first_id):
    """-> [(games/s, rows per ply, proven nodes per ply, proof stops per ply, pruned share of plies)] of `waves` timed waves"""
    e, proof = LEGS[name]
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=games, n_sim=sims, net=hip, seed=3)
    eng.set_exact_endgame(e or None)
    eng.set_proof_backup(proof)
    out = []
    for i in range(waves + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.run(games, first_game_id=first_id + i * games)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        st, ps, cs = eng.stats(), eng.proof_backup_stats(), eng.eval_cache_stats()
        assert st["games_done"] == games and st["error_flags"] == 0
        if i >= 1:
            p = st["plies"]
            out.append((games / dt, (st["net_evals"] - cs["cache_hits"]) / p, ps["proven_nodes"] / p, ps["proof_stops"] / p, ps["pruned_plies"] / p))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r28_proof_backup.txt")
    ap.add_argument("--legs", default="off,proof,E4,E4+proof")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--waves", type=int, default=2)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--kernel-us", default="")
    a = ap.parse_args()
    hip = hip_net(a.games)
    if a.trace is not None:
        leg(hip, a.trace, a.games, a.sims, 1, 0)
        return
    legs = a.legs.split(",")
    res = {n: [] for n in legs}
    say(f"proof backup in the self-play wave: Othello 8x8, {a.games} slots, {a.sims} simulations, random-init OthelloNet; "
        f"{torch.cuda.get_device_name(0)}")
    say(f"legs {legs} in turn, {a.rounds} rounds of {a.waves} timed waves each (one untimed wave first)")
    for r in range(a.rounds):
        for n in legs:
            got = leg(hip, n, a.games, a.sims, a.waves, (r * len(legs) + legs.index(n)) * (a.waves + 1) * a.games)
            res[n] += got
            say(f"  round {r} {n}: " + "  ".join(f"{g[0]:8.1f} games/s" for g in got))
    say("")
    say(f"{'leg':>9} {'games/s median':>15} {'min':>9} {'max':>9} {'vs off':>8} {'rows/ply':>10} {'proven/ply':>11} {'stops/ply':>10} {'pruned':>8}")
    base = statistics.median(x[0] for x in res["off"]) if "off" in res else None
    for n in legs:
        g = [x[0] for x in res[n]]
        mean = [statistics.mean(x[i] for x in res[n]) for i in range(1, 5)]
        say(f"{n:>9} {statistics.median(g):>15.1f} {min(g):>9.1f} {max(g):>9.1f} "
            f"{(statistics.median(g) / base - 1) * 100 if base else float('nan'):>+7.2f}% {mean[0]:>10.2f} {mean[1]:>11.3f} {mean[2]:>10.3f} {mean[3] * 100:>7.2f}%")
    say("")
    say("step kernels, us per launch, mean and maximum (rocprofv3 --kernel-trace --stats on --trace legs): " + (a.kernel_us or "not measured"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
