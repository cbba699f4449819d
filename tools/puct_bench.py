"""What the PUCT exploration settings cost, and a first strength table (the record is profiles/r29_puct.txt).
Othello 8x8, 4096 slots, n_sim 100, random-init OthelloNet on the HIP network; the mode off against (1.25, 19652, off), (2.5, 0, off)
and (1.25, 19652, 0.25), the legs alternated in one process series, two rounds.
  a. a 4096-game self-play wave (SelfPlayEngine.run): games/s, samples/s, network rows per game;
  b. the lock-step kernel alone: one search of 4096 fresh roots with the fake evaluator, whose network stand-in is one small kernel, so
     that the time per lock-step is k_step's / k_step_puct's plus the same constant; the same search with the HIP network beside it.
     The difference of two legs is the cost of a k_step_puct launch over a k_step launch;
  c. strength, a record and not a claim: BatchedArena on Othello 6x6, one seeded random-init network on both sides, 16 simulations,
     opening_plies 4, each setting as player 1 against the mode off (tools/arena_modes_bench.py's table), and the mode off against
     itself.
Wall-clock times of calls that block until their results are there; the first wave and the first two searches of an engine (plain
launches, graph capture) are not timed.
usage: python tools/puct_bench.py [--out profiles/r29_puct.txt] [--wave-repeats 1] [--search-repeats 5] [--rounds 256] [--skip a,b,c]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_amd import engine as E  # noqa: E402
from alphazero_amd.arena import BatchedArena  # noqa: E402
from alphazero_amd.games.othello import OthelloBoard, OthelloConfig, OthelloNet  # noqa: E402

LINES = []
GAMES, N_SIM, SEED = 4096, 100, 3
LEGS = [None, (1.25, 19652.0, -1.0), (2.5, 0.0, -1.0), (1.25, 19652.0, 0.25)]


def say(s):
    print(s, flush=True)
    LINES.append(s)


def name(puct):
    return "mode off            " if puct is None else f"({puct[0]:g}, {puct[1]:g}, {'off' if puct[2] < 0 else f'{puct[2]:g}'})".ljust(20)


def spec(puct):
    return None if puct is None else {"c_init": puct[0], "c_base": puct[1], "fpu": puct[2]}


def engine(hip, puct):
    if hip is None:
        eng = E.SelfPlayEngine(0, 8, 8, n_slots=GAMES, n_sim=N_SIM, evaluator=E.EVAL_FAKE, seed=SEED)
    else:
        eng = E.SelfPlayEngine(0, 8, 8, n_slots=GAMES, n_sim=N_SIM, net=hip, seed=SEED)
    eng.set_puct(spec(puct))
    return eng


def wave(hip, puct, repeats):
    """-> [(games/s, samples/s, network rows per game, cache hits per game)] of whole waves after an untimed first one"""
    eng = engine(hip, puct)
    out = []
    for i in range(repeats + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.run(GAMES, first_game_id=i * GAMES)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        st, cs = eng.stats(), eng.eval_cache_stats()
        assert st["games_done"] == GAMES and st["error_flags"] == 0
        if i >= 1:
            out.append((GAMES / dt, st["samples"] / dt, st["net_evals"] / GAMES, cs["cache_hits"] / GAMES))
    groups = eng.groups()
    eng.close()
    return out, groups


def searches(hip, puct, repeats):
    """-> [seconds] of search(N_SIM) on 4096 fresh roots (the start position, game ids 0 .. 4095, ply 0)"""
    eng = engine(hip, puct)
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


def strength(rounds, seed=1):
    torch.manual_seed(seed)
    net = OthelloNet(config=OthelloConfig(board_size=6)).to("cuda").eval()
    say(f"c. strength: OthelloNet 6x6, seeded random weights (torch.manual_seed({seed})), the same on both sides; {rounds} rounds, 16 simulations "
        f"a side, opening_plies 4, arena seed {seed}; player 1 under the settings, player 2 with the mode off")
    for puct in LEGS[1:] + [None]:
        ar = BatchedArena("othello", net, opponent=net, n_sim=16, opponent_n_sim=16, seed=seed, board_size=6,
                          search={} if puct is None else {"puct": spec(puct)}, opening_plies=4)
        t = time.perf_counter()
        st = ar.play_games(rounds, shard=False)
        dt = time.perf_counter() - t
        say(f"   {name(puct)} vs mode off: wins {len(st['player1'])}, loses {len(st['player2'])}, draws {st['draw']};  player 1 starts "
            f"{dict(st['player1_starts'])}  player 2 starts {dict(st['player2_starts'])}  (win / loss: the starter's; {dt:.2f} s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--wave-repeats", type=int, default=1)
    ap.add_argument("--search-repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=256)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    skip = set(a.skip.split(",")) if a.skip else set()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    net = OthelloNet(8, device="cuda")
    net.eval()
    hip = net.to_hip(max_batch=GAMES)
    med = statistics.median
    say(f"python tools/puct_bench.py: Othello 8x8, {GAMES} slots, n_sim {N_SIM}, random-init OthelloNet, {torch.cuda.get_device_name(0)}")
    if "a" not in skip:
        got = {}
        for puct in LEGS + LEGS:  # alternated: the second round shows the spread of a repeat
            r, groups = wave(hip, puct, a.wave_repeats)
            got.setdefault(puct, []).extend(r)
            for g, s, rows, hits in r:
                say(f"a. wave of {GAMES} games, {name(puct)}, {groups} slot groups: {g:8.1f} games/s {s:10.1f} samples/s; "
                    f"{rows:7.1f} leaf evaluations per game, {hits:6.1f} of them from the cache")
        off = med([x[0] for x in got[None]])
        for puct in LEGS:
            say(f"   {name(puct)} runs: {', '.join(f'{x[0]:.1f}' for x in got[puct])} games/s; over the mode off: {med([x[0] for x in got[puct]]) / off:.3f}")
    if "b" not in skip:
        for net_name, h in (("fake evaluator", None), ("HIP network", hip)):
            res = {}
            for puct in LEGS + LEGS:
                res.setdefault(puct, []).extend(searches(h, puct, a.search_repeats))
            off = med(res[None]) / (N_SIM + 1)
            for puct in LEGS:
                on = med(res[puct]) / (N_SIM + 1)
                say(f"b. search of {GAMES} fresh roots, {net_name}, {name(puct)}: {on * 1e6:7.1f} us per lock-step (min "
                    f"{min(res[puct]) / (N_SIM + 1) * 1e6:.1f}, max {max(res[puct]) / (N_SIM + 1) * 1e6:.1f}): {(on - off) * 1e6:+.2f} us per launch over k_step")
    hip.close()
    if "c" not in skip:
        strength(a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
