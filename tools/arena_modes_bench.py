"""Times BatchedArena in the search modes and records a strength table (the record is profiles/r16_arena_modes.txt).

  python tools/arena_modes_bench.py cost [rounds] [repeats]      Othello 8x8, network against network: ms per match on the default path,
                                                                 with leaf_batch 4 / 8, and with Gumbel m = 16 at 16 / 32 / 100
                                                                 simulations, gumbel_batch 1 / 4 / 16, gumbel_full off / on; and the
                                                                 share of a match spent outside the search calls
  python tools/arena_modes_bench.py strength [rounds] [seed] [iterations]
                                                                 Othello 6x6, one fixed network on both sides (seeded random weights, or
                                                                 a trainer checkpoint of `iterations` iterations), opening_plies = 4:
                                                                 Gumbel (m = 16, full off / on) at 16 simulations against PUCT at 16 and
                                                                 100; wins, draws and losses per starting colour.  A record, no claim.
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from alphazero_amd.arena import BatchedArena
from alphazero_amd.engine import SelfPlayEngine
from alphazero_amd.games.othello import OthelloConfig, OthelloNet

# the calls of a ply, by the part of the match they belong to; what is left of the wall time is set-up (network upload, engines)
PARTS = {"search": ("search", "search_begin", "search_end"), "status": ("root_status",),
         "moves": ("best_moves", "player_moves", "baseline_moves"), "play": ("play",), "switch": ("set_gumbel",)}


class Clock:
    """wall time spent inside the engine calls of PARTS while it is installed (the calls synchronise: host time is device time)"""

    def __init__(self):
        self.t = {k: 0.0 for k in PARTS}
        self._saved = {}

    def __enter__(self):
        for part, names in PARTS.items():
            for name in names:
                fn = getattr(SelfPlayEngine, name)
                self._saved[name] = fn
                setattr(SelfPlayEngine, name, self._timed(fn, part))
        return self

    def _timed(self, fn, part):
        def call(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.t[part] += time.perf_counter() - t0
        return call

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(SelfPlayEngine, name, fn)


def match(nets, rounds, n_sim, opp_sim=None, board_size=8, seed=3, **kw):
    """one arena: (wall seconds, seconds per part, (wins, losses, draws), stats)"""
    ar = BatchedArena("othello", nets[0], opponent=nets[1], n_sim=n_sim, opponent_n_sim=opp_sim, seed=seed, board_size=board_size, **kw)
    torch.cuda.synchronize()
    with Clock() as ck:
        t0 = time.perf_counter()
        st = ar.play_games(rounds, shard=False)
        dt = time.perf_counter() - t0
    return dt, ck.t, (len(st["player1"]), len(st["player2"]), st["draw"]), st


def line(name, runs):
    """min and spread of the repeats; the split of the fastest one"""
    dts = sorted(r[0] for r in runs)
    dt, parts = min(runs, key=lambda r: r[0])[:2]
    loop = sum(parts.values())
    glue = parts["status"] + parts["moves"] + parts["play"] + parts["switch"]
    print(f"{name:44s} {1e3 * dts[0]:8.1f} ms/match (max {1e3 * dts[-1]:8.1f}, n={len(dts)})  search {1e3 * parts['search']:7.1f}  status "
          f"{1e3 * parts['status']:6.1f}  moves {1e3 * parts['moves']:6.1f}  play {1e3 * parts['play']:6.1f}  set-up {1e3 * (dt - loop):6.1f}  "
          f"outside search: {100 * glue / loop:4.1f}% of the plies, {100 * (dt - parts['search']) / dt:4.1f}% of the match  {runs[0][2]}", flush=True)


def cost(rounds, repeats):
    cfg = OthelloConfig(board_size=8)
    nets = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        nets.append(OthelloNet(config=cfg).to("cuda").eval())
    match(nets, rounds, 16)  # warm-up: module load, first captures
    cases = [("default path @100", 100, {}), ("search={} (player_moves) @100", 100, dict(search={}, opponent_search={}))]
    cases += [(f"leaf_batch {k} @100", 100, dict(search={"leaf_batch": k}, opponent_search={"leaf_batch": k})) for k in (4, 8)]
    for n in (16, 32, 100):
        for full in (False, True):
            for K in (1, 4, 16):
                spec = {"gumbel": 16, "gumbel_batch": K, "gumbel_full": full}
                cases.append((f"gumbel m16 K{K} full={'on' if full else 'off'} @{n}", n, dict(search=spec, opponent_search=spec)))
    for name, n, kw in cases:
        line(name, [match(nets, rounds, n, **kw) for _ in range(repeats)])


def trained_net(seed, iterations):
    """a trainer checkpoint of a few iterations: Othello 6x6, self-play with the Gumbel search at 16 simulations"""
    from alphazero_amd.trainer import AlphaZeroTrainer
    tr = AlphaZeroTrainer(verbose=False, engine_slots=512, seed=seed, materialize_memory=False, selfplay_gumbel=16, selfplay_gumbel_batch=4)
    tr.game = "othello"
    tr.config = OthelloConfig(board_size=6, simulations=16, episodes=512, epochs=2, batch_size=64, iterations=iterations, do_eval=False, device="cuda")
    torch.manual_seed(seed)
    tr.setup()
    t0 = time.perf_counter()
    for it in range(iterations):
        tr.self_play(it); tr.optimize_network(it); tr.update_network(it)
    print(f"network: OthelloNet 6x6 after {iterations} trainer iterations (512 self-play games each at 16 simulations, selfplay_gumbel 16, "
          f"selfplay_gumbel_batch 4, 2 epochs of batch 64, seed {seed}; {time.perf_counter() - t0:.1f} s), the same on both sides", flush=True)
    return tr.nn.to("cuda").eval()


def strength(rounds, seed, iterations=0):
    if iterations > 0:
        net = trained_net(seed, iterations)
    else:
        torch.manual_seed(seed)
        net = OthelloNet(config=OthelloConfig(board_size=6)).to("cuda").eval()
        print(f"network: OthelloNet 6x6, seeded random weights (torch.manual_seed({seed})), the same on both sides", flush=True)
    print(f"{rounds} rounds, opening_plies 4, arena seed {seed}", flush=True)
    for full in (False, True):
        for opp_sim in (16, 100):
            spec = {"gumbel": 16, "gumbel_full": full}
            dt, _, _, st = match((net, net), rounds, 16, opp_sim=opp_sim, board_size=6, seed=seed, search=spec, opening_plies=4)
            print(f"gumbel m16 full={'on' if full else 'off'} @16 vs PUCT @{opp_sim}: Gumbel wins {len(st['player1'])}, loses {len(st['player2'])}, "
                  f"draws {st['draw']};  Gumbel starts {dict(st['player1_starts'])}  PUCT starts {dict(st['player2_starts'])}  "
                  f"(win / loss: the starter's; {dt:.2f} s)", flush=True)
    dt, _, _, st = match((net, net), rounds, 16, opp_sim=16, board_size=6, seed=seed, search={}, opening_plies=4)
    print(f"PUCT @16 vs PUCT @16 (the same player twice): player 1 wins {len(st['player1'])}, loses {len(st['player2'])}, draws {st['draw']};  "
          f"player 1 starts {dict(st['player1_starts'])}  player 2 starts {dict(st['player2_starts'])}", flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "cost"
    if what == "cost":
        cost(int(sys.argv[2]) if len(sys.argv) > 2 else 64, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    elif what == "strength":
        strength(int(sys.argv[2]) if len(sys.argv) > 2 else 256, int(sys.argv[3]) if len(sys.argv) > 3 else 1,
                 int(sys.argv[4]) if len(sys.argv) > 4 else 0)
    else:
        sys.exit(__doc__)
