"""CPU: how many leaf evaluations of a self-play wave are repeats (the leaf evaluation cache).

Every game of a wave starts from the same position under one set of weights, so the games of a slot group send the same opening
positions through the network again and again.  This tool plays the first plies of `--games` Othello games with the oracle's own search
(orc_mct_*), through a Python evaluator handed to it as oracle.EVAL_FN that logs the board and calls orc_convnet_eval, and prints per
ply the share of evaluations whose exact (board, side to move) was evaluated before:

  later step only   by any game in an EARLIER lock-step (what a cache whose entries become readable one kernel later can serve);
  same step too     also by another game in the SAME lock-step.

A lock-step here is (ply, index of the evaluation within the game's search of that ply): the root-prior evaluation of a fresh root is
index 0, and a simulation that ends on a terminal node makes no evaluation, so late indices can sit one lock-step early.  The workload
is the headline's: OthelloNet(n=8) under torch.manual_seed(0), Dirichlet 0.03 / 0.25, Philox noise, random tie-break, temperature 1 for
plies 0 .. 4 and 0 after, game ids 0 .. games - 1, 100 simulations per move.

    python tools/eval_cache_count.py --games 1024 --plies 14 --stone-limit 12
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O  # noqa: E402


class LoggedMCT(O.MCT):
    """the oracle's tree with `evaluator` = ("conv", ConvNet) reached through a Python callback: log[] gets (grid bytes, player) of
    every evaluation, in order.  Outputs are memoised by position -- the network is a pure function of it -- which changes no result."""

    def __init__(self, evaluator, memo, alpha=0.03, eps=0.25, tie_mode=O.TIE_RANDOM, noise_mode=O.NOISE_PHILOX, seed=0, game_id=0):
        kind, net = evaluator
        assert kind == "conv"
        self._net, self.log = net, []
        inner = O.EVAL_FN(O.fn_ptr("orc_convnet_eval").value)
        A = net.A

        def logged(ctx, board, probs, value):
            b = board.contents
            key = (C.string_at(b.grid, b.H * b.W), int(b.player))
            self.log.append(key)
            hit = memo.get(key)
            if hit is None:
                inner(net.h, board, probs, value)
                memo[key] = (np.ctypeslib.as_array(probs, (A,)).copy(), float(value[0]))
            else:
                C.memmove(probs, hit[0].ctypes.data, 4 * A)
                value[0] = hit[1]

        self._cb = O.EVAL_FN(logged)  # kept alive with the tree
        cfg = O.MctCfg()
        cfg.eval_method = O.EVAL_NEURAL
        cfg.eval = C.cast(self._cb, C.c_void_p)
        cfg.eval_ctx = None
        cfg.dirichlet_alpha, cfg.dirichlet_epsilon = alpha, eps
        cfg.tie_mode, cfg.noise_mode, cfg.seed, cfg.game_id = tie_mode, noise_mode, seed, game_id
        self.h = O.lib().orc_mct_create(C.byref(cfg))


def stones(key):
    return sum(1 for v in key[0] if v != 0)


def logged_openings(evaluator, games, plies, n_sim, seed=0, first_game_id=0, temp_max_step=4, temp_min_step=4, max_root_stones=None):
    """the first `plies` plies of oracle.selfplay's games, move for move (orc_selfplay's loop): evals[game][ply] = the logged
    evaluations of that ply's search.  max_root_stones: a game stops being followed once its root holds more stones (no leaf below it
    can be within that stone limit)."""
    L, memo, out = O.lib(), {}, []
    for g in range(games):
        t = LoggedMCT(evaluator, memo, seed=seed, game_id=first_game_id + g)
        b = O.new_board(O.OTHELLO, 8, 8)
        per_ply = []
        for ply in range(plies):
            if L.orc_is_over(C.byref(b)):
                break
            if max_root_stones is not None and sum(1 for v in b.grid[:64] if v != 0) > max_root_stones:
                break
            temp = 1.0 if ply <= temp_max_step else (0.0 if ply >= temp_min_step else 1.0 - (ply - temp_max_step) / (temp_min_step - temp_max_step))
            t.set_ply(ply)
            t.log = []
            t.search(b, n_sim)
            per_ply.append(t.log)
            act, _, _ = t.choose(b, temp)
            if L.orc_play(C.byref(b), act) != 0:
                raise RuntimeError("the oracle refused its own move")
            t.change_root(act)
        out.append(per_ply)
    return out


def count(evals, plies, stone_limit):
    """per ply: (evaluations, hits by an earlier lock-step, hits by an earlier or the same lock-step), leaves within the stone limit only
    counting as hits; and the distinct positions within the limit"""
    seen_before, rows = set(), []
    for ply in range(plies):
        n = later = same = 0
        steps = max((len(g[ply]) for g in evals if len(g) > ply), default=0)
        for k in range(steps):
            this_step = set()
            for g in evals:
                if len(g) <= ply or len(g[ply]) <= k:
                    continue
                key = g[ply][k]
                n += 1
                if stones(key) > stone_limit:
                    continue
                if key in seen_before:
                    later += 1
                    same += 1
                elif key in this_step:
                    same += 1
                this_step.add(key)
            seen_before |= this_step
        rows.append((n, later, same))
    return rows, len(seen_before)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--plies", type=int, default=14)
    ap.add_argument("--stone-limit", type=int, default=12)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    from alphazero_amd.games.othello import OthelloNet
    torch.manual_seed(0)
    net = OthelloNet(n=8).eval()
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    evals = logged_openings(("conv", O.ConvNet(O.OTHELLO, 8, 8, sd)), a.games, a.plies, a.sims, seed=a.seed)
    rows, distinct = count(evals, a.plies, a.stone_limit)
    print(f"{a.games} games, {a.sims} sims, stone limit {a.stone_limit}: {sum(r[0] for r in rows)} evaluations, {distinct} distinct positions within the limit")
    print("ply  evals  hit later-step-only  hit same-step-too  rows left per lock-step of the group (later / same)")
    plies_later = plies_same = 0.0
    for ply, (n, later, same) in enumerate(rows):
        if n == 0:
            continue
        plies_later += later / n
        plies_same += same / n
        print(f"{ply:3d} {n:6d} {100.0 * later / n:8.1f} % {100.0 * same / n:8.1f} %   {a.games * (1 - later / n):7.1f} / {a.games * (1 - same / n):7.1f}")
    print(f"plies' worth of repeats per game: {plies_later:.2f} (later step only), {plies_same:.2f} (same step too)")


if __name__ == "__main__":
    main()
