"""Several Sequential Halving leaves per network call without a GPU: the per-slot lock-step plan and the number
of lock-steps the host enqueues, the host model of the contract (tests/gumbel_batch_model.py) and the argument checks of the Python
surface."""
import os
import re

import numpy as np
import pytest

from alphazero_amd import gumbel as G
from conftest import ROOT
from gumbel_batch_model import GumbelBatchModel, wide_root
from gumbel_model import GumbelModel, pass_position, playout
from leaf_batch_model import make_board

PLANS = {(16, 16, 16): [(0, 16)], (16, 9, 16): [(0, 9), (9, 4), (13, 3)], (16, 4, 4): [(0, 4), (4, 4), (8, 4), (12, 4)],
         (7, 4, 4): [(0, 4), (4, 2), (6, 1)], (5, 3, 2): [(0, 2), (2, 1), (3, 2)],
         (24, 5, 4): [(0, 4), (4, 1), (5, 4), (9, 4), (13, 4), (17, 4), (21, 3)],
         (50, 16, 16): [(0, 16), (16, 8), (24, 12), (36, 12), (48, 2)]}
LMAX = {(16, 16, 16): 4, (16, 16, 8): 4, (16, 4, 4): 5, (32, 16, 16): 5, (50, 16, 16): 5, (100, 16, 16): 9, (100, 16, 8): 14,
        (200, 7, 16): 16, (7, 4, 4): 3}


def test_plan_and_lockstep_count_reproduce_the_contracts_tables():
    for args, want in PLANS.items():
        assert G.lockstep_plan(*args) == want, args
    for args, want in LMAX.items():
        assert G.locksteps(*args) == want, args
    assert max(G.locksteps(n, 16, K) - (n + K - 1) // K for n in range(1, 201) for K in range(1, 17)) == 4
    # a root without children takes the m0 = 1 plan
    assert G.lockstep_plan(9, 0, 4) == G.lockstep_plan(9, 1, 4) == [(0, 4), (4, 4), (8, 1)]
    assert G.lockstep_plan(0, 4, 4) == [] and G.locksteps(0, 16, 4) == 0


def test_plans_deal_n_and_never_cross_a_phase():
    for n in range(1, 65):
        for m0 in range(1, 17):
            bounds, e = set(), 0
            for mp, v in G.schedule(n, m0):
                e += mp * v
                bounds.add(e)
            assert G.lockstep_plan(n, m0, 1) == [(s, 1) for s in range(n)], (n, m0)
            for K in range(1, 17):
                plan = G.lockstep_plan(n, m0, K)
                assert sum(kt for _, kt in plan) == n and all(1 <= kt <= K for _, kt in plan), (n, m0, K)
                assert [s for s, _ in plan] == [sum(kt for _, kt in plan[:i]) for i in range(len(plan))]
                for s, kt in plan:
                    assert not any(s < b < s + kt for b in bounds), (n, m0, K, s, kt)
                    assert G.locate(s, n, m0)[0] == G.locate(s + kt - 1, n, m0)[0]
                    # as long as the contract's minimum allows: a shorter lock-step ends on a phase boundary or at n
                    assert kt == K or s + kt == n or s + kt in bounds, (n, m0, K, s, kt)
                assert len(plan) <= G.locksteps(n, max(m0, 1), K)


def test_the_librarys_lockstep_count_is_pythons():
    from alphazero_amd import _lib
    L = _lib.lib()
    for n in (0, 1, 5, 7, 16, 24, 32, 50, 100, 200):
        for m in range(1, 17):
            for K in range(1, 17):
                assert L.az_gumbel_locksteps(n, m, K) == G.locksteps(n, m, K), (n, m, K)
    for bad in ((-1, 4, 4), (16, 0, 4), (16, 17, 4), (16, 4, 0), (16, 4, 17)):
        assert L.az_gumbel_locksteps(*bad) == -1


def tree(node):
    return (node.act, node.N, float(node.Q).hex(), float(node.P).hex(), node.evaluated, node.expanded, node.terminal, node.win,
            [tree(c) for c in node.children])


def ttt_ply4():
    rng = np.random.default_rng(17)
    b = None
    while b is None:
        b = playout("tictactoe", 3, 3, rng, 4)
    return b


@pytest.mark.parametrize("name", ["othello8", "tictactoe"])
def test_batch_model_at_one_walker_is_the_gumbel_model(name):
    board = make_board("othello", 8, 8) if name == "othello8" else ttt_ply4()
    for m, tie in ((4, "lowest"), (16, "random")):
        a = GumbelModel(board, m=m, tie=tie, seed=3, game_id=11)
        b = GumbelBatchModel(board, K=1, m=m, tie=tie, seed=3, game_id=11)
        for n in (16, 7):
            a.search(n)
            b.search(n)
            assert tree(a.root) == tree(b.root) and a.considered() == b.considered() and a.move() == b.move()
            assert np.array_equal(a.policy().view(np.uint32), b.policy().view(np.uint32))
            assert (a.rows, a.dups) == (b.rows, b.dups) and b.plan == [(s, 1) for s in range(n)]
        assert a.advance() == b.advance()
        a.search(16)
        b.search(16)
        assert tree(a.root) == tree(b.root)


def test_one_lockstep_searches_a_wide_root():
    board = wide_root()
    assert len(board.get_moves()) >= 16
    m = GumbelBatchModel(board, K=16, m=16, seed=3, game_id=5)
    m.search(16)
    assert m.plan == [(0, 16)] and len(m.leaves) == 1
    assert [st for st, _ in m.leaves[0]] == ["eval"] * 16 and len({x for _, x in m.leaves[0]}) == 16
    assert m.dups == 0 and m.rows == 17 and m.root.N == 16
    assert sorted(c.N for c in m.root.children)[-16:] == [1] * 16 and len(m.considered()) == 16


def test_a_narrow_root_follows_its_own_plan_and_collides_on_pending_leaves():
    m = GumbelBatchModel(make_board("othello", 8, 8), K=16, m=16, seed=3, game_id=5)
    m.search(16)
    assert m.plan == G.lockstep_plan(16, 4, 16) == [(0, 8), (8, 8)]
    assert m.root.N == 16 and sorted(c.N for c in m.root.children) == [2, 2, 6, 6]
    # the first lock-step visits each of the 4 fresh children twice: 4 rows and 4 duplicates of their pending leaves
    assert [st for st, _ in m.leaves[0]] == ["eval"] * 4 + ["dup"] * 4 and m.dups >= 4
    m.search(16)
    assert m.root.N == 32
    p = GumbelBatchModel(pass_position(8), K=4, m=16, seed=3, game_id=5)
    p.search(7)
    assert p.plan == [(0, 4), (4, 3)] and p.root.N == 7 and len(p.root.children) == 1


@pytest.mark.parametrize("K", [2, 3, 4, 16])
def test_every_root_grows_by_n(K):
    for board in (make_board("othello", 8, 8), wide_root(9), ttt_ply4(), make_board("connect4", 6, 7)):
        for m in (2, 4, 16):
            x = GumbelBatchModel(board, K=K, m=m, seed=3, game_id=7)
            for n in (5, 7, 16, 50):
                before = x.root.N
                x.search(n)
                assert x.root.N == before + n and sum(c.N for c in x.root.children) == x.root.N
                assert x.plan == G.lockstep_plan(n, min(m, len(x.root.children)), K)
                assert len(x.plan) <= G.locksteps(n, m, K)


# ---- argument checks: ValueError before any device work
def _net():
    from alphazero_amd.games.othello import OthelloNet
    return OthelloNet(n=6, device="cpu")


@pytest.mark.parametrize("bad", [0, 17, -1, True, 2.5, "4", None])
def test_gumbel_batch_values_are_checked_by_every_surface(bad):
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    from alphazero_amd.trainer import AlphaZeroTrainer
    hip = _net()
    with pytest.raises(ValueError, match="gumbel_batch"):
        G.check_gumbel_batch(bad, 16)
    with pytest.raises(ValueError, match="gumbel_batch"):
        MCT(eval_method="neural", nn=hip, gumbel=16, gumbel_batch=bad)
    with pytest.raises(ValueError, match="gumbel_batch"):
        AlphaZeroPlayer(n_sim=4, nn=hip, gumbel=16, gumbel_batch=bad)
    with pytest.raises(ValueError, match="gumbel_batch"):
        BatchedAlphaZeroPlayer(n_sim=4, nn=hip, n_slots=2, gumbel=16, gumbel_batch=bad)
    with pytest.raises(ValueError, match="gumbel_batch"):
        AlphaZeroTrainer(selfplay_gumbel=16, selfplay_gumbel_batch=bad)


def test_gumbel_batch_refusals_come_before_any_device_work():
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    from alphazero_amd.trainer import AlphaZeroTrainer
    hip = _net()
    for make in (lambda: MCT(eval_method="neural", nn=hip, gumbel_batch=4),
                 lambda: AlphaZeroPlayer(n_sim=4, nn=hip, gumbel_batch=2),
                 lambda: BatchedAlphaZeroPlayer(n_sim=4, nn=hip, n_slots=2, gumbel_batch=16),
                 lambda: AlphaZeroTrainer(selfplay_gumbel_batch=4)):
        with pytest.raises(ValueError, match="gumbel_batch=.* needs the Gumbel root search"):
            make()
    for make in (lambda: MCT(eval_method="neural", nn=hip, symmetry="all", gumbel=4, gumbel_batch=4),
                 lambda: AlphaZeroPlayer(n_sim=4, nn=hip, symmetry="all", gumbel=4, gumbel_batch=2),
                 lambda: BatchedAlphaZeroPlayer(n_sim=4, nn=hip, n_slots=2, symmetry="all", gumbel=4, gumbel_batch=16)):
        with pytest.raises(ValueError, match="symmetry='all'"):
            make()
    # the leaf_batch x gumbel refusal stands whatever gumbel_batch says
    with pytest.raises(ValueError, match="leaf_batch"):
        MCT(eval_method="neural", nn=hip, leaf_batch=4, gumbel=4, gumbel_batch=4)
    # allowed: 1 everywhere, > 1 with the mode, with the random symmetry and an ensemble at 1; the setting travels
    MCT(eval_method="neural", nn=hip, gumbel_batch=1)
    MCT(eval_method="neural", nn=hip, symmetry="all", gumbel=4, gumbel_batch=1)
    MCT(eval_method="neural", nn=hip, symmetry="random", gumbel=16, gumbel_batch=16)
    assert G.check_gumbel_batch(np.int64(4), 16) == 4
    p = AlphaZeroPlayer(n_sim=4, nn=hip, gumbel=8, gumbel_batch=4)
    assert p.gumbel_batch == 4 and p.clone().gumbel_batch == 4 and p.clone().gumbel == 8
    p.reset()
    assert p.gumbel_batch == 4 and p.mct.gumbel_batch == 4
    assert AlphaZeroPlayer(n_sim=4, nn=hip).gumbel_batch == 1
    assert BatchedAlphaZeroPlayer(n_sim=4, nn=hip, n_slots=2, gumbel=4, gumbel_batch=4).gumbel_batch == 4
    assert AlphaZeroTrainer(selfplay_gumbel=16, selfplay_gumbel_batch=4).selfplay_gumbel_batch == 4
    assert G.parse(16) == (16, 50.0, 0.5, 1.0)  # the spec keeps its 4-tuple: the batch is a separate setting


def test_exports_are_declared_and_listed():
    from alphazero_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_engine_set_gumbel_batch\(az_engine \*e, int32_t k\);", hdr)
    assert re.search(r"int az_gumbel_locksteps\(int32_t n_sim, int32_t m, int32_t k\);", hdr)
    assert {"az_engine_set_gumbel_batch", "az_gumbel_locksteps"} <= set(_lib.SYMBOLS)
    assert G.MAX_GUMBEL_BATCH == _lib.MAX_LEAF_BATCH == 16
