"""leaf_batch (several leaves per lock-step, virtual loss) without a GPU: the host model of the contract (tests/leaf_batch_model.py)
pinned on the golden G3 trees at K = 1, the separation virtual loss buys at K = 8, and the argument checks of the Python surface."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, TAGS, golden
from leaf_batch_model import Model, make_board

MCT_TAGS = ["othello8", "othello6", "connect4", "tictactoe"]
N_POS = 6  # positions per tag, each with and without noise (the whole fixture holds 32: the model is plain Python)


@pytest.mark.parametrize("tag", MCT_TAGS)
def test_model_k1_reproduces_golden_trees(tag):
    """K = 1 is the reference's sequential search: every stage of the G3 records (1, 2, 10, 100 simulations, then the temperature-0
    move and 100 more on the kept subtree), N exact, Q and P within 1e-12"""
    game, gid, H, W, A, n = TAGS[tag]
    fx = golden(f"mct_{tag}.npz")
    ro, stage = fx["row_off"], fx["stage"]
    starts = [s for s in np.flatnonzero(stage == 0)][: 2 * N_POS]
    assert {int(fx["noise"][s]) for s in starts} == {0, 1}

    def check(m, rec):
        sl = slice(ro[rec], ro[rec + 1])
        got = m.root_children()
        assert [c[0] for c in got] == list(fx["action"][sl]), (tag, rec)
        assert [c[1] for c in got] == list(fx["N"][sl]), (tag, rec)
        assert m.root.N == fx["rootN"][rec]
        assert np.abs(np.array([c[2] for c in got]) - fx["Q"][sl]).max() <= 1e-12
        assert np.abs(np.array([c[3] for c in got]) - fx["P"][sl]).max() <= 1e-12

    for s in starts:
        m = Model(make_board(game, H, W, fx["grids"][s], fx["players"][s]), K=1, noise=(0.03, 0.25) if fx["noise"][s] else None)
        for k, sims in enumerate((1, 1, 8, 90)):
            m.search(sims)
            check(m, s + k)
        moved = m.advance()
        if s + 4 < len(stage) and stage[s + 4] == 4:
            assert moved == fx["moved"][s + 4]
            m.search(100)
            check(m, s + 4)


def test_virtual_loss_separates_walkers():
    """Othello 8x8 from the start, lowest-index ties, no noise: along 12 plies of the K = 1 search's most visited moves (64
    simulations per ply) a K = 8 search of every position sends at most a tenth of its walkers onto a leaf that an earlier walker of
    the lock-step already holds.  Without the virtual counts every walker of a lock-step but the first would (share 7/8)."""
    n_sim, dups, total = 64, 0, 0
    line = Model(make_board("othello", 8, 8), K=1)
    for ply in range(12):
        b = line.root.board
        m8 = Model(b, K=8)
        m8.search(n_sim)
        assert m8.root.N == n_sim
        dups += m8.dups
        total += n_sim
        line.search(n_sim)
        line.advance()
    print(f"duplicate share at K = 8: {dups}/{total} = {dups / total:.4f}")
    assert dups / total <= 0.10, (dups, total)
    b = line.root.board
    for K in (1, 2, 3, 8, 16):
        m = Model(b, K=K)
        m.search(50)  # ragged last lock-step for 3, 8 and 16
        assert m.root.N == 50 and sum(c[1] for c in m.root_children()) == 50  # a root with priors: every simulation enters a child
        assert m.rows + m.dups <= 50 + 1 and (K > 1 or m.dups == 0)


def test_model_k_above_one_departs_and_split_matters():
    """the documented consequences: K > 1 is another search than K = 1, and for K > 1 search(3); search(5) walks [3] [4, 1]
    where search(8) walks [4, 4]"""
    b = make_board("othello", 6, 6)
    a, c, d = Model(b, K=4), Model(b, K=4), Model(b, K=1)
    a.search(3); a.search(5)
    c.search(8)
    d.search(8)
    assert a.root.N == c.root.N == d.root.N == 8
    assert a.rows != c.rows or a.root_children() != c.root_children()
    assert c.root_children() != d.root_children()


# ---- argument checks: ValueError before any device work (no library is loaded)
def _nets():
    from alphazero_amd.games.othello import OthelloNet

    class Other(OthelloNet):  # evaluate() overridden: evaluators.route sends it to "board"
        def evaluate(self, board):
            return super().evaluate(board)

    class Torchy(OthelloNet):  # forward() overridden: the HIP network does not serve it ("torch")
        def forward(self, x):
            return super().forward(x)
    return OthelloNet(n=6, device="cpu"), Other(n=6, device="cpu"), Torchy(n=6, device="cpu")


@pytest.mark.parametrize("bad", [0, 17, True, 2.5, -1, "4"])
def test_leaf_batch_values_are_checked(bad):
    from alphazero_amd.mcts import MCT, check_leaf_batch
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    hip, _, _ = _nets()
    with pytest.raises(ValueError, match="leaf_batch"):
        check_leaf_batch(bad, hip)
    with pytest.raises(ValueError, match="leaf_batch"):
        MCT(eval_method="neural", nn=hip, leaf_batch=bad)
    with pytest.raises(ValueError, match="leaf_batch"):
        AlphaZeroPlayer(n_sim=4, nn=hip, leaf_batch=bad)
    with pytest.raises(ValueError, match="leaf_batch"):
        BatchedAlphaZeroPlayer(n_sim=4, nn=hip, n_slots=2, leaf_batch=bad)


def test_leaf_batch_needs_the_hip_route_a_neural_tree_and_no_symmetry():
    from alphazero_amd.evaluators import route
    from alphazero_amd.mcts import MCT, check_leaf_batch
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    hip, board_net, torch_net = _nets()
    assert (route(hip), route(board_net), route(torch_net)) == ("hip", "board", "torch")
    assert check_leaf_batch(None, hip) == 1 and check_leaf_batch(1, board_net) == 1 and check_leaf_batch(np.int64(16), hip) == 16
    for nn in (board_net, torch_net):
        with pytest.raises(ValueError, match="external evaluator"):
            MCT(eval_method="neural", nn=nn, leaf_batch=4)
        with pytest.raises(ValueError, match="external evaluator"):
            BatchedAlphaZeroPlayer(n_sim=4, nn=nn, n_slots=2, leaf_batch=4)
        m = MCT(eval_method="neural", nn=hip, leaf_batch=4)
        with pytest.raises(ValueError, match="external evaluator"):
            m.nn = nn
    with pytest.raises(ValueError, match="rollout|neural"):
        MCT(eval_method="rollout", leaf_batch=4)
    with pytest.raises(ValueError, match="symmetry"):
        MCT(eval_method="neural", nn=hip, symmetry="all", leaf_batch=2)
    with pytest.raises(ValueError, match="symmetry"):
        AlphaZeroPlayer(n_sim=4, nn=hip, symmetry=[0, 1], leaf_batch=8)
    # allowed: the default, 1 with anything, and the setting travels through clone() and reset()
    MCT(eval_method="rollout", leaf_batch=1)
    MCT(eval_method="neural", nn=hip, symmetry="all", leaf_batch=1)
    p = AlphaZeroPlayer(n_sim=4, nn=hip, leaf_batch=8)
    assert p.leaf_batch == 8 and p.clone().leaf_batch == 8
    p.reset()
    assert p.leaf_batch == 8 and p.mct.leaf_batch == 8
    assert AlphaZeroPlayer(n_sim=4, nn=hip).leaf_batch is None


def test_exports_are_declared_and_listed():
    from alphazero_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_engine_set_leaf_batch\(az_engine \*e, int32_t k\);", hdr)
    assert re.search(r"int az_engine_collisions\(az_engine \*e, int64_t \*n\);", hdr)
    assert re.search(r"#define AZ_MAX_LEAF_BATCH 16\b", hdr)
    assert "az_engine_set_leaf_batch" in _lib.SYMBOLS and "az_engine_collisions" in _lib.SYMBOLS
    assert _lib.MAX_LEAF_BATCH == 16
