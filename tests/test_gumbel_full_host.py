"""The full Gumbel search without a GPU: the host model of the contract (tests/gumbel_full_model.py), the pure
restatement of the non-root choice (gumbel.nonroot_choice) and the argument checks of the Python surface."""
import os
import re

import numpy as np
import pytest

from alphazero_amd import gumbel as G
from conftest import ROOT
from gumbel_batch_model import GumbelBatchModel, wide_root
from gumbel_full_model import GumbelFullModel
from gumbel_model import pass_position, playout
from leaf_batch_model import make_board


def tree(node):
    return (node.act, node.N, float(node.Q).hex(), float(node.P).hex(), node.evaluated, node.expanded, node.terminal, node.win,
            [tree(c) for c in node.children])


def ttt_ply4():
    rng = np.random.default_rng(17)
    b = None
    while b is None:
        b = playout("tictactoe", 3, 3, rng, 4)
    return b


def nodes(root):
    out, stack = [], [root]
    while stack:
        x = stack.pop()
        out.append(x)
        stack.extend(x.children)
    return out


# ---- full=False is GumbelBatchModel
@pytest.mark.parametrize("name", ["othello8", "tictactoe"])
def test_switched_off_the_model_is_the_batch_model(name):
    board = make_board("othello", 8, 8) if name == "othello8" else ttt_ply4()
    for m, K, tie in ((4, 1, "lowest"), (16, 4, "random"), (16, 16, "lowest")):
        a = GumbelBatchModel(board, K=K, m=m, tie=tie, seed=3, game_id=11)
        b = GumbelFullModel(board, K=K, full=False, m=m, tie=tie, seed=3, game_id=11)
        for n in (16, 7):
            a.search(n)
            b.search(n)
            assert tree(a.root) == tree(b.root) and a.considered() == b.considered() and a.move() == b.move()
            assert np.array_equal(a.policy().view(np.uint32), b.policy().view(np.uint32))
            assert (a.rows, a.dups, a.plan) == (b.rows, b.dups, b.plan)
            assert [[st for st, _ in step] for step in a.leaves] == [[st for st, _ in step] for step in b.leaves]
        assert a.advance() == b.advance()
        a.search(16)
        b.search(16)
        assert tree(a.root) == tree(b.root) and b.nval == {}


def test_switched_on_the_search_is_another_one():
    board = make_board("othello", 8, 8)
    a = GumbelBatchModel(board, K=1, m=4, seed=3, game_id=11)
    b = GumbelFullModel(board, K=1, m=4, seed=3, game_id=11)
    a.search(50)
    b.search(50)
    assert a.root.N == b.root.N == 50 and tree(a.root) != tree(b.root)


# ---- a fresh node
def test_a_fresh_node_reads_its_own_value_and_its_priors():
    for board in (make_board("othello", 8, 8), wide_root(16), ttt_ply4(), make_board("connect4", 6, 7)):
        m = GumbelFullModel(board, K=1, m=16, seed=3, game_id=5)
        m._evaluate(m.root)
        root = m.root
        vhat = m.root_value()
        assert m._vmix(root) == vhat and vhat == float(np.float32(vhat))
        pi = m.improved_policy(root)
        # no child visited: every completed Q is vhat, the softmax is shift-invariant up to the rounding of log and exp
        tot = sum(c.P for c in root.children)
        assert max(abs(p - c.P / tot) for p, c in zip(pi, root.children)) < 1e-12
        # the first pick is the highest prior, the lowest index among equals
        first = G.nonroot_choice(pi, [0] * len(pi))
        best = max(pi)
        assert first == pi.index(best) and root.children[first].P >= max(c.P for c in root.children) - 1e-12
    assert G.nonroot_choice([0.25, 0.25, 0.25, 0.25], [0, 0, 0, 0]) == 0
    assert G.nonroot_choice([0.2, 0.3, 0.3, 0.2], [0, 0, 0, 0]) == 1
    assert G.nonroot_choice([0.5, 0.5], [1, 0]) == 1 and G.nonroot_choice([0.5, 0.5], [1, 0], [0, 1]) == 0
    assert G.nonroot_choice([float("nan"), 0.5], [0, 0]) == 1
    with pytest.raises(ValueError, match="NaN"):
        G.nonroot_choice([float("nan")] * 3, [0, 0, 0])


def test_vmix_mixes_the_nodes_value_with_its_visited_children():
    m = GumbelFullModel(make_board("othello", 8, 8), K=1, m=4, seed=3, game_id=5)
    m.search(16)
    root = m.root
    num = den = 0.0
    for c in root.children:
        if c.N > 0:
            num += c.P * c.Q
            den += c.P
    sumN = sum(c.N for c in root.children)
    assert sumN == 16 and m._vmix(root) == (m.root_value() + 16.0 * (num / den)) / 17.0
    # below the root too: a visited child's vmix mixes the child's own value with its children's
    child = max(root.children, key=lambda c: c.N)
    assert child.expanded and sum(c.N for c in child.children) == child.N - 1
    assert m._vmix(child) != m.value_of(child) and abs(sum(m.improved_policy(child)) - 1.0) < 1e-12


# ---- nonroot_choice tracks pi
def priors():
    rng = np.random.default_rng(23)
    for n in (2, 3, 5, 8, 16, 17, 33, 40):
        yield "uniform", [1.0 / n] * n
        d = [2.0 ** -(i + 1) for i in range(n)]
        d[-1] = d[-2] if n > 1 else 1.0
        yield "dyadic", d
        yield "skewed", list(rng.dirichlet(np.full(n, 0.3)))
        yield "skewed", list(rng.dirichlet(np.full(n, 3.0)))
        yield "dominant", [0.97] + [0.03 / (n - 1)] * (n - 1)


def test_the_nonroot_choice_tracks_the_policy():
    """from zero counts, over 256 picks, max_a |N(a) - t pi(a)| < 2 at every step t (a survey of 23 000 such priors gave 1.38)"""
    worst = 0.0
    for kind, pi in priors():
        s = sum(pi)
        pi = [p / s for p in pi]
        N = [0] * len(pi)
        for t in range(1, 257):
            N[G.nonroot_choice(pi, N)] += 1
            worst = max(worst, max(abs(n - t * p) for n, p in zip(N, pi)))
            assert worst < 2.0, (kind, len(pi), t, worst)
    print("worst deviation", worst)


# ---- counts
@pytest.mark.parametrize("K", [1, 4, 16])
def test_every_root_grows_by_n_and_the_counters_add_up(K):
    for board in (make_board("othello", 8, 8), wide_root(16), pass_position(8), ttt_ply4(), make_board("connect4", 6, 7)):
        for m in (4, 16):
            x = GumbelFullModel(board, K=K, m=m, seed=3, game_id=7)
            for n in (5, 16, 50):
                before, dups = x.root.N, x.dups
                x.search(n)
                assert x.root.N == before + n and sum(c.N for c in x.root.children) == x.root.N
                assert x.plan == G.lockstep_plan(n, min(m, len(x.root.children)), K) and len(x.plan) <= G.locksteps(n, m, K)
                walked = sum(len(step) for step in x.leaves)
                assert walked == n and x.dups - dups == sum(1 for step in x.leaves for st, _ in step if st == "dup")
                every = nodes(x.root)
                evaluated = [v for v in every if v.evaluated]
                assert x.rows == len(evaluated) and x.node_count() == len(every) == 1 + sum(len(v.children) for v in evaluated)
                # every evaluated node holds a value, in float32, and nothing else was stored
                assert {id(v) for v in evaluated} == set(x.nval)
                assert all(x.value_of(v) == float(np.float32(x.value_of(v))) and abs(x.value_of(v)) <= 1.0 for v in evaluated)
                # no collision at one walker; below the root no draw was made: random ties give the same tree
            if K == 1:
                assert x.dups == 0
            y = GumbelFullModel(board, K=K, m=m, tie="random", seed=3, game_id=7)
            for n in (5, 16, 50):
                y.search(n)
            assert tree(y.root) == tree(x.root)


# ---- root_value after advance
def test_the_root_value_after_a_move_is_the_value_recorded_for_that_child():
    checked = 0
    for board, K in ((make_board("othello", 8, 8), 1), (wide_root(16), 16), (ttt_ply4(), 4), (make_board("connect4", 6, 7), 4)):
        m = GumbelFullModel(board, K=K, m=16, seed=3, game_id=9)
        m.search(50)
        child = m.root.children[m.move_index()]
        if child.terminal:  # the move ends the game: no position to evaluate, no root to read
            continue
        checked += 1
        assert child.evaluated
        want = m.value_of(child)
        b = m._board(child)
        probs, v = m.net(b.grid, b.player, m.A)
        assert want == float(np.float32(v))  # the network's row for that position, in the mover's frame
        m.advance()
        assert m.root is child and m.root_value() == want
        m.search(16)
        assert m.root_value() == want and m.root.N >= 16
    assert checked >= 3


# ---- argument checks: ValueError before any device work
def _net():
    from alphazero_amd.games.othello import OthelloNet
    return OthelloNet(n=6, device="cpu")


@pytest.mark.parametrize("bad", [1, 0, None, "yes", 1.0, np.int64(1)])
def test_gumbel_full_values_are_checked_by_every_surface(bad):
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    from alphazero_amd.trainer import AlphaZeroTrainer
    hip = _net()
    with pytest.raises(ValueError, match="gumbel_full"):
        G.check_gumbel_full(bad, 16)
    with pytest.raises(ValueError, match="gumbel_full"):
        MCT(eval_method="neural", nn=hip, gumbel=16, gumbel_full=bad)
    with pytest.raises(ValueError, match="gumbel_full"):
        AlphaZeroPlayer(n_sim=4, nn=hip, gumbel=16, gumbel_full=bad)
    with pytest.raises(ValueError, match="gumbel_full"):
        BatchedAlphaZeroPlayer(n_sim=4, nn=hip, n_slots=2, gumbel=16, gumbel_full=bad)
    with pytest.raises(ValueError, match="gumbel_full"):
        AlphaZeroTrainer(selfplay_gumbel=16, selfplay_gumbel_full=bad)


def test_gumbel_full_refusals_come_before_any_device_work():
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    from alphazero_amd.trainer import AlphaZeroTrainer
    hip = _net()
    for make in (lambda: MCT(eval_method="neural", nn=hip, gumbel_full=True),
                 lambda: AlphaZeroPlayer(n_sim=4, nn=hip, gumbel_full=True),
                 lambda: BatchedAlphaZeroPlayer(n_sim=4, nn=hip, n_slots=2, gumbel_full=True),
                 lambda: AlphaZeroTrainer(selfplay_gumbel_full=True),
                 lambda: G.check_gumbel_full(True, None)):
        with pytest.raises(ValueError, match="gumbel_full=True needs the Gumbel root search"):
            make()
    t = MCT(eval_method="neural", nn=hip, gumbel=4)
    t.gumbel_full = True
    t.gumbel = None
    with pytest.raises(ValueError, match="gumbel_full=True needs"):  # checked again by search, before the device is touched
        t.search(make_board("othello", 6, 6), n_sim=4)
    # allowed: False everywhere, True with the mode, at every gumbel_batch and with the random symmetry; the setting travels
    assert G.check_gumbel_full(False) is False and G.check_gumbel_full(np.bool_(True), 16) is True
    MCT(eval_method="neural", nn=hip, gumbel_full=False)
    MCT(eval_method="neural", nn=hip, symmetry="random", gumbel=16, gumbel_batch=16, gumbel_full=True)
    p = AlphaZeroPlayer(n_sim=4, nn=hip, gumbel=8, gumbel_batch=4, gumbel_full=True)
    assert p.gumbel_full is True and p.clone().gumbel_full is True and p.clone().gumbel_batch == 4
    p.reset()
    assert p.gumbel_full is True and p.mct.gumbel_full is True and p.mct.gumbel == 8
    assert AlphaZeroPlayer(n_sim=4, nn=hip).gumbel_full is False
    assert BatchedAlphaZeroPlayer(n_sim=4, nn=hip, n_slots=2, gumbel=4, gumbel_full=True).gumbel_full is True
    assert AlphaZeroTrainer(selfplay_gumbel=16, selfplay_gumbel_full=True).selfplay_gumbel_full is True
    assert G.parse(16) == (16, 50.0, 0.5, 1.0)  # the spec keeps its 4-tuple: the switch is a separate setting


def test_exports_are_declared_and_listed():
    from alphazero_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_engine_set_gumbel_full\(az_engine \*e, int32_t on\);", hdr)
    assert re.search(r"int az_engine_root_value\(az_engine \*e, int32_t slot, float \*v\);", hdr)
    assert {"az_engine_set_gumbel_full", "az_engine_root_value"} <= set(_lib.SYMBOLS)
    L = _lib.lib()
    assert L.az_engine_set_gumbel_full(None, 1) == _lib.AZ_EINVAL and L.az_engine_root_value(None, 0, None) == _lib.AZ_EINVAL
