"""The Gumbel root search without a GPU: the Sequential Halving schedule, the Python restatements of the engine's
deterministic log / exp against the oracle's, the Gumbel-max property of the draw, the host model of the contract
(tests/gumbel_model.py) and the argument checks of the Python surface."""
import math
import os
import re

import numpy as np
import pytest

from alphazero_amd import gumbel as G
from conftest import ROOT
from gumbel_model import GumbelModel
from leaf_batch_model import make_board

TABLE = {(16, 16): [(16, 1)], (16, 4): [(4, 2), (2, 4)], (50, 16): [(16, 1), (8, 1), (4, 3), (2, 6), (2, 6)],
         (100, 16): [(16, 1), (8, 3), (4, 6), (2, 12), (2, 12)], (7, 4): [(4, 1), (2, 1), (2, 1)], (5, 3): [(3, 1), (2, 1)],
         (24, 5): [(5, 1), (2, 4), (2, 4), (2, 4)], (200, 7): [(7, 9), (3, 22), (2, 33), (2, 33)]}


def test_schedule_reproduces_the_contracts_table():
    for (n, m0), want in TABLE.items():
        assert G.schedule(n, m0) == want, (n, m0)
    assert G.schedule(9, 1) == [(1, 9)]


def test_schedule_deals_n_simulations_and_full_phases_are_even():
    for n in range(1, 65):
        for m0 in range(1, 17):
            ph = G.schedule(n, m0)
            assert ph[0][0] == m0 and all(a[0] >= b[0] for a, b in zip(ph, ph[1:]))
            assert sum(mp * v for mp, v in ph[:-1]) < n <= sum(mp * v for mp, v in ph), (n, m0)
            visits, seen = {}, []
            for s in range(n):
                p, mp, i = G.locate(s, n, m0)
                assert mp == ph[p][0] and 0 <= i < mp * ph[p][1]
                visits.setdefault(p, [0] * mp)[i % mp] += 1
                seen.append(p)
            assert seen == sorted(seen) and set(seen) == set(range(len(seen) and seen[-1] + 1))
            for p, (mp, v) in enumerate(ph[:-1]):  # every phase but the last is whole
                assert visits[p] == [v] * mp, (n, m0, p)
            with pytest.raises(ValueError):
                G.locate(n, n, m0)


def test_det_log_and_det_exp_are_bit_equal_to_the_oracle():
    from oracle import oracle as O
    L = O.lib()
    rng = np.random.default_rng(0)
    xs = np.concatenate([np.exp(np.linspace(-700, 700, 1501)), rng.random(1500), [2.0 ** -53, 1.0 - 2.0 ** -53, 1.0, 0.0, -1.0,
                         1.4142135623730951, np.nextafter(1.4142135623730951, 2.0), 5e-324, 1e308]])
    for x in xs:
        a, b = G.det_log(float(x)), L.orc_det_log(float(x))
        assert np.float64(a).view(np.int64) == np.float64(b).view(np.int64), x
    xs = np.concatenate([np.linspace(-720, 10, 1501), -36.8 * rng.random(1500), [0.0, -0.0, -700.0, 700.0, 701.0, -math.inf]])
    for x in xs:
        a, b = G.det_exp(float(x)), L.orc_det_exp(float(x))
        assert np.float64(a).view(np.int64) == np.float64(b).view(np.int64), x
    assert G.det_exp(float("nan")) == 0.0 and G.det_log(0.0) == -math.inf


def test_the_first_candidate_is_a_sample_of_the_prior():
    """Gumbel-max: argmax of g + logit over the actions is distributed as the priors.  chi-square on 8000 games against the
    p = 0.001 point of 4 degrees of freedom (18.47)"""
    pri = [0.4, 0.3, 0.15, 0.1, 0.05]
    logit = [G.det_log(p) for p in pri]
    n = 8000
    cnt = [0] * len(pri)
    for gid in range(n):
        sc = [G.gumbel_g(0, gid, 3, a, 1.0) + logit[a] for a in range(len(pri))]
        cnt[max(range(len(pri)), key=lambda a: sc[a])] += 1
    chi2 = sum((c - n * p) ** 2 / (n * p) for c, p in zip(cnt, pri))
    print("chi2", chi2, cnt)
    assert chi2 < 18.47
    # one draw per (game, ply, action); scale 0 makes none
    assert G.gumbel_g(0, 5, 3, 2, 1.0) == G.gumbel_g(0, 5, 3, 2, 1.0) != G.gumbel_g(0, 5, 4, 2, 1.0)
    assert G.gumbel_g(0, 5, 3, 2, 2.0) == 2.0 * G.gumbel_g(0, 5, 3, 2, 1.0) and G.gumbel_g(0, 5, 3, 2, 0.0) == 0.0


@pytest.mark.parametrize("m", [4, 16])
def test_model_visits_follow_the_schedule(m):
    a = GumbelModel(make_board("othello", 8, 8), m=m, seed=3, game_id=11)
    a.search(16)
    assert sorted(c[1] for c in a.root_children()) == [2, 2, 6, 6] and a.root.N == 16
    assert len(a.considered()) == 2 and sorted(c[1] for i, c in enumerate(a.root_children()) if i in a.considered()) == [6, 6]
    assert a.root.children[a.move_index()].N == 6
    b = GumbelModel(make_board("othello", 8, 8), m=m, seed=3, game_id=11)
    b.search(7)
    assert sorted(c[1] for c in b.root_children()) == [1, 1, 2, 3]


def test_model_without_noise_and_sigma_follows_the_priors():
    board = make_board("othello", 8, 8)
    for _ in range(6):
        board.play_move(sorted(board.get_moves())[0])
    m = GumbelModel(board, m=2, c_scale=0.0, gumbel_scale=0.0)
    m.search(8)
    ch = m.root_children()
    assert len(ch) > 2
    top = sorted(range(len(ch)), key=lambda i: (-ch[i][3], i))[:2]
    assert m.considered() == sorted(top)
    assert m.move() == ch[top[0]][0]
    assert sum(c[1] for c in ch) == 8 and all(c[1] == (4 if i in top else 0) for i, c in enumerate(ch))
    # pi' is the renormalised prior when sigma is switched off, and sums to 1
    pi = m.policy()
    assert abs(float(pi.astype(np.float64).sum()) - 1.0) < 1e-6
    want = np.zeros_like(pi)
    for a, _, _, P in ch:
        want[a] = P
    assert np.abs(pi - want).max() < 1e-7
    n = GumbelModel(board, m=4, seed=2, game_id=9)
    n.search(16)
    assert abs(float(n.policy().astype(np.float64).sum()) - 1.0) < 1e-6 and n.move() in [c[0] for c in n.root_children()]
    assert m.advance() == ch[top[0]][0] and m.considered() == [] and m.ply == 1


# ---- argument checks: ValueError before any device work (no library is loaded)
def _nets():
    from alphazero_amd.games.othello import OthelloNet

    class Other(OthelloNet):
        def evaluate(self, board):
            return super().evaluate(board)

    class Torchy(OthelloNet):
        def forward(self, x):
            return super().forward(x)
    return OthelloNet(n=6, device="cpu"), Other(n=6, device="cpu"), Torchy(n=6, device="cpu")


def test_parse():
    assert G.parse(None) is None
    assert G.parse(16) == G.parse({}) == (16, 50.0, 0.5, 1.0)
    assert G.parse({"m": np.int64(4), "gumbel_scale": 0}) == (4, 50.0, 0.5, 0.0)
    for bad in (0, 17, True, 2.5, -1, "4", {"m": 4.0}, {"k": 1}, {"c_visit": -1}, {"c_scale": math.inf}, {"gumbel_scale": math.nan},
                {"c_visit": "1"}):
        with pytest.raises(ValueError, match="gumbel"):
            G.parse(bad)


@pytest.mark.parametrize("bad", [0, 17, True, 2.5, "4"])
def test_gumbel_values_are_checked_by_every_surface(bad):
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    from alphazero_amd.trainer import AlphaZeroTrainer
    hip, _, _ = _nets()
    with pytest.raises(ValueError, match="gumbel"):
        MCT(eval_method="neural", nn=hip, gumbel=bad)
    with pytest.raises(ValueError, match="gumbel"):
        AlphaZeroPlayer(n_sim=4, nn=hip, gumbel=bad)
    with pytest.raises(ValueError, match="gumbel"):
        BatchedAlphaZeroPlayer(n_sim=4, nn=hip, n_slots=2, gumbel=bad)
    with pytest.raises(ValueError, match="gumbel"):
        AlphaZeroTrainer(selfplay_gumbel=bad)


def test_gumbel_refusals_come_before_any_device_work():
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    hip, board_net, torch_net = _nets()
    for nn in (board_net, torch_net):
        with pytest.raises(ValueError, match="external evaluator"):
            MCT(eval_method="neural", nn=nn, gumbel=4)
        with pytest.raises(ValueError, match="external evaluator"):
            AlphaZeroPlayer(n_sim=4, nn=nn, gumbel=4)
        with pytest.raises(ValueError, match="external evaluator"):
            BatchedAlphaZeroPlayer(n_sim=4, nn=nn, n_slots=2, gumbel=4)
        m = MCT(eval_method="neural", nn=hip, gumbel=4)
        with pytest.raises(ValueError, match="external evaluator"):
            m.nn = nn
    with pytest.raises(ValueError, match="rollout|neural"):
        MCT(eval_method="rollout", gumbel=4)
    for make in (lambda: MCT(eval_method="neural", nn=hip, leaf_batch=4, gumbel=4),
                 lambda: AlphaZeroPlayer(n_sim=4, nn=hip, leaf_batch=2, gumbel={"m": 4}),
                 lambda: BatchedAlphaZeroPlayer(n_sim=4, nn=hip, n_slots=2, leaf_batch=16, gumbel=4)):
        with pytest.raises(ValueError, match="leaf_batch"):
            make()
    with pytest.raises(ValueError, match="compute_time"):
        AlphaZeroPlayer(compute_time=0.01, nn=hip, gumbel=4)
    with pytest.raises(ValueError, match="compute_time"):
        MCT(eval_method="neural", nn=hip, gumbel=4).search(make_board("othello", 6, 6), compute_time=0.01)
    # allowed: with leaf_batch 1 and the symmetry modes, and the setting travels through clone() and reset()
    MCT(eval_method="neural", nn=hip, leaf_batch=1, symmetry="random", gumbel=16)
    p = AlphaZeroPlayer(n_sim=4, nn=hip, gumbel={"m": 8, "gumbel_scale": 0})
    assert p.gumbel == {"m": 8, "gumbel_scale": 0} and p.clone().gumbel == p.gumbel
    p.reset()
    assert p.gumbel == {"m": 8, "gumbel_scale": 0} and p.mct.gumbel == p.gumbel
    assert AlphaZeroPlayer(n_sim=4, nn=hip).gumbel is None


def test_exports_are_declared_and_listed():
    from alphazero_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_engine_set_gumbel\(az_engine \*e, int32_t m, double c_visit, double c_scale, double gumbel_scale\);", hdr)
    assert re.search(r"int az_engine_gumbel_considered\(az_engine \*e, int32_t slot, uint64_t \*mask\);", hdr)
    assert re.search(r"#define AZ_MAX_GUMBEL 16\b", hdr)
    assert "az_engine_set_gumbel" in _lib.SYMBOLS and "az_engine_gumbel_considered" in _lib.SYMBOLS
    assert G.MAX_GUMBEL == 16
