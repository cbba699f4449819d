"""CPU: playout cap randomization (az_engine_set_playout_cap) -- what needs no GPU.

  1. az_playout_cap_full, the library's host restatement of the kernels' coin, equals the host model's coin (Philox and u53 restated
     in Python) on 20 000 (seed, game id, ply) triples, game ids >= 2^31 among them; the share of full plies is p_full within 4 sigma;
     p_full = 1.0 makes every ply full;
  2. the option's form is checked where it is given: the trainer's constructor, the engine's setter before it touches the library;
     the combinations the trainer refuses name the other mode;
  3. the ABI: the three symbols are declared with their signatures, listed and exported; null arguments are AZ_EINVAL.
(The engine's own refusals -- leaf_batch, the Gumbel search, the symmetry modes, rollout and external engines, and those modes'
setters while the cap is on -- need an engine and so a GPU: tests/test_gpu_playout_cap.py.)
"""
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from alphazero_amd import _lib
from alphazero_amd import playout_cap as PC
import playout_cap_model as M

N_TRIPLES = 20000


def _triples():
    rng = np.random.default_rng(20191)
    seeds = rng.integers(0, 1 << 32, N_TRIPLES, dtype=np.uint64)
    gids = rng.integers(0, 1 << 32, N_TRIPLES, dtype=np.uint64)
    gids[::5] |= np.uint64(1 << 31)          # every fifth id in the upper half for certain
    gids[:4] = [0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
    seeds[:4] = [0, 1, (1 << 32) - 1, 1 << 31]
    plies = rng.integers(0, 129, N_TRIPLES)
    return [(int(s), int(g), int(p)) for s, g, p in zip(seeds, gids, plies)]


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("p_full", [0.1, 0.25, 0.5, 1.0])
def test_the_librarys_coin_is_the_models_coin(p_full):
    L = _lib.lib()
    tr = _triples()
    assert sum(1 for _, g, _ in tr if g >= 1 << 31) > N_TRIPLES // 5
    full = 0
    for s, g, p in tr:
        want = M.coin_full(s, g, p, p_full)
        got = L.az_playout_cap_full(s, g, p, p_full)
        assert got in (0, 1) and bool(got) == want, (s, g, p, p_full)
        full += got
    sigma = math.sqrt(N_TRIPLES * p_full * (1.0 - p_full))
    assert abs(full - N_TRIPLES * p_full) <= 4.0 * sigma, (full, N_TRIPLES * p_full, sigma)
    if p_full == 1.0:
        assert full == N_TRIPLES


def test_the_python_wrapper_reads_the_same_coin():
    from alphazero_amd.engine import SelfPlayEngine
    for s, g, p in _triples()[:200]:
        assert SelfPlayEngine.playout_cap_full(s, g, p, 0.4) is M.coin_full(s, g, p, 0.4)


def test_the_coin_is_a_draw_of_its_own():
    """purpose id 10 at counter (ply, 0xFFFF, 10, 0): not the move-sample or tie-move draw of the same (game, ply)"""
    from tools import closed_form as cf
    assert M.P_PLAYOUT_CAP == 10 and M.P_PLAYOUT_CAP not in (cf.P_TIE_SELECT, cf.P_NOISE_NORMAL, cf.P_NOISE_BOOST, cf.P_MOVE_SAMPLE,
                                                             cf.P_TIE_MOVE, cf.P_ROLLOUT_EXPAND, cf.P_PLAYOUT, cf.P_SYMMETRY, 9)
    r = cf.philox4x32(7, 3, 5, 0xFFFF, 10, 0)
    assert M.coin_full(7, 3, 5, 0.5) == (cf.u53(r[0], r[1]) < 0.5)
    assert r != cf.philox4x32(7, 3, 5, 0xFFFF, cf.P_MOVE_SAMPLE, 0)


# ------------------------------------------------------------------------------------------------------------------ 2
BAD_FORMS = [4, (4,), (4, 0.4, 1), "4,0.4", (0, 0.4), (-1, 0.4), (4.0, 0.4), (True, 0.4), (4, 0.0), (4, -0.1), (4, 1.5), (4, float("nan")),
             (4, "0.4"), (4, None), (1 << 31, 0.5)]


@pytest.mark.parametrize("bad", BAD_FORMS)
def test_the_form_is_checked_where_the_option_is_given(bad):
    from alphazero_amd.engine import SelfPlayEngine
    from alphazero_amd.trainer import AlphaZeroTrainer
    with pytest.raises(ValueError, match=r"expected None or \(n_fast, p_full\)"):
        PC.parse(bad)
    with pytest.raises(ValueError, match=r"selfplay_playout_cap=.*expected None or \(n_fast, p_full\)"):
        AlphaZeroTrainer(selfplay_playout_cap=bad)
    eng = SelfPlayEngine.__new__(SelfPlayEngine)  # no engine behind it: the form is refused before the library is asked
    eng.h = None
    with pytest.raises(ValueError, match=r"playout_cap=.*expected None or \(n_fast, p_full\)"):
        eng.set_playout_cap(bad)


def test_valid_forms_and_the_trainers_refusals_name_the_other_mode():
    from alphazero_amd.trainer import AlphaZeroTrainer
    assert PC.parse(None) is None and PC.parse((4, 0.4)) == (4, 0.4) and PC.parse([np.int64(25), np.float32(0.25)]) == (25, 0.25)
    assert PC.parse((1, 1)) == (1, 1.0) and isinstance(PC.parse((1, 1))[1], float)
    assert AlphaZeroTrainer().selfplay_playout_cap is None
    assert AlphaZeroTrainer(selfplay_playout_cap=(25, 0.25)).selfplay_playout_cap == (25, 0.25)
    with pytest.raises(ValueError, match=r"selfplay_playout_cap=\(4, 0\.4\) does not combine with selfplay_gumbel=16"):
        AlphaZeroTrainer(selfplay_playout_cap=(4, 0.4), selfplay_gumbel=16)
    with pytest.raises(ValueError, match=r"selfplay_playout_cap=\(4, 0\.4\) does not combine with selfplay_symmetry='random'"):
        AlphaZeroTrainer(selfplay_playout_cap=(4, 0.4), selfplay_symmetry="random")
    t = AlphaZeroTrainer(selfplay_playout_cap=(4, 0.4))
    t.selfplay_gumbel = 8  # set after construction: checked again before the engine is built
    with pytest.raises(ValueError, match="does not combine with selfplay_gumbel=8"):
        t._check_selfplay_playout_cap()


# ------------------------------------------------------------------------------------------------------------------ 3
def test_the_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_engine_set_playout_cap\(az_engine \*e, int32_t n_fast, double p_full\);", hdr)
    assert re.search(r"int az_engine_playout_cap_stats\(az_engine \*e, int64_t \*full_plies, int64_t \*fast_plies\);", hdr)
    assert re.search(r"int az_playout_cap_full\(uint32_t seed, uint32_t game_id, int32_t ply, double p_full\);", hdr)
    assert {"az_engine_set_playout_cap", "az_engine_playout_cap_stats", "az_playout_cap_full"} <= set(_lib.SYMBOLS)
    L = _lib.lib()
    for s in ("az_engine_set_playout_cap", "az_engine_playout_cap_stats", "az_playout_cap_full"):
        assert hasattr(L, s), s
    assert L.az_version() >= 109
    assert L.az_engine_set_playout_cap(None, 4, 0.4) == _lib.AZ_EINVAL
    assert L.az_engine_playout_cap_stats(None, None, None) == _lib.AZ_EINVAL
    with pytest.raises(ValueError, match="null engine"):
        _lib.check(L.az_engine_set_playout_cap(None, 0, 1.0))


# ------------------------------------------------------------------------------------------------------------------ the model itself
def test_the_model_records_full_plies_only_and_off_is_the_plain_game():
    """the host model on TicTacToe: with the cap the samples are the full plies by the coin, a fast ply walks n_fast simulations and a
    full one n_sim on top of what it inherits; cap None and p_full = 1.0 are the same game"""
    args = dict(game="tictactoe", H=3, W=3, seed=5, first_game_id=0, n_games=6, n_sim=12, noise=(0.03, 0.25), tie="random", tmax=1, tmin=5)
    off, c_off = M.play_wave(cap=None, **args)
    one, c_one = M.play_wave(cap=(4, 1.0), **args)
    for k in off:
        assert np.array_equal(off[k], one[k]), k
    assert c_off == c_one and c_off["fast_plies"] == 0 and c_off["samples"] == c_off["plies"]
    cap, c = M.play_wave(cap=(4, 0.4), **args)
    assert 0 < c["fast_plies"] and 0 < c["full_plies"] == c["samples"] == len(cap["z"]) and c["rows"] < c_off["rows"]
    for gid, ply in cap["meta"][:, :2]:
        assert M.coin_full(5, int(gid), int(ply), 0.4)
    inherited = cap["root_N"] - cap["visits"].sum(axis=1)  # the root's own first visit (a fresh root) or nothing
    assert np.all(cap["visits"].sum(axis=1) >= 12) and np.all((inherited == 0) | (inherited == 1))
