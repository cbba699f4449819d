"""CPU: resignation in self-play (az_engine_set_resign) -- what needs no GPU.

  1. az_resign_value, the library's host restatement of the kernels' arithmetic, equals the host model's value bit for bit on a few
     thousand random child arrays: zero-visit children, ties in N, one child, no visit at all (NaN);
  2. az_resign_holdout equals the model's coin (Philox and u53 restated in Python) on 20 000 (seed, game id) pairs, game ids >= 2^31
     among them, at p 0 / 0.1 / 0.5 / 1.0; the share of holdouts is p within 4 sigma;
  3. resign.calibrate on hand-made logs: no side at all, ties, the clip at both ends, and never more than c sides below the result;
  4. the option's form is checked where it is given: resign.parse, the trainer's constructor, the engine's setter;
  5. the ABI: the six symbols are declared with their signatures, listed and exported; az_version() >= 118;
  6. the host model itself: record-only (holdout 1.0) is the plain game, a resigned game is a prefix of it.
(The engine's own refusals and everything a wave does need a GPU: tests/test_gpu_resign.py.)
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from alphazero_amd import _lib
from alphazero_amd import resign as R
import playout_cap_model as PM
import resign_model as M

N_PAIRS = 20000


def _bits(x):
    return np.array([x], np.float64).view(np.int64)[0]


# ------------------------------------------------------------------------------------------------------------------ 1
def _child_arrays():
    rng = np.random.default_rng(1118)
    out = [(np.array([5], np.int32), np.array([-0.25])), (np.array([0], np.int32), np.array([0.5])),
           (np.array([3, 3, 3], np.int32), np.array([-0.9, 0.1, 0.4])), (np.array([0, 0, 7, 7], np.int32), np.array([0.3, 0.9, -0.2, -0.1])),
           (np.array([1, 2], np.int32), np.array([-0.0, 0.0])), (np.array([2, 1], np.int32), np.array([0.0, -0.0])),
           (np.zeros(6, np.int32), rng.uniform(-1, 1, 6))]
    for i in range(4000):
        nc = 1 if i % 50 == 0 else int(rng.integers(1, 65))
        N = rng.integers(0, [2, 4, 40, 2000][i % 4], nc).astype(np.int32)  # small ranges: many zeros and many ties
        Q = rng.uniform(-1.0, 1.0, nc)
        if i % 7 == 0:
            Q = np.round(Q, 1)
        out.append((N, Q))
    return out


def test_the_librarys_value_is_the_models_value():
    from alphazero_amd.engine import SelfPlayEngine
    L = _lib.lib()
    untested = ties = zeros = single = 0
    for N, Q in _child_arrays():
        want = M.value(N, Q)
        v = C.c_double(123.0)
        assert L.az_resign_value(len(N), N.ctypes.data, Q.ctypes.data, C.byref(v)) == _lib.AZ_OK
        if want is None:
            assert math.isnan(v.value) and math.isnan(SelfPlayEngine.resign_value(N, Q))
            untested += 1
            continue
        assert _bits(v.value) == _bits(want), (N, Q, v.value, want)
        assert _bits(SelfPlayEngine.resign_value(N, Q)) == _bits(want)
        ties += int((N == N.max()).sum() > 1)
        zeros += int((N == 0).any())
        single += int(len(N) == 1)
    assert untested > 10 and ties > 500 and zeros > 500 and single > 20


def test_the_value_by_hand():
    assert M.value([5], [-0.25]) == -0.25
    assert M.value([3, 3, 3], [-0.9, 0.1, 0.4]) == max((3 * -0.9 + 3 * 0.1 + 3 * 0.4) / 9.0, -0.9)  # the tie goes to child 0
    assert M.value([0, 0, 7, 7], [0.3, 0.9, -0.2, -0.1]) == (7.0 * -0.2 + 7.0 * -0.1) / 14.0  # unvisited children do not count
    assert M.value([1, 9], [1.0, -0.5]) == (1.0 + 9.0 * -0.5) / 10.0  # the mean above the most visited child's value
    assert M.value([0, 0], [0.1, 0.2]) is None
    v = C.c_double()
    L = _lib.lib()
    assert L.az_resign_value(0, None, None, C.byref(v)) == _lib.AZ_OK and math.isnan(v.value)
    N, Q = np.array([1, -1], np.int32), np.array([0.0, 0.0])
    assert L.az_resign_value(2, N.ctypes.data, Q.ctypes.data, C.byref(v)) == _lib.AZ_EINVAL
    assert L.az_resign_value(2, None, Q.ctypes.data, C.byref(v)) == _lib.AZ_EINVAL
    assert L.az_resign_value(2, N.ctypes.data, Q.ctypes.data, None) == _lib.AZ_EINVAL
    assert L.az_resign_value(-1, N.ctypes.data, Q.ctypes.data, C.byref(v)) == _lib.AZ_EINVAL


# ------------------------------------------------------------------------------------------------------------------ 2
def _pairs():
    rng = np.random.default_rng(20371)
    seeds = rng.integers(0, 1 << 32, N_PAIRS, dtype=np.uint64)
    gids = rng.integers(0, 1 << 32, N_PAIRS, dtype=np.uint64)
    gids[::5] |= np.uint64(1 << 31)  # every fifth id in the upper half for certain
    gids[:4] = [0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
    seeds[:4] = [0, 1, (1 << 32) - 1, 1 << 31]
    return [(int(s), int(g)) for s, g in zip(seeds, gids)]


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 1.0])
def test_the_librarys_holdout_coin_is_the_models(p):
    L = _lib.lib()
    pairs = _pairs()
    assert sum(1 for _, g in pairs if g >= 1 << 31) > N_PAIRS // 5
    held = 0
    for s, g in pairs:
        got = L.az_resign_holdout(s, g, p)
        assert got in (0, 1) and bool(got) == M.holdout(s, g, p), (s, g, p)
        held += got
    sigma = math.sqrt(N_PAIRS * p * (1.0 - p))
    assert abs(held - N_PAIRS * p) <= 4.0 * sigma, (held, N_PAIRS * p, sigma)
    if p in (0.0, 1.0):
        assert held == int(N_PAIRS * p)


def test_the_coin_is_a_draw_of_its_own_and_the_wrapper_reads_it():
    from alphazero_amd.engine import SelfPlayEngine
    from tools import closed_form as cf
    assert M.P_RESIGN == 11 and M.P_RESIGN not in (cf.P_TIE_SELECT, cf.P_NOISE_NORMAL, cf.P_NOISE_BOOST, cf.P_MOVE_SAMPLE, cf.P_TIE_MOVE,
                                                   cf.P_ROLLOUT_EXPAND, cf.P_PLAYOUT, cf.P_SYMMETRY, 9, PM.P_PLAYOUT_CAP)
    r = cf.philox4x32(7, 3, 0, 0xFFFF, 11, 0)
    assert M.holdout(7, 3, 0.5) == (cf.u53(r[0], r[1]) < 0.5)
    for s, g in _pairs()[:200]:
        assert SelfPlayEngine.resign_holdout(s, g, 0.3) is M.holdout(s, g, 0.3)


# ------------------------------------------------------------------------------------------------------------------ 3
def _below(low, winner, t, holdout=None):
    """the non-losing sides of the (holdout) games whose low is below t: the false positives a threshold t would have made"""
    n = 0
    for i, (lo, w) in enumerate(zip(low, winner)):
        if holdout is not None and not holdout[i]:
            continue
        n += int(w >= 0 and lo[0] < t) + int(w <= 0 and lo[1] < t)
    return n


def test_calibrate_on_hand_made_logs():
    assert R.calibrate(np.zeros((0, 2)), np.zeros(0, np.int8), 0.05, -0.3) == -0.3  # n = 0: the current threshold
    low = [[-0.9, 0.5], [-0.2, -0.8]]
    assert R.calibrate(low, [-1, 1], 0.0, -0.4) == -0.2  # one side per game counts, the winner's: [-0.2, 0.5] -> c = 0
    assert R.calibrate(low, [-1, 1], 0.5, -0.4) == R.BELOW_ZERO  # c = 1: 0.5, clipped below 0
    assert R.calibrate(low, [-1, -1], 0.0, -0.4) == -0.8  # sides [0.5, -0.8]: c = 0, the lowest
    assert R.calibrate(low, [1, -1], 0.0, -0.4) == -0.9
    assert R.calibrate(low, [1, 1], 0.0, -0.4, holdout=[0, 0]) == -0.4  # no holdout game: the current threshold
    assert R.calibrate(low, [1, 1], 0.0, -0.4, holdout=[0, 1]) == -0.2
    # a draw counts both sides
    assert R.calibrate([[-0.5, -0.7]], [0], 0.0, -0.1) == -0.7 and R.calibrate([[-0.5, -0.7]], [0], 0.5, -0.1) == -0.5
    # the clip: a window that was never full (2.0) or a positive low gives the greatest threshold below 0; nothing below -1
    t = R.calibrate([[2.0, 2.0], [0.4, 2.0]], [1, 1], 0.0, -0.4)
    assert t == R.BELOW_ZERO and -1e-300 < t < 0.0
    assert R.calibrate([[-1.0, 2.0]], [1], 0.0, -0.4) == -1.0
    # ties: every side at one value -- none of them is below the result
    low = [[-0.5, 2.0]] * 10
    t = R.calibrate(low, [1] * 10, 0.3, -0.1)
    assert t == -0.5 and _below(low, [1] * 10, t) == 0
    for bad in (-0.1, 1.0, float("nan"), None, "0.05"):
        with pytest.raises(ValueError, match="target_fp"):
            R.calibrate(low, [1] * 10, bad, -0.1)
    with pytest.raises(ValueError, match="rows of low"):
        R.calibrate(low, [1] * 9, 0.1, -0.1)


def test_calibrate_never_leaves_more_than_c_sides_below():
    rng = np.random.default_rng(37)
    for trial in range(300):
        n = int(rng.integers(1, 60))
        low = np.round(rng.uniform(-1.0, 0.6, (n, 2)), 1 if trial % 2 else 3)  # one decimal: many ties
        low[rng.random((n, 2)) < 0.1] = 2.0
        winner = rng.integers(-1, 2, n)
        holdout = rng.random(n) < 0.6
        target = float(rng.choice([0.0, 0.05, 0.1, 0.25, 0.5, 0.9]))
        sides = int(((winner >= 0) & holdout).sum() + ((winner <= 0) & holdout).sum())
        t = R.calibrate(low, winner, target, -0.25, holdout=holdout)
        assert -1.0 <= t < 0.0
        if sides == 0:
            assert t == -0.25
        else:
            assert _below(low, winner, t, holdout) <= math.floor(target * sides), (trial, t)


# ------------------------------------------------------------------------------------------------------------------ 4
GOOD = {"threshold": -0.9, "consecutive": 2, "min_ply": 4, "holdout": 0.1}
BAD_FORMS = [-0.9, (-0.9, 2, 4, 0.1), "resign", {}, {"consecutive": 2}, dict(GOOD, threshold=0.0), dict(GOOD, threshold=-1.5),
             dict(GOOD, threshold=float("nan")), dict(GOOD, threshold="-0.9"), dict(GOOD, threshold=True), dict(GOOD, consecutive=0),
             dict(GOOD, consecutive=5), dict(GOOD, consecutive=2.0), dict(GOOD, consecutive=True), dict(GOOD, min_ply=-1),
             dict(GOOD, min_ply=1.5), dict(GOOD, min_ply=1 << 31), dict(GOOD, holdout=-0.1), dict(GOOD, holdout=1.1),
             dict(GOOD, holdout=float("nan")), dict(GOOD, holdout=None), dict(GOOD, window=3)]


@pytest.mark.parametrize("bad", BAD_FORMS)
def test_the_form_is_checked_where_the_option_is_given(bad):
    from alphazero_amd.engine import SelfPlayEngine
    from alphazero_amd.trainer import AlphaZeroTrainer
    with pytest.raises(ValueError, match=r"expected None or a dict of threshold in \[-1, 0\)"):
        R.parse(bad)
    with pytest.raises(ValueError, match=r"selfplay_resign=.*expected None or a dict of threshold"):
        AlphaZeroTrainer(selfplay_resign=bad)
    eng = SelfPlayEngine.__new__(SelfPlayEngine)  # no engine behind it: the form is refused before the library is asked
    eng.h = None
    with pytest.raises(ValueError, match=r"resign=.*expected None or a dict of threshold"):
        eng.set_resign(bad)


def test_valid_forms_and_calibrate_belongs_to_the_trainer():
    from alphazero_amd.engine import SelfPlayEngine
    from alphazero_amd.trainer import AlphaZeroTrainer
    assert R.parse(None) is None and R.parse(GOOD) == GOOD
    assert R.parse({"threshold": -1}) == {"threshold": -1.0, "consecutive": 1, "min_ply": 0, "holdout": 0.1}
    got = R.parse({"threshold": np.float32(-0.5), "consecutive": np.int64(4), "min_ply": np.int32(0), "holdout": 1})
    assert got == {"threshold": -0.5, "consecutive": 4, "min_ply": 0, "holdout": 1.0} and isinstance(got["holdout"], float)
    assert R.parse(dict(GOOD, calibrate=0.05), calibrate=True) == dict(GOOD, calibrate=0.05)
    assert R.parse(GOOD, calibrate=True) == dict(GOOD, calibrate=None)
    with pytest.raises(ValueError, match="expected None or a dict of threshold"):
        R.parse(dict(GOOD, calibrate=0.05))  # the engine's setter takes a fixed threshold
    eng = SelfPlayEngine.__new__(SelfPlayEngine)
    eng.h = None
    with pytest.raises(ValueError, match="expected None or a dict of threshold"):
        eng.set_resign(dict(GOOD, calibrate=0.05))
    for bad in (1.0, -0.1, "0.05", True, float("nan")):
        with pytest.raises(ValueError, match=r"selfplay_resign=.*calibrate None or a target false-positive rate in \[0, 1\)"):
            AlphaZeroTrainer(selfplay_resign=dict(GOOD, calibrate=bad))
    t = AlphaZeroTrainer()
    assert t.selfplay_resign is None and t.resign_threshold is None and t.resign_stats == {}
    t = AlphaZeroTrainer(selfplay_resign=dict(GOOD, calibrate=0.05))
    assert t.resign_threshold == -0.9 and t._check_selfplay_resign() == dict(GOOD, calibrate=0.05)
    # every self-play mode combines: the rule reads the root's children and nothing else
    AlphaZeroTrainer(selfplay_resign=GOOD, selfplay_gumbel=16)
    AlphaZeroTrainer(selfplay_resign=GOOD, selfplay_playout_cap=(4, 0.4), selfplay_forced_playouts=2.0)
    AlphaZeroTrainer(selfplay_resign=GOOD, selfplay_symmetry="random")


def test_calibrate_is_refused_with_more_than_one_rank(monkeypatch):
    from alphazero_amd.trainer import AlphaZeroTrainer
    monkeypatch.setattr(AlphaZeroTrainer, "_dist", staticmethod(lambda: (0, 2)))
    AlphaZeroTrainer(selfplay_resign=GOOD)  # a fixed threshold is served
    with pytest.raises(ValueError, match=r"calibrate is not served with more than one rank"):
        AlphaZeroTrainer(selfplay_resign=dict(GOOD, calibrate=0.05))


# ------------------------------------------------------------------------------------------------------------------ 5
def test_the_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_engine_set_resign\(az_engine \*e, double v_resign, int32_t consecutive, int32_t min_ply, double p_holdout\);", hdr)
    assert re.search(r"int az_engine_resign_stats\(az_engine \*e, int64_t \*resigned, int64_t \*holdout_games, int64_t \*holdout_triggered,\s+"
                     r"int64_t \*holdout_false_positives\);", hdr)
    assert re.search(r"int az_engine_game_log\(az_engine \*e, int64_t \*n, const int32_t \*\*d_rows, const double \*\*d_low\);", hdr)
    assert re.search(r"int az_engine_resign_values\(az_engine \*e, double \*d_v\);", hdr)
    assert re.search(r"int az_resign_value\(int32_t n_children, const int32_t \*N, const double \*Q, double \*v\);", hdr)
    assert re.search(r"int az_resign_holdout\(uint32_t seed, uint32_t game_id, double p_holdout\);", hdr)
    names = ("az_engine_set_resign", "az_engine_resign_stats", "az_engine_game_log", "az_engine_resign_values", "az_resign_value",
             "az_resign_holdout")
    assert set(names) <= set(_lib.SYMBOLS)
    L = _lib.lib()
    for s in names:
        assert hasattr(L, s), s
    assert L.az_version() >= 118
    assert L.az_engine_set_resign(None, -0.9, 2, 4, 0.1) == _lib.AZ_EINVAL
    assert L.az_engine_resign_stats(None, None, None, None, None) == _lib.AZ_EINVAL
    assert L.az_engine_game_log(None, None, None, None) == _lib.AZ_EINVAL
    assert L.az_engine_resign_values(None, None) == _lib.AZ_EINVAL
    with pytest.raises(ValueError, match="null engine"):
        _lib.check(L.az_engine_set_resign(None, float("nan"), 0, 0, 0.0))


# ------------------------------------------------------------------------------------------------------------------ 6
def test_the_model_record_only_is_the_plain_game_and_a_resigned_game_is_a_prefix():
    args = dict(game="tictactoe", H=3, W=3, seed=11, first_game_id=1000, n_games=12, n_sim=12, noise=(0.03, 0.25), tie="random", tmax=2, tmin=7)
    off, c_off = PM.play_wave(cap=None, **args)
    rec, c_rec, rows, low = M.play_wave(resign=(-0.05, 1, 4, 1.0), cap=None, **args)
    for k in off:
        assert np.array_equal(off[k], rec[k]), k
    assert c_rec["resigned"] == 0 and c_rec["holdout_games"] == 12 and c_rec["samples"] == c_off["samples"] and c_rec["rows"] == c_off["rows"]
    assert list(rows[:, 0]) == list(range(1000, 1012)) and np.all(rows[:, 3] == 0) and np.all(rows[:, 4] == 1) and np.all(rows[:, 7] == 0)
    for row, lo in zip(rows, low):  # a trigger exists iff the side's low is below the threshold
        assert (row[5] >= 0) == bool((lo < -0.05).any())
        if row[5] >= 0:
            assert lo[0 if row[6] == 1 else 1] < -0.05 and row[5] >= 4
    on, c_on, rows_on, _ = M.play_wave(resign=(-0.05, 1, 4, 0.0), cap=None, **args)
    assert c_on["resigned"] > 0 and c_on["holdout_games"] == 0 and c_on["samples"] == c_on["plies"] < c_off["plies"]
    for row, full in zip(rows_on, rows):
        mine, theirs = on["meta"][:, 0] == row[0], off["meta"][:, 0] == row[0]
        n = int(mine.sum())
        assert n == row[1] <= full[1]
        for k in ("state", "pi", "visits", "meta"):
            assert np.array_equal(on[k][mine], off[k][theirs][:n]), (row[0], k)
        if row[3]:  # resigned where the record-only game first triggered: the mover lost
            assert (row[5], row[6]) == (full[5], full[6]) and row[1] == row[5] + 1 and row[2] == -row[6]
            assert np.array_equal(on["z"][mine], (-row[6] * on["meta"][mine][:, 2]).astype(np.int8))
        else:
            assert full[5] < 0 and np.array_equal(on["z"][mine], off["z"][theirs])
