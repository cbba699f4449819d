"""CPU: forced playouts and policy target pruning (az_engine_set_forced_playouts) -- what needs no GPU.

  1. az_forced_playout and az_forced_prune, the library's host restatement of the kernels' arithmetic, equal the host model
     (tests/forced_playouts_model.py) on 20 000 random roots: 1 .. 64 children, root_n 0 .. 800, Q in [-1, 1], priors that sum to 1,
     k in {0.5, 2, 8}; the invariants of the pruned counts hold on every root; k = 1e-12 forces nothing and prunes nothing;
  2. the option's form is checked where it is given: the parser, the trainer's constructor, the engine's setter before it touches the
     library; the combinations the trainer refuses name the other mode, and the playout cap combines;
  3. the ABI: the four symbols are declared with their signatures, listed and exported; null arguments are AZ_EINVAL;
  4. the preconditions of tests/test_gpu_forced_playouts.py, on the model: every (game, tie mode) wave it plays, with the playout cap
     and without, has forced picks, pruned playouts and at least one recorded pi that differs from the raw-count policy.
(The engine's own refusals need an engine and so a GPU: tests/test_gpu_forced_playouts.py.)
"""
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from alphazero_amd import _lib
from alphazero_amd import forced_playouts as FP
import forced_playouts_model as F

N_ROOTS = 20000
KS = (0.5, 2.0, 8.0)
_CACHE = {}


def _roots():
    """[(N, Q, P, root_n)]: visit counts that sum to about root_n - 1 (a searched root), some roots with stray counts above it"""
    if "roots" not in _CACHE:
        rng = np.random.default_rng(20192)
        out = []
        for i in range(N_ROOTS):
            nc = int(rng.integers(1, 65))
            root_n = int(rng.integers(0, 801))
            P = rng.dirichlet(np.full(nc, 0.3 if i & 1 else 1.0))
            P = P / P.sum()
            Q = rng.uniform(-1.0, 1.0, nc)
            if i % 7 == 0:
                Q = np.round(Q * 4.0) / 4.0  # equal values: gap == 0.0 happens
            if root_n <= 1:
                N = np.zeros(nc, np.int64)
            elif i % 5 == 0:
                N = rng.integers(0, root_n + 1, nc)  # counts no search would leave: the arithmetic is total all the same
            else:
                N = rng.multinomial(root_n - 1, rng.dirichlet(np.full(nc, 0.5)))
            out.append((N.astype(np.int32), Q.astype(np.float64), P.astype(np.float64), root_n))
        _CACHE["roots"] = out
    return _CACHE["roots"]


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("k", KS)
def test_the_librarys_arithmetic_is_the_models(k):
    from alphazero_amd.engine import SelfPlayEngine
    L = _lib.lib()
    forced_seen = pruned_seen = zeroed_seen = 0
    for N, Q, P, root_n in _roots():
        want_f = [F.forced(int(n), float(p), root_n, k) for n, p in zip(N, P)]
        got_f = [L.az_forced_playout(int(n), float(p), root_n, k) for n, p in zip(N, P)]
        assert all(g in (0, 1) for g in got_f) and [bool(g) for g in got_f] == want_f, (N, P, root_n, k)
        want = F.prune([int(n) for n in N], [float(q) for q in Q], [float(p) for p in P], root_n, k)
        got = SelfPlayEngine.forced_prune(N, Q, P, root_n, k)
        assert got.dtype == np.int32 and list(got) == want, (N, Q, P, root_n, k, list(got), want)
        # the invariants of the pruned counts
        star = int(np.argmax(N))  # the first of the greatest
        assert got[star] == N[star]
        assert np.all(got >= 0) and np.all(got <= N)
        assert np.all(got[N == 0] == 0)
        for n, m, p in zip(N, got, P):
            nf = int(math.sqrt((k * float(p)) * float(root_n)))
            # at most the forced playouts go -- unless the child was zeroed from N' = 1, which then was >= N - nf
            assert n - m <= nf or (m == 0 and n - 1 <= nf), (n, m, nf)
        forced_seen += sum(want_f)
        pruned_seen += int((N - got).sum() > 0)
        zeroed_seen += int(np.any((got == 0) & (N > 0)))
    assert forced_seen > 1000 and pruned_seen > 1000 and zeroed_seen > 100, (forced_seen, pruned_seen, zeroed_seen)


def test_the_python_wrappers():
    from alphazero_amd.engine import SelfPlayEngine
    assert SelfPlayEngine.forced_playout(1, 0.5, 10, 2.0) is True      # 1 < 2 * 0.5 * 10
    assert SelfPlayEngine.forced_playout(4, 0.5, 10, 2.0) is False     # 16 >= 10
    assert SelfPlayEngine.forced_playout(0, 0.5, 10, 2.0) is False     # never visited
    assert SelfPlayEngine.forced_playout(3, 0.5, 0, 2.0) is False      # a fresh root
    assert SelfPlayEngine.forced_playout(1, 0.5, 10, 0.0) is False     # off
    assert list(SelfPlayEngine.forced_prune([], [], [], 5, 2.0)) == []
    assert list(SelfPlayEngine.forced_prune([7], [0.1], [1.0], 8, 2.0)) == [7]
    assert list(SelfPlayEngine.forced_prune([5, 3, 0], [0.5, -0.5, 0.0], [0.5, 0.3, 0.2], 9, 0.0)) == [5, 3, 0]  # k = 0 copies
    with pytest.raises(ValueError, match="one length"):
        SelfPlayEngine.forced_prune([1, 2], [0.0], [0.5, 0.5], 4, 2.0)
    with pytest.raises(ValueError, match=r"az_forced_prune: k must be finite and in \[0, 64\]"):
        SelfPlayEngine.forced_prune([1, 2], [0.0, 0.0], [0.5, 0.5], 4, 65.0)
    with pytest.raises(ValueError, match=r"az_forced_prune: k must be finite"):
        SelfPlayEngine.forced_prune([1, 2], [0.0, 0.0], [0.5, 0.5], 4, float("nan"))


def test_a_tiny_k_forces_nothing_and_prunes_nothing():
    from alphazero_amd.engine import SelfPlayEngine
    L = _lib.lib()
    for N, Q, P, root_n in _roots()[:4000]:
        assert not any(L.az_forced_playout(int(n), float(p), root_n, 1e-12) for n, p in zip(N, P))
        assert not any(F.forced(int(n), float(p), root_n, 1e-12) for n, p in zip(N, P))
        got = SelfPlayEngine.forced_prune(N, Q, P, root_n, 1e-12)
        want = F.prune([int(n) for n in N], [float(q) for q in Q], [float(p) for p in P], root_n, 1e-12)
        # nf = 0 for every child: N' = min(N, max(N - 0, need, 0)) = N
        assert list(got) == want == list(N), (N, Q, P, root_n, list(got))


def test_the_worked_example():
    """one root by hand: N = (10, 4, 1), R.N = 16, k = 2; sq = 4; star = 0.2 + (0.5 * 4) / 11"""
    N, Q, P = [10, 4, 1], [0.2, 0.0, -0.5], [0.5, 0.3, 0.2]
    star = 0.2 + (0.5 * 4.0) / 11.0
    # child 1: nf = int(sqrt(0.6 * 16)) = 3; want = (0.3 * 4) / star - 1 = 2.14...; need = 3; N' = max(4 - 3, 3) = 3
    assert int(math.sqrt((2.0 * 0.3) * 16.0)) == 3 and math.floor((0.3 * 4.0) / star - 1.0) == 2
    # child 2: nf = int(sqrt(0.4 * 16)) = 2; want = 0.8 / (star + 0.5) - 1 < 0; need = 0; N' = max(-1, 0, 0) = 0
    assert F.prune(N, Q, P, 16, 2.0) == [10, 3, 0]
    from alphazero_amd.engine import SelfPlayEngine
    assert list(SelfPlayEngine.forced_prune(N, Q, P, 16, 2.0)) == [10, 3, 0]
    assert [F.forced(n, p, 16, 2.0) for n, p in zip(N, P)] == [False, False, True]  # 100 < 16 and 16 < 9.6 are false, 1 < 6.4 is true


# ------------------------------------------------------------------------------------------------------------------ 2
BAD_FORMS = [0, 0.0, -1, -0.5, 64.5, 1e9, float("inf"), float("nan"), True, "2", (2,), [2.0], {"k": 2}]


@pytest.mark.parametrize("bad", BAD_FORMS)
def test_the_form_is_checked_where_the_option_is_given(bad):
    from alphazero_amd.engine import SelfPlayEngine
    from alphazero_amd.trainer import AlphaZeroTrainer
    with pytest.raises(ValueError, match=r"expected None or a number k in \(0, 64\]"):
        FP.parse(bad)
    with pytest.raises(ValueError, match=r"selfplay_forced_playouts=.*expected None or a number k in \(0, 64\]"):
        AlphaZeroTrainer(selfplay_forced_playouts=bad)
    eng = SelfPlayEngine.__new__(SelfPlayEngine)  # no engine behind it: the form is refused before the library is asked
    eng.h = None
    with pytest.raises(ValueError, match=r"forced_playouts=.*expected None or a number k in \(0, 64\]"):
        eng.set_forced_playouts(bad)


def test_valid_forms_and_the_trainers_refusals_name_the_other_mode():
    from alphazero_amd.trainer import AlphaZeroTrainer
    assert FP.parse(None) is None and FP.parse(2) == 2.0 and isinstance(FP.parse(2), float)
    assert FP.parse(np.float32(0.5)) == 0.5 and FP.parse(np.int64(64)) == 64.0 and FP.parse(1e-12) == 1e-12
    assert AlphaZeroTrainer().selfplay_forced_playouts is None
    assert AlphaZeroTrainer(selfplay_forced_playouts=2).selfplay_forced_playouts == 2
    t = AlphaZeroTrainer(selfplay_forced_playouts=2, selfplay_playout_cap=(25, 0.25))  # the two halves of the recipe combine
    assert t._check_selfplay_forced_playouts() == 2.0 and t._check_selfplay_playout_cap() == (25, 0.25)
    with pytest.raises(ValueError, match=r"selfplay_forced_playouts=2 does not combine with selfplay_gumbel=16"):
        AlphaZeroTrainer(selfplay_forced_playouts=2, selfplay_gumbel=16)
    with pytest.raises(ValueError, match=r"selfplay_forced_playouts=2 does not combine with selfplay_symmetry='random'"):
        AlphaZeroTrainer(selfplay_forced_playouts=2, selfplay_symmetry="random")
    t = AlphaZeroTrainer(selfplay_forced_playouts=2)
    t.selfplay_gumbel = 8  # set after construction: checked again before the engine is built
    with pytest.raises(ValueError, match="does not combine with selfplay_gumbel=8"):
        t._check_selfplay_forced_playouts()


def test_the_option_stays_a_self_play_device():
    """neither the arena's search spec nor the players take it"""
    import inspect
    from alphazero_amd import arena, players
    assert not any("forced" in k for k in arena.SEARCH_KEYS)
    for _, cls in inspect.getmembers(players, inspect.isclass):
        if cls.__module__ == players.__name__:
            assert not any("forced" in p for p in inspect.signature(cls.__init__).parameters), cls


# ------------------------------------------------------------------------------------------------------------------ 3
def test_the_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_engine_set_forced_playouts\(az_engine \*e, double k\);", hdr)
    assert re.search(r"int az_engine_forced_playouts_stats\(az_engine \*e, int64_t \*forced_picks, int64_t \*pruned_playouts\);", hdr)
    assert re.search(r"int az_forced_playout\(int32_t n, double p, int32_t root_n, double k\);", hdr)
    assert re.search(r"int az_forced_prune\(int32_t n_children, const int32_t \*N, const double \*Q, const double \*P, int32_t root_n, double k, int32_t \*out_N\);", hdr)
    names = ("az_engine_set_forced_playouts", "az_engine_forced_playouts_stats", "az_forced_playout", "az_forced_prune")
    assert set(names) <= set(_lib.SYMBOLS)
    L = _lib.lib()
    for s in names:
        assert hasattr(L, s), s
    assert L.az_version() >= 110
    assert L.az_engine_set_forced_playouts(None, 2.0) == _lib.AZ_EINVAL
    assert L.az_engine_forced_playouts_stats(None, None, None) == _lib.AZ_EINVAL
    assert L.az_forced_prune(3, None, None, None, 4, 2.0, None) == _lib.AZ_EINVAL
    assert L.az_forced_prune(-1, None, None, None, 4, 2.0, None) == _lib.AZ_EINVAL
    assert L.az_forced_prune(0, None, None, None, 4, 2.0, None) == _lib.AZ_OK
    with pytest.raises(ValueError, match="null engine"):
        _lib.check(L.az_engine_set_forced_playouts(None, 0.0))


def test_the_contract_is_stated_in_three_places():
    """above the setter in the header, above the code, in the model: each names the forced test and the pruned count as written"""
    texts = [open(os.path.join(ROOT, "include", "az_amd.h")).read(),
             open(os.path.join(ROOT, "alphazero_amd", "csrc", "az_engine.hip")).read(), F.__doc__]
    for t in texts:
        flat = re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)?", " ", t))  # line breaks and the comment's margin aside
        assert "< (k * c.P) *" in flat and "(c.P * sq) / gap - 1.0" in flat and "max(c.N - nf, need, 0)" in flat


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("cap", [None, F.CAP], ids=["cap off", "cap on"])
@pytest.mark.parametrize("tie", ["lowest", "random"])
@pytest.mark.parametrize("tag", ["othello6", "connect4", "tictactoe"])
def test_the_gpu_waves_exercise_the_mode(tag, tie, cap):
    arr, ctr = F.wave(tag, tie, cap)
    assert ctr["forced_picks"] > 0 and ctr["pruned_playouts"] > 0, ctr
    differs = (arr["pi"].view(np.uint32) != arr["raw_pi"].view(np.uint32)).any(axis=1)
    assert differs.any()
    assert np.array_equal(arr["visits"].sum(axis=1) > 0, np.ones(len(arr["z"]), bool))
    # pruning removes playouts from the target, never from the visits: pi is 0 wherever visits is 0, and sums to 1 in float32
    assert np.all(arr["pi"][arr["visits"] == 0] == 0.0)
    # (every entry is a double p_i rounded to float32, off by at most p_i 2^-24; the p_i sum to 1 within a few 2^-53: 2^-23 bounds it)
    assert np.all(np.abs(arr["pi"].astype(np.float64).sum(axis=1) - 1.0) <= 2.0 ** -23)
    if cap is None:
        assert ctr["fast_plies"] == 0 and ctr["samples"] == ctr["plies"]
    else:
        assert 0 < ctr["fast_plies"] and 0 < ctr["full_plies"] == ctr["samples"]


def test_the_model_without_the_mode_is_the_playout_cap_model():
    """k None: the wave loop, the move policy and the counters are playout_cap_model's, with the cap and without"""
    import playout_cap_model as PC
    for cap in (None, F.CAP):
        a = F.play_wave("tictactoe", 3, 3, 5, 0, 6, 12, None, cap, (0.03, 0.25), "random", 1, 5)
        b = PC.play_wave("tictactoe", 3, 3, 5, 0, 6, 12, cap, (0.03, 0.25), "random", 1, 5)
        for k in b[0]:
            assert np.array_equal(a[0][k], b[0][k]), k
        assert np.array_equal(a[0]["pi"], a[0]["raw_pi"])
        assert a[1]["forced_picks"] == 0 and a[1]["pruned_playouts"] == 0
        for k in b[1]:
            assert a[1][k] == b[1][k], k
