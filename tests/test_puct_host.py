"""CPU: the PUCT exploration settings (az_engine_set_puct) without a GPU.

  1. the spec parser (alphazero_amd/puct.py) and every refusal message, where the option is given: MCT, the players, the arena's search
     spec, the trainer;
  2. az_puct_c / az_puct_key -- the functions the kernels call, as host code -- against the model's arithmetic (tests/puct_model.py), bit
     for bit, on seeded random inputs that include vis = 0, parent_n = 0, p = 0 and c_base at both ends of its range;
  3. the ABI: the four symbols are declared with their signatures, listed and exported; null handles and out-of-range values are
     AZ_EINVAL;
  4. the neutral triple through the model is leaf_batch_model.Model's own wave, array for array;
  5. for every setting and board tests/test_gpu_puct.py plays, the model's wave differs from the plain wave in `visits` (without this
     the GPU comparison would show nothing); on the wide root, first-play urgency changes a selection among the children of index 16
     or more, and the vis sum is not the plain ascending one there."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import puct_model as PM
from alphazero_amd import _lib
from alphazero_amd import puct as PU
from conftest import ROOT


def bits(x):
    return np.float64(x).view(np.int64)


# ------------------------------------------------------------------------------------------------------------------ 1
def test_valid_forms():
    assert PU.parse(None) == PU.OFF == (1.0, 0.0, -1.0) and not PU.is_on(PU.parse(None))
    assert PU.parse(2.5) == (2.5, 0.0, -1.0) and PU.parse(2) == (2.0, 0.0, -1.0) and PU.parse(np.float32(0.5)) == (0.5, 0.0, -1.0)
    assert PU.parse({}) == PU.OFF and PU.parse(1) == PU.OFF and PU.parse({"c_init": 1.0, "c_base": 0, "fpu": -3}) == PU.OFF
    assert PU.parse({"c_init": 1.25, "c_base": 19652, "fpu": 0.25}) == (1.25, 19652.0, 0.25)
    assert PU.parse({"fpu": 0}) == (1.0, 0.0, 0.0) and PU.is_on(PU.parse({"fpu": 0}))
    assert PU.parse({"fpu": None}) == PU.OFF and PU.parse({"fpu": float("-inf")}) == PU.OFF
    assert PU.parse({"c_base": 1}) == (1.0, 1.0, -1.0) and PU.parse({"c_base": 1e9, "c_init": 64, "fpu": 4}) == (64.0, 1e9, 4.0)
    assert all(isinstance(x, float) for x in PU.parse({"c_init": np.int64(2), "c_base": np.int32(8)}))


@pytest.mark.parametrize("bad,msg", [
    ("1.25", "expected None, a number"), ((1.25, 0, -1), "expected None, a number"), ([2.0], "expected None, a number"),
    (True, "expected None, a number"), ({"c_puct": 2}, r"unknown key\(s\) \['c_puct'\]"), ({"c_init": 1, "cbase": 8}, r"unknown key\(s\) \['cbase'\]"),
    (0, "c_init must be finite and in"), (-1.0, "c_init must be finite and in"), (64.5, "c_init must be finite and in"),
    (float("inf"), "c_init must be finite and in"), (float("nan"), "c_init must be finite and in"),
    ({"c_init": "2"}, "c_init must be a number"), ({"c_init": True}, "c_init must be a number"),
    ({"c_base": 0.5}, "c_base must be 0"), ({"c_base": -1}, "c_base must be 0"), ({"c_base": 2e9}, "c_base must be 0"),
    ({"c_base": float("nan")}, "c_base must be 0"), ({"c_base": float("inf")}, "c_base must be 0"), ({"c_base": None}, "c_base must be a number"),
    ({"fpu": 4.5}, "fpu must be None or negative"), ({"fpu": float("nan")}, "fpu must be None or negative"),
    ({"fpu": float("inf")}, "fpu must be None or negative"), ({"fpu": "0.25"}, "fpu must be a number")])
def test_the_form_is_checked_where_the_option_is_given(bad, msg):
    from alphazero_amd.arena import check_search
    from alphazero_amd.engine import SelfPlayEngine
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    from alphazero_amd.trainer import AlphaZeroTrainer
    with pytest.raises(ValueError, match="puct=.*" + msg):
        PU.parse(bad)
    with pytest.raises(ValueError, match="selfplay_puct=.*" + msg):
        AlphaZeroTrainer(selfplay_puct=bad)
    for make in (lambda: MCT(eval_method="neural", puct=bad), lambda: AlphaZeroPlayer(n_sim=4, puct=bad),
                 lambda: BatchedAlphaZeroPlayer(n_sim=4, n_slots=2, puct=bad), lambda: check_search({"puct": bad}, None)):
        with pytest.raises(ValueError, match="puct=.*" + msg):
            make()
    eng = SelfPlayEngine.__new__(SelfPlayEngine)  # no engine behind it: the form is refused before the library is asked
    eng.h = None
    with pytest.raises(ValueError, match="puct=.*" + msg):
        eng.set_puct(bad)


ON = {"c_init": 1.25, "c_base": 19652, "fpu": 0.25}


def test_every_refusal_names_both_options():
    from alphazero_amd.arena import check_search
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    from alphazero_amd.trainer import AlphaZeroTrainer
    others = [("symmetry", "all"), ("symmetry", "random"), ("leaf_batch", 4), ("gumbel", 8), ("exact_endgame", 6), ("proof_backup", True)]
    for key, val in others:
        for cls, kw in ((MCT, dict(eval_method="neural")), (AlphaZeroPlayer, dict(n_sim=4)), (BatchedAlphaZeroPlayer, dict(n_sim=4, n_slots=2))):
            with pytest.raises(ValueError, match=rf"puct=.* does not combine with {key}={val!r}: PUCT exploration settings are served in the plain"):
                cls(puct=ON, **{key: val}, **kw)
            cls(puct=None, **{key: val}, **kw)                      # off combines with everything
            cls(puct={"c_init": 1.0, "fpu": -1}, **{key: val}, **kw)   # and so does the neutral triple
    for key, val in others[:4]:
        with pytest.raises(ValueError, match=rf"puct=.* does not combine with {key}={val!r}"):
            check_search({"puct": ON, key: val}, None)
    assert check_search({"puct": ON}, None)["puct"] == ON and check_search({"puct": ON}, "fake")["puct"] == ON
    assert check_search({"gumbel": 8}, None)["puct"] is None
    with pytest.raises(ValueError, match="puct=.* needs eval_method 'neural': a rollout tree"):
        MCT(eval_method="rollout", puct=ON)
    with pytest.raises(ValueError, match="puct=.* needs eval_method 'neural': a rollout tree"):
        check_search({"puct": ON}, "mcts")
    with pytest.raises(ValueError, match="has no search tree"):
        check_search({"puct": ON}, "random")
    for key, val in (("selfplay_gumbel", 16), ("selfplay_symmetry", "random"), ("selfplay_playout_cap", (4, 0.5)), ("selfplay_forced_playouts", 2),
                     ("selfplay_exact_endgame", 6), ("selfplay_proof_backup", True)):
        with pytest.raises(ValueError, match=rf"selfplay_puct=.* does not combine with {key}={re.escape(repr(val))}"):
            AlphaZeroTrainer(selfplay_puct=ON, **{key: val})
        AlphaZeroTrainer(selfplay_puct=None, **{key: val})
    t = AlphaZeroTrainer(selfplay_puct=ON)
    assert t._check_selfplay_puct() == (1.25, 19652.0, 0.25) and AlphaZeroTrainer()._check_selfplay_puct() == PU.OFF
    t.selfplay_gumbel = 8  # set after construction: checked again before the engine is built
    with pytest.raises(ValueError, match="does not combine with selfplay_gumbel=8"):
        t._check_selfplay_puct()
    # eval_search "selfplay" hands the settings to the arena, and only when there are some
    assert AlphaZeroTrainer(selfplay_puct=ON, eval_search="selfplay")._eval_search_spec()["puct"] == ON
    assert "puct" not in AlphaZeroTrainer(eval_search="selfplay")._eval_search_spec()
    assert AlphaZeroTrainer(eval_search={"puct": 2.5})._eval_search_spec() == {"puct": 2.5}


def test_an_external_network_is_refused_by_name():
    from alphazero_amd.base import PolicyValueNetwork
    from alphazero_amd.mcts import MCT

    class Other(PolicyValueNetwork):  # no HIP route: its leaves go through the external evaluator
        pass

    nn = Other.__new__(Other)
    from alphazero_amd.evaluators import route
    assert route(nn) != "hip"
    with pytest.raises(ValueError, match="puct=.* needs a network the HIP network serves; Other evaluates its leaves through an external evaluator"):
        PU.check_puct(ON, nn)
    assert PU.check_puct(None, nn) == PU.OFF
    with pytest.raises(ValueError, match="Other evaluates its leaves through an external evaluator"):
        MCT(eval_method="neural", nn=nn, puct=ON)


def test_clones_keep_the_settings():
    from alphazero_amd.players import AlphaZeroPlayer, BatchedAlphaZeroPlayer
    p = AlphaZeroPlayer(n_sim=4, puct=ON)
    assert p.puct == ON and p.mct.puct == ON and p.clone().puct == ON
    p.reset()
    assert p.puct == ON and p.mct._engine_puct == PU.OFF
    assert AlphaZeroPlayer(n_sim=4).puct is None and BatchedAlphaZeroPlayer(n_sim=4, n_slots=2, puct=2.5).puct == 2.5


# ------------------------------------------------------------------------------------------------------------------ 2
C_BASES = (0.0, 1.0, 8.0, 19652.0, 1e9)


def _inputs(n, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        parent_n = int(rng.choice([0, 1, 2, 3, 12, 100, 799, 2**31 - 1])) if i % 3 == 0 else int(rng.integers(0, 5000))
        n_child = 0 if i % 2 == 0 else int(rng.integers(0, parent_n + 1))
        p = 0.0 if i % 17 == 0 else float(rng.random())
        vis = 0.0 if i % 5 == 0 else float(rng.random())
        fpu = -1.0 if i % 4 == 0 else float(rng.choice([0.0, 0.25, 1.0, 4.0, rng.random() * 4.0]))
        out.append((float(rng.uniform(-1, 1)), p, n_child, parent_n, float(rng.uniform(-1, 1)), vis,
                    float(rng.choice([1.0, 1.25, 2.5, 64.0, rng.uniform(1e-3, 64.0)])), float(C_BASES[i % len(C_BASES)]), fpu))
    return out


def test_the_host_arithmetic_is_the_models_bit_for_bit():
    L = _lib.lib()
    ins = _inputs(4000)
    assert any(x[5] == 0.0 and x[2] == 0 and x[8] >= 0 for x in ins) and any(x[3] == 0 for x in ins) and any(x[1] == 0.0 for x in ins)
    assert {x[7] for x in ins} == set(C_BASES)
    for q, p, n, pn, pq, vis, c_init, c_base, fpu in ins:
        assert bits(L.az_puct_c(pn, c_init, c_base)) == bits(PM.c_of(pn, c_init, c_base)), (pn, c_init, c_base)
        got, want = L.az_puct_key(q, p, n, pn, pq, vis, c_init, c_base, fpu), PM.key_of(q, p, n, pn, pq, vis, c_init, c_base, fpu)
        assert bits(got) == bits(want), (q, p, n, pn, pq, vis, c_init, c_base, fpu, got, want)


def test_the_neutral_triple_is_the_reference_key():
    L = _lib.lib()
    for q, p, n, pn, pq, vis, _, _, _ in _inputs(500, seed=6):
        plain = q + (p * math.sqrt(float(pn))) / float(1 + n)
        assert bits(L.az_puct_key(q, p, n, pn, pq, vis, 1.0, 0.0, -1.0)) == bits(plain) == bits(PM.key_of(q, p, n, pn, pq, vis, *PM.OFF))
        assert L.az_puct_c(pn, 1.0, 0.0) == 1.0


def test_a_worked_example():
    """parent of 10 visits and Q = 0.2, (1.25, 8, 0.25): c = 1.25 + log(19 / 8); an unvisited child of prior 0.3 under a visited mass of 0.5"""
    L = _lib.lib()
    c = 1.25 + PM.det_log(((1.0 + 10.0) + 8.0) / 8.0)
    assert abs(c - (1.25 + math.log(19.0 / 8.0))) < 1e-12 and bits(L.az_puct_c(10, 1.25, 8.0)) == bits(c)
    want = ((-0.2) - 0.25 * math.sqrt(0.5)) + ((c * 0.3) * math.sqrt(10.0)) / 1.0
    assert bits(L.az_puct_key(0.7, 0.3, 0, 10, 0.2, 0.5, 1.25, 8.0, 0.25)) == bits(want)   # an unvisited child's own Q is not read
    visited = 0.7 + ((c * 0.3) * math.sqrt(10.0)) / 4.0
    assert bits(L.az_puct_key(0.7, 0.3, 3, 10, 0.2, 0.5, 1.25, 8.0, 0.25)) == bits(visited)  # a visited one keeps it


def test_vis_is_summed_in_lane_and_stride_order():
    rng = np.random.default_rng(8)
    differs = 0
    for k in (1, 7, 16, 17, 34, 64):
        for _ in range(50):
            P = [float(x) for x in rng.dirichlet(np.ones(k))]
            N = [int(x) for x in rng.integers(0, 3, k)]
            v = PM.vis_of(N, P)
            exact = math.fsum(p for n, p in zip(N, P) if n > 0)
            assert abs(v - exact) <= 64 * 2.0 ** -53  # at most 63 additions of terms that sum to at most 1
            seq = 0.0
            for n, p in zip(N, P):
                seq = seq + (p if n > 0 else 0.0)
            differs += bits(seq) != bits(v)
    assert differs > 0  # the order is part of the contract: the ascending sum is another number
    assert PM.vis_of([0, 0, 0], [0.2, 0.3, 0.5]) == 0.0 and PM.vis_of([], []) == 0.0


# ------------------------------------------------------------------------------------------------------------------ 3
def test_the_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_engine_set_puct\(az_engine \*e, double c_init, double c_base, double fpu\);", hdr)
    assert re.search(r"int az_engine_puct\(az_engine \*e, double \*c_init, double \*c_base, double \*fpu\);", hdr)
    assert re.search(r"double az_puct_c\(int32_t parent_n, double c_init, double c_base\);", hdr)
    assert re.search(r"double az_puct_key\(double q_child, double p_child, int32_t n_child, int32_t parent_n, double parent_q, double vis,\s+"
                     r"double c_init, double c_base, double fpu\);", hdr)
    names = ("az_engine_set_puct", "az_engine_puct", "az_puct_c", "az_puct_key")
    assert set(names) <= set(_lib.SYMBOLS)
    L = _lib.lib()
    for s in names:
        assert hasattr(L, s), s
    assert L.az_version() >= 116
    assert L.az_engine_set_puct(None, 1.25, 19652.0, 0.25) == _lib.AZ_EINVAL
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    assert L.az_engine_puct(None, C.byref(a), C.byref(b), C.byref(c)) == _lib.AZ_EINVAL
    with pytest.raises(ValueError, match="null engine"):
        _lib.check(L.az_engine_set_puct(None, 1.0, 0.0, -1.0))


def test_the_contract_is_stated_in_the_header_the_code_and_the_model():
    texts = [open(os.path.join(ROOT, "include", "az_amd.h")).read(), PM.__doc__]
    for t in texts:
        flat = re.sub(r"\s+", " ", re.sub(r"\n\s*(\*|//)?", " ", t))  # line breaks and the comment's margin aside
        assert "(-p.Q) - fpu * sqrt(vis)" in flat and "q + ((c * c.P) * sq) /" in flat and "1, 2, 4, 8" in flat
    src = open(os.path.join(ROOT, "alphazero_amd", "csrc", "az_engine.hip")).read()
    assert "(-parent_q) - fpu * sqrt(vis)" in src and "q + ((c * p_child) * sq) / (double)(1 + n_child)" in src


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("tag,tie", [("tictactoe", "random"), ("tictactoe", "lowest"), ("othello6", "random")])
def test_the_neutral_triple_is_the_plain_model(tag, tie):
    game, _, H, W = PM.GAMES[tag]
    n = 6
    a, ca = PM.play_wave(game, H, W, PM.SEED, PM.FIRST, n, PM.N_SIMS[tag], PM.OFF, PM.NOISE, tie, PM.TMAX, PM.TMIN)
    b, cb = PM.PC.play_wave(game, H, W, PM.SEED, PM.FIRST, n, PM.N_SIMS[tag], None, PM.NOISE, tie, PM.TMAX, PM.TMIN)
    for k in b:
        assert a[k].shape == b[k].shape and np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k
    assert (ca["samples"], ca["rows"]) == (cb["samples"], cb["rows"])


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("tag,tie,puct", PM.WAVES, ids=[f"{t}-{tie}-{p}" for t, tie, p in PM.WAVES])
def test_the_gpu_waves_exercise_the_settings(tag, tie, puct):
    arr, ctr = PM.wave(tag, tie, puct)
    plain, _ = PM.plain_wave(tag, tie)
    assert ctr["samples"] == ctr["plies"] == len(arr["z"]) and np.all(arr["visits"].sum(axis=1) > 0)
    # ply 0 of every game is searched from the same fresh root under either key: the first sample's visits already differ somewhere
    first, pfirst = arr["visits"][arr["meta"][:, 1] == 0], plain["visits"][plain["meta"][:, 1] == 0]
    assert first.shape == pfirst.shape == (PM.N_GAMES, arr["visits"].shape[1])
    assert (first != pfirst).any(), "the settings never changed a first ply's visit counts: the GPU comparison would show nothing"
    assert arr["visits"].shape != plain["visits"].shape or (arr["visits"] != plain["visits"]).any()


def test_the_settings_differ_from_each_other():
    """the four settings on othello6 are four different waves: no test of one passes on another's kernel arguments"""
    waves = [PM.wave("othello6", "random", p)[0]["visits"] for p in (PM.FULL, (2.5, 0.0, -1.0), (1.0, 8.0, -1.0), (1.0, 0.0, 0.25))]
    for i in range(len(waves)):
        for j in range(i):
            assert waves[i].shape != waves[j].shape or (waves[i] != waves[j]).any(), (i, j)


@pytest.mark.parametrize("tie", ["lowest", "random"])
def test_on_the_wide_root_fpu_changes_a_selection_among_the_high_children(tie):
    for gid in PM.WIDE_GIDS:
        m = PM.wide_root(tie, gid)
        assert len(m.root.children) == 34 and m.root.N == PM.WIDE_SIMS
        assert m.high_fpu_picks > 0, "first-play urgency never changed a selection of a child in the second or third round of 16 lanes"
        N, P = [c.N for c in m.root.children], [c.P for c in m.root.children]
        assert sum(1 for n in N[16:] if n > 0) > 0  # visited children beyond the first round: vis crosses rounds and lanes
