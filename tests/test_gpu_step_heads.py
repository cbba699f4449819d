"""GPU: the policy / value heads computed inside the search step kernel (k_step_heads).  Where the form is in force a
lock-step's forward stops behind fc2 and the step kernel computes the heads of its own block's rows with k_heads2's arithmetic; the
samples must not change by a bit.

Every case plays the real OthelloNet under torch.manual_seed(0), its BatchNorm statistics moved off their initial values, with the
defaults of self-play (Dirichlet noise from the Philox stream, random tie-break).  The cases run once per setting of
AZ_ENGINE_STEP_HEADS -- 1 and 0 -- in a child process each (the switch is read when an engine is created).  A child saves, per case, a
digest of every sample array in (game id, move index) order, the counters, and the rows of the first and the last game id; the tests
hold switch 1 == switch 0 on the digests and both to the oracle's replay of those two games, bit for bit.  Whole games throughout (a
run cannot stop after a few plies): the opening's cached plies, the mid-game and the last plies are all in every case.
  1. 1, 17 and 48 slots at 8 simulations: inert groups, a block with one live group, blocks of mixed rows.
  2. 16 slots at 16 simulations: the last plies have blocks in which every leaf is terminal.
  3. 2112 slots as two groups against one (4 simulations; the cache is in force there by its rule: k_step_heads<., true, 5> beside
     another chain, each chain reading its own lane's rows).
  4. the cache with hits, tables of 8 entries and of 1: the payload copied out of LDS is what a later hit reads.
  5. refill: 48 games through 17 slots.
  6. a second weight set committed between two runs of one engine.
  7. OthelloNet 6x6 (48 padded logits: three tiles), 48 slots.
  8. every mode the form is not served for, under switch 1: the run reports the old kernels and equals its switch-0 run.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
KEYS = ("state", "pi", "z", "meta", "visits")
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 3
UNSERVED = ("cap", "forced", "exact", "proof", "puct", "gumbel", "leaf_batch", "sym", "symr", "fake", "rollout", "external", "profiled", "search")


def state_dict(seed, n=8):
    """OthelloNet(n) as torch initialises it under the seed, with BatchNorm running statistics and affine terms drawn off their initial
    0 / 1 (a freshly made net normalises with mean 0, variance 1: the folded kernels would never see another scale)"""
    import torch
    from alphazero_amd.games.othello import OthelloNet
    torch.manual_seed(seed)
    net = OthelloNet(n=n).eval()
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        for name, m in net.named_modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
                m.weight.copy_(0.75 + 0.5 * torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    return {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).digest(), np.uint8).copy()


def child_cases(out):
    """runs in the child: every case under the AZ_ENGINE_STEP_HEADS of its environment, saved as one npz"""
    import torch
    from alphazero_amd import engine as E
    res, on = {}, os.environ["AZ_ENGINE_STEP_HEADS"] == "1"

    def wave(tag, eng, games, served=True, **run_kw):
        assert eng.step_heads()["in_force"] == (on and served), (tag, eng.step_heads())
        got = eng.run(games, **run_kw)
        assert eng.step_heads()["used"] == (on and served), (tag, eng.step_heads())
        meta = got["meta"].cpu().numpy()
        order = np.lexsort((meta[:, 1], meta[:, 0]))
        ids = meta[order, 0]
        first = run_kw.get("first_game_id", 0)
        for k in KEYS:
            a = got[k].cpu().numpy()[order]
            res[f"{tag}/{k}/sha"] = digest(a)
            res[f"{tag}/{k}/first"] = a[ids == first]
            res[f"{tag}/{k}/last"] = a[ids == first + games - 1]
        st = eng.stats()
        assert st["error_flags"] == 0 and st["games_done"] == games, (tag, st)
        res[f"{tag}/counts"] = np.array([st["net_evals"], st["cache_hits"], st["games_done"], st["samples"], int(eng.step_heads()["used"])], np.int64)

    net = E.HipNet(0, 8, 8, state_dict(0), max_batch=2112)

    def engine(slots, n_sim, **kw):
        return E.SelfPlayEngine(0, 8, 8, n_slots=slots, n_sim=n_sim, net=net, seed=SEED, **kw)

    for slots in (1, 17, 48):  # 1
        eng = engine(slots, 8)
        wave(f"slots{slots}", eng, slots)
        eng.close()
    eng = engine(16, 16)  # 2
    wave("terminal", eng, 16)
    eng.close()
    for groups in (1, 2):  # 3
        eng = engine(2112, 4, groups=groups)
        assert eng.groups() == groups and eng.eval_cache_stats()["in_force"]
        wave(f"groups{groups}", eng, 2112)
        eng.close()
    eng = engine(64, 16)  # 4
    for cap in (8, 1):
        eng.set_eval_cache(True, capacity=cap)
        wave(f"cap{cap}", eng, 64)
    eng.close()
    eng = engine(17, 8, sample_capacity=48 * 128)  # 5
    wave("refill17", eng, 48)
    eng.close()
    eng = engine(16, 8)  # 6
    wave("w0", eng, 16)
    wave("w0_again", eng, 16)  # the searches replay as graphs from here on
    net.load_state_dict(state_dict(1))
    wave("w1", eng, 16)
    eng.close()
    eng = engine(16, 8)
    wave("w1_fresh", eng, 16)
    eng.close()
    net.load_state_dict(state_dict(0))
    net6 = E.HipNet(0, 6, 6, state_dict(0, n=6), max_batch=64)  # 7
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=48, n_sim=8, net=net6, seed=SEED)
    wave("othello6", eng, 48)
    eng.close()
    for mode in UNSERVED:  # 8
        if mode in ("fake", "rollout", "external"):
            ev = {"fake": E.EVAL_FAKE, "rollout": E.EVAL_ROLLOUT, "external": E.EVAL_EXTERNAL}[mode]
            eng = E.SelfPlayEngine(0, 8, 8, n_slots=16, n_sim=8, evaluator=ev, seed=SEED)
            if mode == "external":
                eng.set_evaluator(lambda b: net.forward_dyn(b.x, b.count, probs=b.probs, v=b.value))
        else:
            eng = engine(16, 8)
        if mode == "cap":
            eng.set_playout_cap((4, 0.5))
        elif mode == "forced":
            eng.set_forced_playouts(2.0)
        elif mode == "exact":
            eng.set_exact_endgame(6)
        elif mode == "proof":
            eng.set_proof_backup(True)
        elif mode == "puct":
            eng.set_puct(1.5, 1000.0, 0.2)
        elif mode == "gumbel":
            eng.set_gumbel(4)
        elif mode == "leaf_batch":
            eng.set_leaf_batch(2)
        elif mode == "sym":
            eng.set_symmetry("all")
        elif mode == "symr":
            eng.set_symmetry("random")
        if mode == "profiled":
            net.profile(True)
        try:
            if mode == "search":  # az_engine_search on the start position: never the form, whatever the switch says
                grids = np.zeros((16, 8, 8), np.int8)
                grids[:, 3, 3] = grids[:, 4, 4] = 1
                grids[:, 3, 4] = grids[:, 4, 3] = -1
                eng.set_roots(grids, np.ones(16, np.int8))
                eng.search(24)
                assert not eng.step_heads()["used"]
                res["unserved_search/visits"] = np.concatenate([np.stack(eng.root_children(s)[:2]).ravel() for s in range(16)])
                res["unserved_search/Q"] = np.concatenate([eng.root_children(s)[2] for s in range(16)])
            else:
                wave(f"unserved_{mode}", eng, 16, served=False)
        finally:
            if mode == "profiled":
                net.profile(False)
        eng.close()
    torch.cuda.synchronize()
    np.savez(out, **res)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{switch: the child's arrays} for AZ_ENGINE_STEP_HEADS = "1" and "0"; the children run one after the other"""
    out = {}
    for switch in ("1", "0"):
        path = str(tmp_path_factory.mktemp("step_heads") / f"cases_{switch}.npz")
        code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_step_heads as T; T.child_cases(sys.argv[1])" % (ROOT, HERE)
        subprocess.check_call([sys.executable, "-c", code, path], env=dict(os.environ, AZ_ENGINE_STEP_HEADS=switch), timeout=600)
        with np.load(path) as z:
            out[switch] = {k: z[k] for k in z.files}
    return out


_ORACLE = {}


def oracle_game(n, seed_w, n_sim, g):
    """one game replayed alone by the oracle, once per (net, simulations, game id)"""
    from oracle import oracle as O
    key = (n, seed_w, n_sim, g)
    if key not in _ORACLE:
        if (n, seed_w) not in _ORACLE:
            _ORACLE[(n, seed_w)] = ("conv", O.ConvNet(O.OTHELLO, n, n, state_dict(seed_w, n=n)))
        _ORACLE[key] = O.selfplay(O.OTHELLO, n, n, 1, n_sim, _ORACLE[(n, seed_w)], seed=SEED, first_game_id=g)
    return _ORACLE[key]


def same(a, ta, b, tb):
    for k in KEYS:
        assert np.array_equal(a[f"{ta}/{k}/sha"], b[f"{tb}/{k}/sha"]), (ta, tb, k)
    assert np.array_equal(a[f"{ta}/counts"][[0, 2, 3]], b[f"{tb}/counts"][[0, 2, 3]]), (ta, tb, a[f"{ta}/counts"], b[f"{tb}/counts"])


def fused_equals_unfused_equals_oracle(runs, tag, n_sim, games, first=0, n=8, seed_w=0):
    on, off = runs["1"], runs["0"]
    assert on[f"{tag}/counts"][4] == 1 and off[f"{tag}/counts"][4] == 0, tag  # the form ran in one child and not in the other
    same(on, tag, off, tag)
    for which, g in (("first", first), ("last", first + games - 1)):
        ref = oracle_game(n, seed_w, n_sim, g)
        for k in KEYS:
            for leg in (on, off):
                got = leg[f"{tag}/{k}/{which}"]
                assert got.shape == ref[k].shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(ref[k]).view(np.uint8)), (tag, g, k)
    print(tag, "net_evals", on[f"{tag}/counts"][0], "cache_hits on / off", on[f"{tag}/counts"][1], off[f"{tag}/counts"][1])


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("slots", [1, 17, 48])
def test_slot_counts(runs, slots):
    fused_equals_unfused_equals_oracle(runs, f"slots{slots}", 8, slots)


# ------------------------------------------------------------------------------------------------------------------ 2
def test_blocks_of_terminal_leaves(runs):
    fused_equals_unfused_equals_oracle(runs, "terminal", 16, 16)


# ------------------------------------------------------------------------------------------------------------------ 3
def test_two_groups_against_one(runs):
    fused_equals_unfused_equals_oracle(runs, "groups1", 4, 2112)
    fused_equals_unfused_equals_oracle(runs, "groups2", 4, 2112)
    same(runs["1"], "groups2", runs["1"], "groups1")
    assert runs["1"]["groups1/counts"][1] > 0 and runs["1"]["groups2/counts"][1] > 0  # the cache was hit: k_step_heads' cached form ran


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("cap", [8, 1])
def test_cache_payload_from_lds(runs, cap):
    fused_equals_unfused_equals_oracle(runs, f"cap{cap}", 16, 64)
    assert runs["1"][f"cap{cap}/counts"][1] > 0, "cache_hits"


# ------------------------------------------------------------------------------------------------------------------ 5
def test_refill(runs):
    fused_equals_unfused_equals_oracle(runs, "refill17", 8, 48)


# ------------------------------------------------------------------------------------------------------------------ 6
def test_weights_changed_between_two_runs(runs):
    fused_equals_unfused_equals_oracle(runs, "w0", 8, 16)
    fused_equals_unfused_equals_oracle(runs, "w0_again", 8, 16)
    fused_equals_unfused_equals_oracle(runs, "w1", 8, 16, seed_w=1)
    fused_equals_unfused_equals_oracle(runs, "w1_fresh", 8, 16, seed_w=1)
    same(runs["1"], "w1", runs["1"], "w1_fresh")
    assert not np.array_equal(runs["1"]["w1/pi/sha"], runs["1"]["w0/pi/sha"])


# ------------------------------------------------------------------------------------------------------------------ 7
def test_othello_6x6(runs):
    fused_equals_unfused_equals_oracle(runs, "othello6", 8, 48, n=6)


# ------------------------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("mode", UNSERVED)
def test_unserved_modes_keep_the_old_kernels(runs, mode):
    on, off = runs["1"], runs["0"]
    if mode == "search":
        for k in ("visits", "Q"):
            assert np.array_equal(on[f"unserved_search/{k}"].view(np.uint8), off[f"unserved_search/{k}"].view(np.uint8)), k
        assert on["unserved_search/visits"].sum() > 0
        return
    tag = f"unserved_{mode}"
    assert on[f"{tag}/counts"][4] == 0 and off[f"{tag}/counts"][4] == 0
    same(on, tag, off, tag)
    assert on[f"{tag}/counts"][3] > 0
