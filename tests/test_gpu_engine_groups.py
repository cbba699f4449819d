"""GPU: az_engine_run as slot groups (az_engine_set_groups).  The slots are split into contiguous groups, each a
launch chain of its own on its own stream with its own leaf-row counters, network rows, net lane and search graph.  A game depends on
(seed, game id) only and a network row on its board only, so a grouped run must give the samples of the one-group run of the same
build bit for bit once they are in (game id, move index) order, and the same counters."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, TAGS
from alphazero_amd import _lib
from alphazero_amd import engine as E

pytestmark = pytest.mark.gpu
KEYS = ("state", "pi", "z", "meta", "visits")
STATS = ("games_done", "samples", "plies", "net_evals", "lockstep_iters", "error_flags")
_CACHE = {}


def sort_samples(d):
    meta = d["meta"] if isinstance(d["meta"], np.ndarray) else d["meta"].cpu().numpy()
    order = np.lexsort((meta[:, 1], meta[:, 0]))
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy())[order] for k, v in d.items()}


def fake_engine(slots, groups, **kw):
    game, gid, H, W, A, n = TAGS["othello6"]
    kw.setdefault("node_capacity", 8192)
    return E.SelfPlayEngine(gid, H, W, n_slots=slots, n_sim=20, evaluator=E.EVAL_FAKE, seed=1, groups=groups, **kw)


def fake_run(slots, games, groups):
    """(sorted samples, stats) of the fake-evaluator run; the one-group reference is computed once and shared"""
    key = ("fake", slots, games, groups)
    if groups != 1 or key not in _CACHE:
        eng = fake_engine(slots, groups, sample_capacity=games * 72)
        assert eng.groups() == groups
        out = (sort_samples(eng.run(games)), eng.stats())
        eng.close()
        if groups != 1:
            return out
        _CACHE[key] = out
    return _CACHE[key]


def same(got, ref):
    (a, sa), (b, sb) = got, ref
    for k in STATS:
        print(k, sa[k], sb[k])
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    for k in STATS:
        assert sa[k] == sb[k], (k, sa[k], sb[k])


@pytest.mark.parametrize("groups", [2, 4])
@pytest.mark.parametrize("slots,games", [(32, 32), (40, 40), (64, 64 * 3 + 1)])
def test_fake_evaluator_groups_equal_one_group(slots, games, groups):
    """32 slots: equal groups; 40: unequal groups, the last one not filling a block; 64 slots and 193 games: refill across groups and a
    last wave in which all but one group are empty"""
    same(fake_run(slots, games, groups), fake_run(slots, games, 1))


def get_net(kind):
    if kind not in _CACHE:
        torch.manual_seed(0)
        if kind == "othello":
            from alphazero_amd.games.othello import OthelloNet
            _CACHE[kind] = (0, 8, 8, OthelloNet(n=8).eval().to_hip(max_batch=64))
        else:
            from alphazero_amd.games.connect4 import Connect4Net
            _CACHE[kind] = (1, 6, 7, Connect4Net(7, 6).eval().to_hip(max_batch=64))
    return _CACHE[kind]


def net_run(kind, slots, games, groups):
    key = ("net", kind, slots, games, groups)
    if groups != 1 or key not in _CACHE:
        gid, H, W, net = get_net(kind)
        eng = E.SelfPlayEngine(gid, H, W, n_slots=slots, n_sim=8, net=net, seed=2, groups=groups)
        assert eng.groups() == groups
        out = (sort_samples(eng.run(games)), eng.stats())
        eng.close()
        if groups != 1:
            return out
        _CACHE[key] = out
    return _CACHE[key]


@pytest.mark.parametrize("kind,slots", [("othello", 64), ("connect4", 48)])
def test_real_network_two_forwards_on_one_net(kind, slots):
    """two groups put two forwards in flight on one az_net: each on its own lane of activation rows (Connect4Net: the fused tail)"""
    same(net_run(kind, slots, slots, 2), net_run(kind, slots, slots, 1))


def test_a_group_that_never_holds_a_game():
    """5 games on 40 slots, 2 groups: slots 32 .. 39 stay empty; the run ends and the second group plays nothing"""
    same(fake_run(40, 5, 2), fake_run(40, 5, 1))


def test_groups_replay_their_own_graphs():
    """every group captures and replays its own linear graph; without graphs (fresh process) the grouped run gives the same samples"""
    a, st = fake_run(32, 32, 2)
    assert st["graph_replays"] > 0
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import numpy as np\n"
            "from test_gpu_engine_groups import fake_engine, sort_samples\n"
            "eng = fake_engine(32, 2); assert eng.groups() == 2\n"
            "s = sort_samples(eng.run(32)); assert eng.stats()['graph_replays'] == 0\n"
            "np.savez(sys.argv[1], **s)\n") % (ROOT, os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "az_groups_nograph_%d.npz" % os.getpid())
    subprocess.check_call([sys.executable, "-c", code, out], env=dict(os.environ, AZ_ENGINE_GRAPHS="0"))
    b = np.load(out)
    os.remove(out)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


def test_profiling_runs_one_group():
    """under az_net_profile the run is today's launch sequence (one group): same samples, every kernel family that fired has a positive
    time; with profiling off the groups are back"""
    ref = net_run("othello", 64, 64, 1)
    gid, H, W, net = get_net("othello")
    eng = E.SelfPlayEngine(gid, H, W, n_slots=64, n_sim=8, net=net, seed=2, groups=2)
    net.profile(True)
    try:
        assert eng.groups() == 1
        got = (sort_samples(eng.run(64)), eng.stats())
        prof = net.profile_read()
    finally:
        net.profile(False)
    same(got, ref)
    fired = {k: v for k, v in prof.items() if v[1] > 0}
    assert fired and all(v[0] > 0 for v in fired.values()), prof
    assert eng.groups() == 2
    same((sort_samples(eng.run(64)), eng.stats()), ref)
    eng.close()


def test_capacity_error_is_reported_from_a_group():
    """a node pool too small for the search: the capacity error of the one-group run, as loudly, with two groups"""
    msgs = []
    for groups in (1, 2):
        eng = fake_engine(40, groups, node_capacity=160)
        with pytest.raises(_lib.AzError, match=r"\[-4\].*node pool") as ei:
            eng.run(40)
        msgs.append(str(ei.value))
        eng.close()
    assert msgs[0] == msgs[1]


def test_unserved_modes_refuse_groups():
    game, gid, H, W, A, n = TAGS["othello6"]
    ext = E.SelfPlayEngine(gid, H, W, n_slots=32, n_sim=4, evaluator=E.EVAL_EXTERNAL)
    with pytest.raises(ValueError, match="AZ_EVAL_EXTERNAL"):
        ext.set_groups(2)
    assert ext.groups() == 1
    ext.close()
    gid8, H8, W8, net = get_net("othello")
    sym = E.SelfPlayEngine(gid8, H8, W8, n_slots=8, n_sim=4, net=net)
    sym.set_symmetry("all")
    with pytest.raises(ValueError, match="symmetry"):
        sym.set_groups(2)
    sym.set_symmetry(None)
    with pytest.raises(ValueError, match="less than a block to split"):
        sym.set_groups(2)
    sym.close()
    with pytest.raises(ValueError, match="0 = auto, 1, 2 or 4"):
        fake_engine(32, 3)
    eng = fake_engine(32, 2)
    grids = np.zeros((32, H, W), np.int8)
    from oracle import oracle as O
    b0 = O.new_board(0, 6, 6)
    grids[:] = np.array([b0.grid[i] for i in range(36)], np.int8).reshape(6, 6)
    eng.set_roots(grids, np.ones(32, np.int8))
    eng.search_begin(4)
    with pytest.raises(_lib.AzError, match=r"\[-3\].*az_engine_set_groups"):
        eng.set_groups(1)
    eng.search_end()
    eng.close()
