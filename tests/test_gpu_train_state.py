"""The hand-written training step (csrc/az_train.hip) depends on NOTHING but its inputs: parameters, momenta, running statistics, the
hyper-parameter block and the batch.  Every other test of the step starts from a fresh trainer whose workspace is zeros and hands it
whole torch allocations; here the same two steps (lr 0.1, momentum 0.9, weight decay 1e-4, dropout 0.3, Philox seed 3: the second
step reads what the first stored, the masks take part) are repeated while everything that must not matter is changed:
  a. a second trainer, and the first one again after load() + begin(): the same bits, workspace included;
  b. every workspace buffer (az_trainer_buffer lists ALL allocations by class) filled with NaN bytes / with 1e30 before each step;
  c. the batch size changed on a live trainer (512 -> 144 -> 32 -> 144) against fresh trainers of exactly that size;
  d. three trainers of three networks stepping in turn in one process;
  e. the caller's arrays -- samples, permutation, loss slots, the tensors load() reads and store() writes -- carved out of guard
     bands of 0xFF / zero bytes, at aligned and at odd element offsets; the bands come back untouched;
  f. the network's forward (HipNet.forward, forward_dyn) between such bands.
Every comparison is bit equality (check_train_step.same_bits compares bytes): no tolerance, no float64 model, no seed exceptions.
Cases: the smallest batch that reaches each dispatch of enqueue_step (check_train_step.STATE_CASES)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_train_step as C  # noqa: E402
from alphazero_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

CONV_CASES = [c for c in C.STATE_CASES if c[0] != "tictactoe"]
_PROBLEMS, _SOLO = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """the cached problems and reference runs go with the module: the tests that follow find the device memory as they would without this file"""
    yield
    _PROBLEMS.clear()
    _SOLO.clear()
    torch.cuda.empty_cache()


def problem(tag, B):
    if (tag, B) not in _PROBLEMS:
        _PROBLEMS[tag, B] = C.StateProblem(tag, B)
    return _PROBLEMS[tag, B]


def solo(tag, B, calls=C.TWO_CALLS):
    """the reference of every test: the run on a fresh trainer, computed once and left unchanged"""
    if (tag, B, calls) not in _SOLO:
        hip = problem(tag, B).trainer()
        _SOLO[tag, B, calls] = C.state_run(hip, problem(tag, B), calls, workspace=True)
        hip.close()
        r = _SOLO[tag, B, calls]
        assert C.all_finite(r) and all((r[f"call{k}.loss_pi"] > 0).all() for k in range(len(calls))), (tag, B)
        assert int(r["sd.bn1.num_batches_tracked"]) == sum(n for _, n in calls)
    return _SOLO[tag, B, calls]


def without_workspace(res):
    return {k: v for k, v in res.items() if not k.startswith("ws.")}


# ---------------------------------------------------------------------------------------------------------------- the listing itself
@pytest.mark.parametrize("tag,B", [("connect4", 144), ("othello8", 144), ("tictactoe", 64)])
def test_every_allocation_is_listed_with_a_class(tag, B):
    """az_trainer_buffer walks every allocation of az_trainer_create: the parameters and statistics add up to the module's own, every
    parameter has a momentum buffer of its size, debug()'s names are workspace names with the listing's sizes, and TicTacToeNet's
    single-kernel step has no workspace at all"""
    prob = problem(tag, B)
    hip = prob.trainer()
    bufs = hip.buffers()
    names = [b[0] for b in bufs]
    assert len(set(names)) == len(names) and {b[1] for b in bufs} <= set(_lib.TRAINER_BUFFER_CLASSES)
    assert len({b[2] for b in bufs}) == len(bufs) and all(b[3] > 0 for b in bufs)
    by = {c: {n: nb for n, cl, p, nb in bufs if cl == c} for c in _lib.TRAINER_BUFFER_CLASSES}
    assert {n[2:]: nb for n, nb in by["parameter"].items()} == {n[2:]: nb for n, nb in by["momentum"].items()}
    assert list(by["hyper"].values()) == [48]  # sizeof(Hyper)
    n_par, n_stat = sum(p.numel() for p in prob.net.parameters()), sum(b.numel() for b in prob.net.buffers() if b.dtype == torch.float32)
    assert sum(by["running_stat"].values()) == 4 * n_stat
    if tag == "tictactoe":
        assert by["workspace"] == {} and list(hip.views("workspace")) == []
        assert sum(by["parameter"].values()) == 4 * 320 and n_par == 316  # k_ttt_step's padded block
    else:
        gid, H, W = prob.net.hip_shape()
        pad = ((prob.net.action_size + 1 + 15) // 16 * 16 - prob.net.action_size - 1) * (prob.net.fc2.out_features + 1)  # the heads' zero rows
        assert sum(by["parameter"].values()) == 4 * (n_par + pad)
        assert len(by["workspace"]) > 0
        for name, shape in (("c1", B * H * W * 32), ("dy4", B * (H - 4) * (W - 4) * 32), ("h1", B * prob.net.fc1.out_features), ("losspart", B // 16 * 2)):
            assert by["workspace"][name] == 4 * shape and hip.debug(name).numel() == shape
        with pytest.raises(ValueError, match="unknown workspace buffer"):
            hip.debug("p.w1")
        views = dict(hip.views("workspace"))
        assert sorted(views) == sorted(by["workspace"]) and all(v.dtype == torch.uint8 and v.numel() == by["workspace"][k] for k, v in views.items())
        views["fdone1"].fill_(7)  # a view is the trainer's memory, not a copy
        assert bool((hip.debug("fdone1").view(torch.uint8) == 7).all())
    hip.close()


# ---------------------------------------------------------------------------------------------------------------- a. twice is the same
@pytest.mark.parametrize("tag,B", C.STATE_CASES)
def test_twice_is_the_same(tag, B):
    """a fresh trainer, a second fresh trainer, and the second one again after load() + begin() (its workspace, graphs and step counter
    are those the first pass left): the same losses, state dict and workspace bytes"""
    prob, first = problem(tag, B), solo(tag, B)
    hip = prob.trainer()
    second = C.state_run(hip, prob, workspace=True)
    third = C.state_run(hip, prob, workspace=True)
    hip.close()
    C.same_bits(first, second, (tag, B, "second trainer"))
    C.same_bits(first, third, (tag, B, "the same trainer after load() + begin()"))


# ---------------------------------------------------------------------------------------------------------------- b. poisoned workspace
@pytest.mark.parametrize("kind", ["nan", "1e30"])
@pytest.mark.parametrize("tag,B", CONV_CASES)
def test_a_step_writes_its_workspace_before_it_reads_it(tag, B, kind):
    """every workspace-class buffer filled after begin() and again between the two steps: losses and state dict keep the clean run's
    bits and stay finite.  No buffer of the workspace class carries anything from step to step (were one to, it would be a class
    of its own that begin() resets)."""
    prob = problem(tag, B)
    hip = prob.trainer()
    n_workspace = sum(cls == "workspace" for _, cls, _, _ in hip.buffers())
    filled = []
    got = C.state_run(hip, prob, before_call=lambda k: filled.append(C.poison_workspace(hip, kind)))
    assert n_workspace > 0 and filled == [n_workspace, n_workspace]  # every listed workspace buffer, before either step
    with pytest.raises(_lib.AzError):
        hip.close() or hip.buffers()  # a closed trainer has no listing: an error, not an empty one
    assert C.all_finite(got), (tag, B, kind, [k for k, v in got.items() if v.dtype.kind == "f" and not np.isfinite(v).all()][:8])
    C.same_bits(without_workspace(solo(tag, B)), got, (tag, B, kind))


# ---------------------------------------------------------------------------------------------------------------- c. another batch size
@pytest.mark.parametrize("new_pointers", [False, True])
@pytest.mark.parametrize("tag", ["connect4", "othello6"])
def test_another_batch_size_on_a_live_trainer(tag, new_pointers):
    """one trainer of max_batch 512: two steps at 512, begin() and two at 144, then WITHOUT begin() two at 32 and two at 144 again, each
    leg one az_trainer_steps call.  With the same sample / permutation / loss pointers throughout only the batch size tells the cached
    graphs apart.  Before each leg a fresh trainer with that batch as its max_batch takes over parameters, momenta, running statistics
    and Hyper (check_train_step.copy_state) and runs the same call: same losses, same state dict."""
    prob = problem(tag, 512)
    live = prob.trainer(512)
    live.load(prob.net)
    keep = []
    for leg, (B, begin) in enumerate(((512, True), (144, True), (32, False), (144, False))):
        arrays = {k: v.clone() for k, v in prob.arrays.items()} if new_pointers else prob.arrays
        keep.append(arrays)  # alive: a clone must not get the address of the leg before
        if begin:
            live.begin(*C.STATE_HYPER, C.state_dropout(tag), seed=3)
        fresh = prob.trainer(B)
        C.copy_state(live, fresh)
        a = C.state_run(live, prob, ((0, 2),), B=B, arrays=arrays, load=False, begin=False)
        b = C.state_run(fresh, prob, ((0, 2),), B=B, arrays=arrays, load=False, begin=False)
        fresh.close()
        assert C.all_finite(a) and int(a["sd.bn1.num_batches_tracked"]) == (2 if begin else 2 * leg)
        C.same_bits(b, a, (tag, "leg", leg, "batch", B, "new pointers" if new_pointers else "same pointers"))
    live.close()


# ---------------------------------------------------------------------------------------------------------------- d. two trainers at once
def test_three_trainers_stepping_in_turn():
    """Connect4Net at 512, OthelloNet 8x8 at 64 and TicTacToeNet at 64 alive together, their calls interleaved X, Y, T, X, Y, T, X, Y, T
    (the third call repeats the second one's pointers: a replay of the cached graph).  Kernel attributes and the AZ_TRAIN_* caches are
    process-wide, graphs per trainer: each trainer's result is its solo run's."""
    calls = ((0, 1), (1, 1), (1, 1))
    cases = [("connect4", 512), ("othello8", 64), ("tictactoe", 64)]
    alone = [solo(tag, B, calls) for tag, B in cases]
    for (tag, B), r in zip(cases, alone):  # the first two calls of the three are the two of (a)
        if (tag, B) in C.STATE_CASES:
            two = solo(tag, B)
            assert all(r[k].tobytes() == two[k].tobytes() for k in two if k.startswith(("call0.", "call1.")))
    probs = [problem(tag, B) for tag, B in cases]
    hips = [p.trainer() for p in probs]
    res = [C.state_begin(h, p) for h, p in zip(hips, probs)]
    for k, call in enumerate(calls):
        for h, p, r in zip(hips, probs, res):
            C.state_call(h, p, r, k, call)
    for (tag, B), h, p, r, want in zip(cases, hips, probs, res, alone):
        C.same_bits(want, C.state_end(h, p, r, workspace=True), (tag, B, "interleaved"))
    for h in hips:
        h.close()


# ---------------------------------------------------------------------------------------------------------------- e. guard bands
@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("fill", [0xFF, 0x00])
@pytest.mark.parametrize("tag,B", [("connect4", 144), ("othello6", 48), ("tictactoe", 2)])
def test_the_step_stays_inside_the_callers_arrays(tag, B, fill, odd):
    """state, pi, z, perm, loss_pi, loss_v and every tensor load() reads or store() writes are contiguous views with at least B rows of
    band bytes on either side (0xFF: NaN floats, -1 boards and permutation entries; or zeros), starting at the band's end or one element
    further; the permutation takes row 0 and the last row.  The result is (a)'s, and every band byte is what was written there."""
    prob = problem(tag, B)
    perm = prob.arrays["perm"].cpu()
    assert 0 in perm and prob.arrays["state"].shape[0] - 1 in perm
    bands = C.Banded(B, fill, odd)
    arrays = {k: bands.carve(v) for k, v in prob.arrays.items()}
    source, target = bands.module(prob.net), bands.module(prob.net)
    for v in target.state_dict().values():
        if v.dtype == torch.float32:
            v.fill_(float("nan"))  # store() has to write every element
    assert all((v.data_ptr() // v.element_size()) % 2 == int(odd) for v in arrays.values())
    hip = prob.trainer()
    got = C.state_run(hip, prob, arrays=arrays, load=source, out=target)
    hip.close()
    C.same_bits(without_workspace(solo(tag, B)), got, (tag, B, hex(fill), "odd offset" if odd else "aligned"))
    assert bands.check() >= 2 * len(bands.items) * B
    for k, v in prob.net.state_dict().items():  # load() only read
        assert torch.equal(v, source.state_dict()[k]), k


# ---------------------------------------------------------------------------------------------------------------- f. the network's forward
@pytest.mark.parametrize("tag,rows", [("connect4", 1), ("connect4", 65), ("connect4", 600), ("othello6", 1), ("othello6", 65)])
def test_the_forward_stays_inside_the_callers_arrays(tag, rows):
    """HipNet.forward and forward_dyn with the input a view between 0xFF bands (NaN floats) and the outputs views between sentinel
    bands: the plain call's bits, the bands untouched"""
    import ctypes
    from alphazero_amd import engine as E
    net = C.make_net(tag).cuda().eval()
    gid, H, W = net.hip_shape()
    hip = E.HipNet(gid, H, W, net.state_dict(), max_batch=640)
    x = torch.randint(-1, 2, (rows, H * W), generator=torch.Generator().manual_seed(rows)).float().cuda()
    probs, v = hip.forward(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(probs).all()) and bool(torch.isfinite(v).all())
    count = torch.tensor([rows], dtype=torch.int32, device="cuda")
    for dyn in (False, True):
        bands = C.Banded(rows, 0xFF, False)
        xb, pb, vb = bands.carve(x), bands.empty(probs.shape, torch.float32), bands.empty(v.shape, torch.float32)
        if dyn:
            hip.forward_dyn(xb, count, pb, vb)
        else:
            _lib.check(_lib.lib().az_net_forward(hip.h, xb.data_ptr(), rows, pb.data_ptr(), vb.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        assert pb.cpu().numpy().tobytes() == probs.cpu().numpy().tobytes() and vb.cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), (tag, rows, dyn)
        assert torch.equal(xb, x) and bands.check() >= 6 * rows
    hip.close()
