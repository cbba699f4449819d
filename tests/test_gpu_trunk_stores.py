"""k_trunk_quad's prefetching form with vector stores (StagePlan::quad_stores): conv3's planes written under one
predicate per accumulator as paired LDS writes, conv4's features stored as one 16-byte vector per accumulator.  OthelloNet 8x8 beside
another chain (beside = 1 is az_net_forward_lane's flag: what a slot group sets) takes it by default wherever it takes the
prefetching form.  No output element's chain changes, so every comparison is bit equality against the CPU oracle,
O.ConvNet(...).forward: the closed-form weights and torch random-init weights (a seed no other test uses) whose BatchNorm statistics
are moved, 600 boards per oracle call and larger batches built from them by index.  The last test runs the file's other cases again
in a child process per value of AZ_TRUNK_QUAD_STORES (read once per process): 0 and 1."""
import ast
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, TAGS, golden
from oracle import oracle as O
from tools import closed_form as cf
from alphazero_amd import engine as E

pytestmark = pytest.mark.gpu
N_REF = 600
SEED = 3125
SENT = -7.0
_CTX = {}
NAMES = ["random", "closed"]
GID, H, W, A = TAGS["othello8"][1], 8, 8, 65


def state_dict(kind, seed=SEED):
    if kind == "random":
        from alphazero_amd.games.othello import OthelloNet
        torch.manual_seed(seed)
        net = OthelloNet(n=8).eval()
        with torch.no_grad():  # running statistics away from BatchNorm's initial 0 / 1
            for name, buf in net.state_dict().items():
                if name.endswith("running_mean"):
                    buf.copy_(0.1 * torch.randn_like(buf))
                elif name.endswith("running_var"):
                    buf.copy_(0.5 + torch.rand_like(buf))
        return {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    fx = golden("net_othello8.npz")
    shapes = {str(k): ast.literal_eval(str(v)) for k, v in zip(fx["shape_keys"], fx["shape_vals"])}
    return {k: v for k, v in cf.closed_form_state_dict(shapes).items() if not k.endswith("num_batches_tracked")}


def boards():
    if "boards" not in _CTX:
        grids, players, _ = O.random_positions(GID, H, W, 53, 80, 1500)
        assert len(players) >= N_REF
        _CTX["boards"] = (grids * players[:, None]).astype(np.float32)[:N_REF]
    return _CTX["boards"]


def oracle_of(sd):
    op, ov = O.ConvNet(GID, H, W, sd).forward(boards())
    return torch.as_tensor(op, device="cuda"), torch.as_tensor(ov, device="cuda")


def ctx(kind):
    """per weight set, once: HipNet (host fold), 600 canonical boards on the device, the oracle's (probs, v)"""
    if kind not in _CTX:
        sd = state_dict(kind)
        hnet = E.HipNet(GID, H, W, sd, max_batch=2048)
        # the rule: with the prefetching form; the switch: 0 nowhere, 1 wherever the prefetching form runs
        want = hnet.trunk_prefetch(2048, 1) and os.environ.get("AZ_TRUNK_QUAD_STORES") in (None, "1")
        assert hnet.trunk_stores(513, 1) == hnet.trunk_stores(1024, 1) == hnet.trunk_stores(2048, 1) == want
        assert not hnet.trunk_stores(2048, 0) and not hnet.trunk_stores(512, 1)
        _CTX[kind] = (hnet, torch.as_tensor(boards(), device="cuda"), *oracle_of(sd))
    return _CTX[kind]


def outputs(rows):
    return torch.full((rows, A), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda")


def fwd(hnet, x, count=None):
    B = x.shape[0]
    c = torch.tensor([B if count is None else count], dtype=torch.int32, device="cuda")
    p, v = outputs(B)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    E.check(E.lib().az_net_forward_lane(hnet.h, 0, 1, x.data_ptr(), c.data_ptr(), B, p.data_ptr(), v.data_ptr(), st))
    return p, v


@pytest.mark.parametrize("kind", NAMES)
def test_ragged_last_workgroup(kind):
    """B = 513 .. 516, the smallest launches the plan gives to k_trunk_quad: the last workgroup holds 1 .. 4 boards, so its shared row
    tiles end after 36, 72, 108 and 144 rows of conv3 and 16 .. 64 of conv4 -- the vector stores' bound at every number of boards"""
    hnet, x, op, ov = ctx(kind)
    for B in (513, 514, 515, 516):
        p, v = fwd(hnet, x[:B].clone())
        assert torch.equal(p, op[:B]) and torch.equal(v, ov[:B]), (kind, B)


@pytest.mark.parametrize("kind", NAMES)
def test_counts_and_poisoned_rows(kind):
    """a 1024-row launch whose row count is a device counter, with NaN and +-Inf in the input rows at and beyond the count, which the
    waves request before they know the count: workgroups of fewer than four boards store only their boards' vectors.
    Rows below the count equal the oracle, rows at and beyond it keep the output sentinel"""
    hnet, x, op, ov = ctx(kind)
    idx = (torch.arange(1024, device="cuda") * 5 + 2) % N_REF
    junk = torch.tensor([float("nan"), float("inf"), float("-inf")], device="cuda")
    for count in (0, 1, 4, 5, 515, 1023):
        xx = x[idx].contiguous()
        xx[count:] = junk[(torch.arange(1024 - count, device="cuda")[:, None] + torch.arange(64, device="cuda")[None, :]) % 3]
        p, v = fwd(hnet, xx, count)
        assert torch.equal(p[:count], op[idx[:count]]) and torch.equal(v[:count], ov[idx[:count]]), (kind, count)
        assert bool((p[count:] == SENT).all()) and bool((v[count:] == SENT).all()), (kind, count, "rows at and beyond the count")


def test_both_fold_paths():
    """weights folded on the host (a HipNet built from numpy weights) and by k_fold (CUDA tensors): each equals the oracle at 516 rows,
    and after a second weight set has been loaded into the same net each equals THAT set's oracle"""
    sds = [state_dict("random", SEED + 1), state_dict("random", SEED + 2)]
    refs = [oracle_of(sd) for sd in sds]
    x = torch.as_tensor(boards(), device="cuda")[:516].contiguous()
    as_host = lambda sd: sd
    as_device = lambda sd: {k: torch.as_tensor(v, device="cuda") for k, v in sd.items()}
    for conv in (as_host, as_device):
        hnet = E.HipNet(GID, H, W, conv(sds[0]), max_batch=516)
        for which in (0, 1):
            if which:
                hnet.load_state_dict(conv(sds[1]))
            p, v = fwd(hnet, x)
            assert torch.equal(p, refs[which][0][:516]) and torch.equal(v, refs[which][1][:516]), (conv is as_device, which)


@pytest.mark.parametrize("kind", NAMES)
def test_two_forwards_in_flight(kind):
    """one az_net on lanes 0 and 1 at 2048 rows each -- the headline's two groups: 512 trunk workgroups per launch on 256 CUs --, ten
    rounds issued on two streams without a synchronisation: every round of either lane equals the first, and the first the oracle
    (conv3's paired writes land in planes the other waves of the workgroup read behind the next barrier)"""
    hnet, x, op, ov = ctx(kind)
    E.check(E.lib().az_net_set_lanes(hnet.h, 2, 2048))
    streams = [torch.cuda.current_stream(), torch.cuda.Stream(priority=-1)]
    idx = [(torch.arange(2048, device="cuda") * s + o) % N_REF for s, o in ((7, 3), (11, 34))]
    xs = [x[i].contiguous() for i in idx]
    c = torch.tensor([2048], dtype=torch.int32, device="cuda")
    outs = [[outputs(2048) for lane in range(2)] for _ in range(10)]
    torch.cuda.synchronize()
    for r in range(10):
        for lane in range(2):
            p, v = outs[r][lane]
            E.check(E.lib().az_net_forward_lane(hnet.h, lane, 1, xs[lane].data_ptr(), c.data_ptr(), 2048, p.data_ptr(), v.data_ptr(),
                                                C.c_void_p(streams[lane].cuda_stream)))
    torch.cuda.synchronize()
    for lane in range(2):
        p0, v0 = outs[0][lane]
        assert torch.equal(p0, op[idx[lane]]) and torch.equal(v0, ov[idx[lane]]), (kind, "lane", lane)
        for r in range(1, 10):
            assert torch.equal(outs[r][lane][0], p0) and torch.equal(outs[r][lane][1], v0), (kind, "round", r, "lane", lane)


@pytest.mark.parametrize("value", ["0", "1"])
def test_forced_switch(value):
    """the cases above in a child process under AZ_TRUNK_QUAD_STORES: 0 = the prefetching form as it was, 1 = its vector stores"""
    if "AZ_TRUNK_QUAD_STORES_CHILD" in os.environ:
        return
    env = dict(os.environ, AZ_TRUNK_QUAD_STORES=value, AZ_TRUNK_QUAD_STORES_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
