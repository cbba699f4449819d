"""k_trunk with its workgroup's four boards sharing the 16-row MFMA tiles of conv3 and conv4 (the QUAD form): those layers read LDS
planes across waves between workgroup barriers, a tile may straddle two boards, and a wave without a board still computes its share.
Every output element keeps its k-ordered chain, so every comparison here is bit equality against the CPU oracle (closed-form
weights, as tests/test_gpu_net.py::nets builds them), 600 boards per oracle call.
The QUAD form is built for the Winograd 8x8 and 7x6 kernels only: 7x6 (connect4) runs it on every k_trunk launch, 8x8 (othello8)
beside another chain, so every case runs both as a plain forward and under the beside flag of az_net_forward_lane.  The othello6
and untuned-plane cases hold the per-board k_trunk, the only form those planes have, to the same bits at the same batch sizes."""
import ast
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import TAGS, golden
from oracle import oracle as O
from tools import closed_form as cf
from alphazero_amd import engine as E

pytestmark = pytest.mark.gpu
N_REF = 600
_CTX = {}


def ctx(tag):
    """per tag, once: the HIP net, 600 canonical boards on the device and the oracle's (probs, v) for them (never modified)"""
    if tag not in _CTX:
        game, gid, H, W, A, n = TAGS[tag]
        fx = golden(f"net_{tag}.npz")
        shapes = {str(k): ast.literal_eval(str(v)) for k, v in zip(fx["shape_keys"], fx["shape_vals"])}
        sd = {k: v for k, v in cf.closed_form_state_dict(shapes).items() if not k.endswith("num_batches_tracked")}
        grids, players, _ = O.random_positions(gid, H, W, 31, 80, 1500)
        assert len(players) >= N_REF
        canon = (grids * players[:, None]).astype(np.float32)[:N_REF]
        op, ov = O.ConvNet(gid, H, W, sd).forward(canon)
        hnet = E.HipNet(gid, H, W, sd, max_batch=2048)
        assert hnet.stage_kernel(0, 513) == "k_trunk" and hnet.stage_kernel(0, 2048) == "k_trunk"
        _CTX[tag] = (hnet, torch.as_tensor(canon, device="cuda"), torch.as_tensor(op, device="cuda"), torch.as_tensor(ov, device="cuda"), A)
    return _CTX[tag]


def fwd(hnet, x, A, beside, count=None):
    """the forward on lane 0, alone (beside = 0: az_net_forward_dyn) or as a launch chain beside another one (beside = 1)"""
    B = x.shape[0]
    c = torch.tensor([B if count is None else count], dtype=torch.int32, device="cuda")
    probs = torch.full((B, A), -7.0, device="cuda")
    v = torch.full((B,), -7.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    E.check(E.lib().az_net_forward_lane(hnet.h, 0, beside, x.data_ptr(), c.data_ptr(), B, probs.data_ptr(), v.data_ptr(), st))
    return probs, v


@pytest.mark.parametrize("tag", ["othello8", "othello6", "connect4"])
def test_ragged_last_workgroup(tag):
    """B = 513 .. 516: the last workgroup holds 1, 2, 3, 4 boards; its waves without a board pass every barrier and compute tiles"""
    hnet, x, op, ov, A = ctx(tag)
    for B in (513, 514, 515, 516):
        p, v = hnet.forward(x[:B].contiguous())
        assert torch.equal(p, op[:B]) and torch.equal(v, ov[:B]), (tag, B)
        p, v = fwd(hnet, x[:B].contiguous(), A, 1)
        assert torch.equal(p, op[:B]) and torch.equal(v, ov[:B]), (tag, B, "beside")


def test_dynamic_row_counts():
    """a launch sized 2048: counts that leave a workgroup 0 .. 4 boards, workgroups wholly behind the count leave before any barrier"""
    hnet, x, op, ov, A = ctx("othello8")
    cap = 2048
    idx = (torch.arange(cap, device="cuda") * 5 + 1) % N_REF
    xx = x[idx].contiguous()
    for count in (0, 1, 2, 3, 4, 5, 7, 513, 1023, 2048, 3000):
        c = torch.tensor([count], dtype=torch.int32, device="cuda")
        probs = torch.full((cap, A), -7.0, device="cuda")
        v = torch.full((cap,), -7.0, device="cuda")
        hnet.forward_dyn(xx, c, probs, v)
        m = min(count, cap)
        assert torch.equal(probs[:m], op[idx[:m]]) and torch.equal(v[:m], ov[idx[:m]]), count
        assert bool((probs[m:] == -7.0).all()) and bool((v[m:] == -7.0).all()), count
        probs, v = fwd(hnet, xx, A, 1, count)
        assert torch.equal(probs[:m], op[idx[:m]]) and torch.equal(v[:m], ov[idx[:m]]), (count, "beside")
        assert bool((probs[m:] == -7.0).all()) and bool((v[m:] == -7.0).all()), (count, "beside")


@pytest.mark.parametrize("tag", ["othello8", "othello6", "connect4"])
def test_row_independence(tag):
    """the same 600 boards in two orders: other workgroup partners, another row offset inside the shared tiles"""
    hnet, x, op, ov, A = ctx(tag)
    perm = torch.as_tensor(np.random.RandomState(3).permutation(N_REF), device="cuda")
    p0, v0 = hnet.forward(x)
    p1, v1 = hnet.forward(x[perm].contiguous())
    assert torch.equal(p0, op) and torch.equal(v0, ov), tag
    assert torch.equal(p1, p0[perm]) and torch.equal(v1, v0[perm]), tag
    p2, v2 = fwd(hnet, x[perm].contiguous(), A, 1)
    assert torch.equal(p2, p0[perm]) and torch.equal(v2, v0[perm]), (tag, "beside")


@pytest.mark.parametrize("H,W", [(7, 7), (6, 8)])
def test_untuned_plane(H, W):
    """the planes plane_tuned leaves out run k_trunk (every board its own tiles) at every size: 7x7 and 8x6 at 5 and 6 boards -- a full
    workgroup and one of 1 and 2 boards"""
    from alphazero_amd.games.connect4 import Connect4Net
    torch.manual_seed(10 * H + W)
    net = Connect4Net(W, H).eval()
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    hnet = E.HipNet(1, H, W, sd, max_batch=64)
    assert hnet.stage_kernel(0, 5) == "k_trunk"
    grids, players, _ = O.random_positions(O.CONNECT4, H, W, 21 + H + W, 40, 64)
    canon = (grids * players[:, None]).astype(np.float32)[:6]
    assert len(canon) == 6
    op, ov = O.ConvNet(O.CONNECT4, H, W, sd).forward(canon)
    for B in (5, 6):
        p, v = hnet.forward(torch.as_tensor(canon[:B], device="cuda"))
        assert np.array_equal(p.cpu().numpy(), op[:B]) and np.array_equal(v.cpu().numpy(), ov[:B]), (H, W, B)
        p, v = fwd(hnet, torch.as_tensor(canon[:B], device="cuda"), hnet.A, 1)
        assert np.array_equal(p.cpu().numpy(), op[:B]) and np.array_equal(v.cpu().numpy(), ov[:B]), (H, W, B, "beside")
    hnet.close()


def test_beside_lane():
    """lane 1 under beside = 1 (the forward of a slot group next to another chain) at count 515 of a 1024-row launch: lane 0's bits"""
    hnet, x, op, ov, A = ctx("othello8")
    L = E.lib()
    E.check(L.az_net_set_lanes(hnet.h, 2, 1024))
    idx = (torch.arange(1024, device="cuda") * 7 + 2) % N_REF
    xx = x[idx].contiguous()
    c = torch.tensor([515], dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []
    for lane, beside in ((0, 0), (1, 1)):
        probs = torch.full((1024, A), -7.0, device="cuda")
        v = torch.full((1024,), -7.0, device="cuda")
        E.check(L.az_net_forward_lane(hnet.h, lane, beside, xx.data_ptr(), c.data_ptr(), 1024, probs.data_ptr(), v.data_ptr(), st))
        out.append((probs, v))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0][:515], op[idx[:515]]) and torch.equal(out[0][1][:515], ov[idx[:515]])
    assert torch.equal(out[1][0], out[0][0]) and torch.equal(out[1][1], out[0][1])
    assert bool((out[1][0][515:] == -7.0).all()) and bool((out[1][1][515:] == -7.0).all())


@pytest.mark.parametrize("tag,beside", [("othello8", 1), ("connect4", 0)])
def test_race_screen(tag, beside):
    """the layers share LDS planes across waves: twenty runs of one 516-board forward give identical bits"""
    hnet, x, op, ov, A = ctx(tag)
    xx = x[:516].contiguous()
    for _ in range(20):
        p, v = fwd(hnet, xx, A, beside)
        assert torch.equal(p, op[:516]) and torch.equal(v, ov[:516])
