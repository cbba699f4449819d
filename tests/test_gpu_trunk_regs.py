"""k_trunk_quad with the Winograd conv2 in four passes of one frequency row: carries between the passes, patch
offsets and store addresses formed per pass, 124 .. 134 registers so that three or four waves -- another chain's among them -- share a
SIMD.  7x6 runs it on every k_trunk launch (form 1), 8x8 beside another chain (form 2; beside = 1 is az_net_forward_lane's flag: what
a slot group sets).  The forms keep every output element's chain operation for operation, so every comparison here is bit equality
against the CPU oracle, O.ConvNet(...).forward: torch random-init weights under a seed no other test uses and the closed-form
weights, Othello 8x8 and Connect4 7x6, 600 boards per oracle call and larger batches built from them by index.  The last test holds
fc2's 64 x 64 k_gemm tile beside another chain to the same bits at its first and its headline row count."""
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
SEED = 1923
SENT = -7.0
_CTX = {}
NAMES = ["othello8-random", "othello8-closed", "connect4-random", "connect4-closed"]


def ctx(name):
    """per (tag, weights), once: HipNet, state dict's oracle net, 600 canonical boards on the device, the oracle's (probs, v), A"""
    if name not in _CTX:
        tag, kind = name.split("-")
        game, gid, H, W, A, n = TAGS[tag]
        if kind == "random":
            from alphazero_amd.games.connect4 import Connect4Net
            from alphazero_amd.games.othello import OthelloNet
            torch.manual_seed(SEED + H)
            net = (OthelloNet(n=8) if tag == "othello8" else Connect4Net(W, H)).eval()
            sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
        else:
            fx = golden(f"net_{tag}.npz")
            shapes = {str(k): ast.literal_eval(str(v)) for k, v in zip(fx["shape_keys"], fx["shape_vals"])}
            sd = {k: v for k, v in cf.closed_form_state_dict(shapes).items() if not k.endswith("num_batches_tracked")}
        grids, players, _ = O.random_positions(gid, H, W, 47, 80, 1500)
        assert len(players) >= N_REF
        canon = (grids * players[:, None]).astype(np.float32)[:N_REF]
        onet = O.ConvNet(gid, H, W, sd)
        op, ov = onet.forward(canon)
        hnet = E.HipNet(gid, H, W, sd, max_batch=2048)
        assert hnet.stage_kernel(0, 513) == "k_trunk" and hnet.stage_kernel(0, 2048) == "k_trunk"
        _CTX[name] = (hnet, onet, torch.as_tensor(canon, device="cuda"), torch.as_tensor(op, device="cuda"), torch.as_tensor(ov, device="cuda"), A)
    return _CTX[name]


def outputs(rows, A):
    return torch.full((rows, A), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda")


def launch(hnet, lane, beside, x, count, probs, v, stream=None):
    st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    E.check(E.lib().az_net_forward_lane(hnet.h, lane, beside, x.data_ptr(), count.data_ptr(), x.shape[0], probs.data_ptr(), v.data_ptr(), st))


def fwd(hnet, x, A, beside, count=None):
    B = x.shape[0]
    c = torch.tensor([B if count is None else count], dtype=torch.int32, device="cuda")
    got = outputs(B, A)
    launch(hnet, 0, beside, x, c, *got)
    return got


def modes(name):
    """8x8 takes the QUAD form beside another chain only; 7x6 on every k_trunk launch"""
    return (1,) if name.startswith("othello8") else (1, 0)


@pytest.mark.parametrize("name", NAMES)
def test_ragged_last_workgroup(name):
    """B = 513 .. 516: the last workgroup holds 1 .. 4 boards, under weights without the closed form's structure as well"""
    hnet, onet, x, op, ov, A = ctx(name)
    for B in (513, 514, 515, 516):
        for beside in modes(name):
            p, v = fwd(hnet, x[:B].contiguous(), A, beside)
            assert torch.equal(p, op[:B]) and torch.equal(v, ov[:B]), (name, B, beside)


def extreme_boards(H, W):
    """the boards that load the Winograd border tiles (patches half outside the plane) and the carries between the passes (sums of
    equal and of alternating terms): empty, all +1, all -1, checkerboard, one stone in each corner and on each edge centre"""
    P = H * W
    bs = [np.zeros(P), np.ones(P), -np.ones(P), np.array([1.0 if (i // W + i % W) % 2 == 0 else -1.0 for i in range(P)])]
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):
        b = np.zeros(P)
        b[y * W + x] = 1.0
        bs.append(b)
    return np.stack(bs).astype(np.float32)


@pytest.mark.parametrize("name", NAMES)
def test_extreme_boards(name):
    hnet, onet, x, op, ov, A = ctx(name)
    game, gid, H, W, _, n = TAGS[name.split("-")[0]]
    boards = extreme_boards(H, W)
    ep, ev = onet.forward(boards)
    idx = torch.arange(516, device="cuda") % len(boards)
    xx = torch.as_tensor(boards, device="cuda")[idx].contiguous()
    ep, ev = torch.as_tensor(ep, device="cuda")[idx], torch.as_tensor(ev, device="cuda")[idx]
    for beside in modes(name):
        p, v = fwd(hnet, xx, A, beside)
        assert torch.equal(p, ep) and torch.equal(v, ev), (name, beside)


@pytest.mark.parametrize("name", NAMES)
def test_device_counts(name):
    """a 1024-row launch whose rows are a device counter: no workgroup, one board, a full workgroup, one board into the next, a ragged
    count; rows behind the count keep their fill value"""
    hnet, onet, x, op, ov, A = ctx(name)
    idx = (torch.arange(1024, device="cuda") * 5 + 2) % N_REF
    xx = x[idx].contiguous()
    for count in (0, 1, 4, 5, 515):
        for beside in modes(name):
            p, v = fwd(hnet, xx, A, beside, count)
            assert torch.equal(p[:count], op[idx[:count]]) and torch.equal(v[:count], ov[idx[:count]]), (name, count, beside)
            assert bool((p[count:] == SENT).all()) and bool((v[count:] == SENT).all()), (name, count, beside, "rows behind the count")


@pytest.mark.parametrize("name", ["othello8-random", "othello8-closed"])
def test_two_forwards_in_flight(name):
    """one az_net on lanes 0 and 1 at 2048 rows each, beside = 1 -- the smallest size at which both chains' waves can share SIMDs (512
    trunk workgroups per launch on 256 CUs) --, ten rounds issued without a synchronisation: every round of either lane holds the
    oracle's bits"""
    hnet, onet, x, op, ov, A = ctx(name)
    E.check(E.lib().az_net_set_lanes(hnet.h, 2, 2048))
    streams = [torch.cuda.current_stream(), torch.cuda.Stream(priority=-1)]
    idx = [(torch.arange(2048, device="cuda") * s + o) % N_REF for s, o in ((7, 3), (11, 34))]
    xs = [x[i].contiguous() for i in idx]
    c = torch.tensor([2048], dtype=torch.int32, device="cuda")
    outs = [[outputs(2048, A) for lane in range(2)] for _ in range(10)]
    torch.cuda.synchronize()
    for r in range(10):
        for lane in range(2):
            launch(hnet, lane, 1, xs[lane], c, *outs[r][lane], stream=streams[lane])
    torch.cuda.synchronize()
    for r in range(10):
        for lane in range(2):
            p, v = outs[r][lane]
            assert torch.equal(p, op[idx[lane]]) and torch.equal(v, ov[idx[lane]]), (name, "round", r, "lane", lane)


@pytest.mark.parametrize("name", ["othello8-random", "othello8-closed"])
def test_fc2_beside_tile(name):
    """1985 and 2048 rows under beside = 1: fc2 (K = 1024) on k_gemm's 64 x 64 tile, 1985 rows the first size that takes it and a
    ragged last row band, 2048 the headline's launch"""
    hnet, onet, x, op, ov, A = ctx(name)
    for B in (1985, 2048):
        idx = (torch.arange(B, device="cuda") * 13 + 5) % N_REF
        p, v = fwd(hnet, x[idx].contiguous(), A, 1)
        assert torch.equal(p, op[idx]) and torch.equal(v, ov[idx]), (name, B)
