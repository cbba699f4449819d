"""k_trunk_quad's prefetching form: the board's input, conv1's weights and conv2's first U k-steps requested before
the wave knows the row count, the U ring run through conv2's pass boundaries, conv3 / conv4's weights read from the per-half order
TrunkParams::wh, which both fold paths fill.  OthelloNet 8x8 beside another chain (beside = 1 is
az_net_forward_lane's flag: what a slot group sets) takes the form by default.  No output element's chain changes, so every comparison
here is bit equality against the CPU oracle, O.ConvNet(...).forward: torch random-init weights under a seed no other test uses and
the closed-form weights, 600 boards per oracle call and larger batches built from them by index."""
import ast
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import TAGS, golden
from oracle import oracle as O
from tools import closed_form as cf
from alphazero_amd import engine as E

pytestmark = pytest.mark.gpu
N_REF = 600
SEED = 2924
SENT = -7.0
_CTX = {}
NAMES = ["random", "closed"]
GID, H, W, A = TAGS["othello8"][1], 8, 8, 65


def state_dict(kind, seed=SEED):
    if kind == "random":
        from alphazero_amd.games.othello import OthelloNet
        torch.manual_seed(seed)
        net = OthelloNet(n=8).eval()
        # running statistics and affine terms away from BatchNorm's initial 0 / 1, so that a fold that skipped one would show
        with torch.no_grad():
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
        want = os.environ.get("AZ_TRUNK_QUAD_PREFETCH") in (None, "1")  # the default rule; the file also runs under the switch's 0
        assert hnet.trunk_prefetch(513, 1) == hnet.trunk_prefetch(2048, 1) == want and not hnet.trunk_prefetch(2048, 0)
        _CTX[kind] = (hnet, torch.as_tensor(boards(), device="cuda"), *oracle_of(sd))
    return _CTX[kind]


def outputs(rows):
    return torch.full((rows, A), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda")


def launch(hnet, lane, x, count, probs, v, stream=None):
    st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    E.check(E.lib().az_net_forward_lane(hnet.h, lane, 1, x.data_ptr(), count.data_ptr(), x.shape[0], probs.data_ptr(), v.data_ptr(), st))


def fwd(hnet, x, count=None):
    B = x.shape[0]
    c = torch.tensor([B if count is None else count], dtype=torch.int32, device="cuda")
    got = outputs(B)
    launch(hnet, 0, x, c, *got)
    return got


@pytest.mark.parametrize("kind", NAMES)
def test_ragged_last_workgroup(kind):
    """B = 513 .. 516, the smallest launches the plan gives to k_trunk_quad: the last workgroup holds 1 .. 4 boards, and its waves
    without a board request no input (the tensor ends with row B - 1)"""
    hnet, x, op, ov = ctx(kind)
    for B in (513, 514, 515, 516):
        p, v = fwd(hnet, x[:B].clone())
        assert torch.equal(p, op[:B]) and torch.equal(v, ov[:B]), (kind, B)


@pytest.mark.parametrize("kind", NAMES)
def test_speculative_loads(kind):
    """a 1024-row launch whose row count is a device counter: the input rows at and beyond the count, which the waves request before
    they know the count, hold NaN and +-Inf.  Rows below the count equal the oracle, rows at and beyond it keep the output sentinel"""
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
    """the per-half weight order is filled by the host fold (az_net_commit: a HipNet built from numpy weights) and by k_fold
    (az_net_commit_device: CUDA tensors): each equals the oracle at 516 rows, and after a second weight set has been loaded into the
    same net each equals THAT set's oracle -- a per-half buffer left from the first set would show"""
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
    rounds issued on two streams without a synchronisation: every round of either lane holds the oracle's bits"""
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
            launch(hnet, lane, xs[lane], c, *outs[r][lane], stream=streams[lane])
    torch.cuda.synchronize()
    for r in range(10):
        for lane in range(2):
            p, v = outs[r][lane]
            assert torch.equal(p, op[idx[lane]]) and torch.equal(v, ov[idx[lane]]), (kind, "round", r, "lane", lane)
