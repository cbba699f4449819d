"""k_gemm's ring form: the 64 x 64 tile with a ring of three K tiles in LDS, the next-but-one tile written inside
the k-steps and the fragment ring carried across the tile boundary.  By the rule OthelloNet 8x8's beside launches (beside = 1 is
az_net_forward_lane's flag: what a slot group sets) of at most one block per CU take it: fc2 at 1985 .. 2048 rows.  Every other 64 x 64
launch -- fc1, lone launches, the other nets -- takes it under AZ_GEMM_FORM=1 only.  The chain is the double-buffer form's -- bias, then k ascending on v_mfma_f32_32x32x2_f32 --, so every
comparison is bit equality of pi and v with the CPU oracle, O.ConvNet(...).forward: torch random-init weights under a seed no other
test uses, 600 boards per oracle call and larger batches built from them by index.  Every case runs under beside = 1 and beside = 0;
the last test runs the file's other cases again in a child process per value of AZ_GEMM_FORM (the library reads it once per process):
0, the double-buffer form everywhere, and 1, the ring form on every 64 x 64 launch -- fc1 and the lone launches included.  The
children also set AZ_NO_FUSED_TAIL=1, under which Connect4Net 6x7 runs fc1 (K = 192) as a dense stage of its own.
What these tests cannot see is WHICH form ran: az_net_stage_kernel names the family, k_gemm, for both, and the two forms give the
same bits by design, so a launch that fell back to the double buffer would pass here.  That the ring runs where the plan says rests
on tests/test_net_plan_gemm_form.py (the plan's gemm_form per launch), on launch_dense's one-line dispatch on that field, and on the
tracer's k_gemm_ring row in profiles/r23_gemm_form.txt."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from oracle import oracle as O
from alphazero_amd import engine as E

pytestmark = pytest.mark.gpu
N_REF = 600
SEED = 2317
SENT = -7.0
_CTX = {}
NETS = {"othello8": (0, 8, 8, 65), "othello6": (0, 6, 6, 37), "connect4": (1, 6, 7, 7), "connect4_5x6": (1, 5, 6, 6)}  # oracle game id, H, W, action size


def ctx(tag):
    """per net, once: HipNet, 600 canonical boards on the device, the oracle's (probs, v), A"""
    if tag not in _CTX:
        import numpy as np
        from alphazero_amd.games.connect4 import Connect4Net
        from alphazero_amd.games.othello import OthelloNet
        gid, H, W, A = NETS[tag]
        torch.manual_seed(SEED + H)
        net = (OthelloNet(n=H) if gid == 0 else Connect4Net(W, H)).eval()
        sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
        grids, players, _ = O.random_positions(gid, H, W, 53, 80, 1500)
        assert len(players) >= N_REF
        canon = (grids * players[:, None]).astype(np.float32)[:N_REF]
        op, ov = O.ConvNet(gid, H, W, sd).forward(canon)
        hnet = E.HipNet(gid, H, W, sd, max_batch=2048)
        assert hnet.stage_kernel(1, 1025) == ("k_tail_mfma" if tag == "connect4" and "AZ_NO_FUSED_TAIL" not in os.environ else "k_gemm")
        _CTX[tag] = (hnet, torch.as_tensor(canon, device="cuda"), torch.as_tensor(op, device="cuda"), torch.as_tensor(ov, device="cuda"), A)
    return _CTX[tag]


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


@pytest.mark.parametrize("beside", [1, 0])
@pytest.mark.parametrize("tag,B", [("othello8", 1025), ("othello8", 1985), ("othello8", 2048), ("othello6", 1025), ("connect4_5x6", 321), ("connect4", 321)])
def test_rows(tag, B, beside):
    """othello8, 1025 rows: fc1's first size on the tile, 17 row bands, the last holding one row.  1985: the first size that takes the
    64 x 64 tile for fc2 beside another chain, a ragged last band; 2048: a full last band.  othello6, 1025 rows: fc1 has K = 128, four K
    tiles of 32 k.  connect4_5x6, 321 rows: fc1 has K = 64, the shortest ring -- four tiles of 16 k, all staged by the prologue, which
    meets the drain with no steady state between; six row bands, the last holding one row (othello8's 32 and 64 tiles of 16 k, 16 and 8
    here: none a multiple of the ring's three buffers, the register sets' four divide them all).  connect4 (6x7), 321 rows: the fused
    tail in this process; in test_forced_form's children fc1 with K = 192, twelve tiles of 16 k, the one tile count that is a multiple
    of both the three buffers and the four register sets."""
    hnet, x, op, ov, A = ctx(tag)
    idx = (torch.arange(B, device="cuda") * 13 + 5) % N_REF
    p, v = fwd(hnet, x[idx].contiguous(), A, beside)
    assert torch.equal(p, op[idx]) and torch.equal(v, ov[idx]), (tag, B, beside)


@pytest.mark.parametrize("beside", [1, 0])
def test_device_counts(beside):
    """a 2048-row launch whose rows are a device counter: no work, one row, a full row band, one row into the next, the headline's
    count; rows behind the count keep their fill value"""
    hnet, x, op, ov, A = ctx("othello8")
    idx = (torch.arange(2048, device="cuda") * 5 + 2) % N_REF
    xx = x[idx].contiguous()
    for count in (0, 1, 64, 65, 1885):
        p, v = fwd(hnet, xx, A, beside, count)
        assert torch.equal(p[:count], op[idx[:count]]) and torch.equal(v[:count], ov[idx[:count]]), (count, beside)
        assert bool((p[count:] == SENT).all()) and bool((v[count:] == SENT).all()), (count, beside, "rows behind the count")


def test_two_forwards_in_flight():
    """one az_net on lanes 0 and 1 at 2048 rows each on two streams, beside = 1, ten rounds issued without a synchronisation: every round
    of either lane holds the oracle's bits (a ring slot read or refilled too early would show here, with the other chain's waves
    stretching the skew between a workgroup's four waves)"""
    hnet, x, op, ov, A = ctx("othello8")
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
            assert torch.equal(p, op[idx[lane]]) and torch.equal(v, ov[idx[lane]]), ("round", r, "lane", lane)


@pytest.mark.parametrize("form", ["0", "1"])
def test_forced_form(form):
    """the cases above in a child process under AZ_GEMM_FORM: 0 = the double-buffer form still holds the same bits on every launch;
    1 = the ring form on every 64 x 64 launch, the lone ones (beside = 0) included.  AZ_NO_FUSED_TAIL=1 in both: Connect4Net 6x7's
    fc1 as a k_gemm launch"""
    if "AZ_GEMM_FORM_CHILD" in os.environ:
        return
    env = dict(os.environ, AZ_GEMM_FORM=form, AZ_NO_FUSED_TAIL="1", AZ_GEMM_FORM_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
