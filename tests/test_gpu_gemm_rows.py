"""The count-following row forms of k_gemm's 64 x 64 tile (StagePlan::gemm_rows, gemm_rows_per_block): a block of
fc1 (k_gemm) / fc2 (k_gemm_ring) takes 16 or 32 rows where the launch's row bands still cover the device row count, on 16x16x4 chains,
and 64 rows above that, the path as it was.  OthelloNet 8x8 beside another chain (beside = 1 is az_net_forward_lane's flag: what a slot
group sets) takes them by default.  No output element's chain changes -- bias, then k ascending -- so every comparison is bit equality
against the CPU oracle, O.ConvNet(...).forward: the closed-form weights and torch random-init weights (a seed no other test uses)
whose BatchNorm statistics are moved, 600 boards per oracle call and larger batches built from them by index.  The last test runs the
file's other cases again in a child process per value of AZ_GEMM_ROWS (read once per process): 0 and 1."""
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
SEED = 3429
SENT = -7.0
_CTX = {}
NAMES = ["random", "closed"]
GID, H, W, A = TAGS["othello8"][1], 8, 8, 65
FOLLOW = os.environ.get("AZ_GEMM_ROWS") != "0"  # unset: the rule, which a beside launch of OthelloNet 8x8 meets; 1: everywhere
COUNTS_2048 = (0, 1, 15, 16, 17, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)


def rows_of(bands, count):
    """gemm_rows_per_block, restated: the narrowest of 16 / 32 / 64 rows per block whose `bands` blocks cover the count"""
    if not FOLLOW:
        return 64
    return 16 if -(-count // 16) <= bands else 32 if -(-count // 32) <= bands else 64


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
        grids, players, _ = O.random_positions(GID, H, W, 59, 80, 1500)
        assert len(players) >= N_REF
        _CTX["boards"] = (grids * players[:, None]).astype(np.float32)[:N_REF]
    return _CTX["boards"]


def ctx(kind):
    """per weight set, once: HipNet, 600 canonical boards on the device, the oracle's (probs, v); and what the plan says it runs"""
    if kind not in _CTX:
        sd = state_dict(kind)
        hnet = E.HipNet(GID, H, W, sd, max_batch=2048)
        op, ov = O.ConvNet(GID, H, W, sd).forward(boards())
        # fc1 and fc2 of a 2048-row beside launch both run the 64 x 64 tile (32 bands); a lone launch follows the count under the switch only
        for stage in (1, 2):
            assert "k_gemm 64x64" in hnet.stage_plan(stage, 2048, 1) and ("rows=count" if FOLLOW else "rows=64") in hnet.stage_plan(stage, 2048, 1)
            for count in COUNTS_2048:
                assert hnet.gemm_rows(stage, 2048, 1, count) == rows_of(32, count), (stage, count)
        assert hnet.gemm_rows(1, 2048, 1, 5000) == 64 and hnet.gemm_rows(0, 2048, 1, 1) == 0 and hnet.gemm_rows(1, 256, 1, 1) == 0
        if os.environ.get("AZ_GEMM_ROWS") is None:
            assert hnet.gemm_rows(2, 4096, 0, 1) == 64
        _CTX[kind] = (hnet, torch.as_tensor(boards(), device="cuda"), torch.as_tensor(op, device="cuda"), torch.as_tensor(ov, device="cuda"))
    return _CTX[kind]


def outputs(rows):
    return torch.full((rows, A), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda")


def poisoned(x, idx, count):
    """the launch's input rows: boards idx below the count, NaN and +-Inf at and beyond it"""
    B = len(idx)
    junk = torch.tensor([float("nan"), float("inf"), float("-inf")], device="cuda")
    xx = x[idx].contiguous()
    xx[count:] = junk[(torch.arange(B - count, device="cuda")[:, None] + torch.arange(64, device="cuda")[None, :]) % 3]
    return xx


def check_counts(kind, B, counts):
    """a B-row launch per device count: rows below the count equal the oracle, rows at and beyond it keep the output sentinel"""
    hnet, x, op, ov = ctx(kind)
    idx = (torch.arange(B, device="cuda") * 5 + 2) % N_REF
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for count in counts:
        xx = poisoned(x, idx, count)
        c = torch.tensor([count], dtype=torch.int32, device="cuda")
        p, v = outputs(B)
        E.check(E.lib().az_net_forward_lane(hnet.h, 0, 1, xx.data_ptr(), c.data_ptr(), B, p.data_ptr(), v.data_ptr(), st))
        assert torch.equal(p[:count], op[idx[:count]]) and torch.equal(v[:count], ov[idx[:count]]), (kind, B, count)
        assert bool((p[count:] == SENT).all()) and bool((v[count:] == SENT).all()), (kind, B, count, "rows at and beyond the count")


@pytest.mark.parametrize("kind", NAMES)
def test_counts_of_a_2048_row_launch(kind):
    """the headline's group launch, 32 row bands: 16-row blocks up to 512 rows, 32-row blocks up to 1024, 64-row blocks above, and
    each form's last block full, one row short and holding a single row"""
    check_counts(kind, 2048, COUNTS_2048)


@pytest.mark.parametrize("kind", NAMES)
@pytest.mark.parametrize("B", [1025, 1985])
def test_counts_around_the_thresholds_of_other_launches(kind, B):
    """1025 rows: 17 bands, fc1 on the 64 x 64 tile (the first size beside), fc2 on the 64 x 128 tile, which has no narrow form;
    1985 rows: 32 bands, the first size at which fc2 runs the 64 x 64 tile, in its ring form.  Counts around 16 and 32 times the bands,
    as the plan function gives them, with the launch's ends"""
    hnet = ctx(kind)[0]
    bands = (B + 63) // 64
    assert bands == {1025: 17, 1985: 32}[B]
    counts = [0, 1]
    for r in (16, 32):
        t = r * bands
        assert rows_of(bands, t) == (r if FOLLOW else 64) and rows_of(bands, t + 1) == ((2 * r) if FOLLOW else 64)
        counts += [t - 1, t, t + 1]
    counts += [B - 1, B]
    for count in counts:
        assert hnet.gemm_rows(1, B, 1, count) == rows_of(bands, count), (B, count)
        assert hnet.gemm_rows(2, B, 1, count) == (rows_of(bands, count) if B == 1985 else 64), (B, count)
    assert ("64x64 form=1" in hnet.stage_plan(2, B, 1)) == (B == 1985) and "64x64 form=0" in hnet.stage_plan(1, B, 1)
    check_counts(kind, B, counts)


@pytest.mark.parametrize("kind", NAMES)
def test_two_forwards_in_flight(kind):
    """one az_net on lanes 0 and 1 at 2048 rows each -- the headline's two groups --, ten rounds issued on two streams without a
    synchronisation, the lanes' counts different in every round and across the three forms: every round of either lane equals the
    oracle below its count and keeps the sentinel beyond"""
    hnet, x, op, ov = ctx(kind)
    E.check(E.lib().az_net_set_lanes(hnet.h, 2, 2048))
    streams = [torch.cuda.current_stream(), torch.cuda.Stream(priority=-1)]
    idx = [(torch.arange(2048, device="cuda") * s + o) % N_REF for s, o in ((7, 3), (11, 34))]
    counts = [[1, 16, 300, 512, 513, 777, 1024, 1025, 2048, 40], [2048, 1500, 33, 1000, 17, 2047, 0, 600, 511, 1030]]
    xs = [[poisoned(x, idx[lane], counts[lane][r]) for r in range(10)] for lane in range(2)]
    cs = [[torch.tensor([counts[lane][r]], dtype=torch.int32, device="cuda") for r in range(10)] for lane in range(2)]
    outs = [[outputs(2048) for lane in range(2)] for _ in range(10)]
    torch.cuda.synchronize()
    for r in range(10):
        for lane in range(2):
            p, v = outs[r][lane]
            E.check(E.lib().az_net_forward_lane(hnet.h, lane, 1, xs[lane][r].data_ptr(), cs[lane][r].data_ptr(), 2048, p.data_ptr(), v.data_ptr(),
                                                C.c_void_p(streams[lane].cuda_stream)))
    torch.cuda.synchronize()
    for r in range(10):
        for lane in range(2):
            (p, v), n = outs[r][lane], counts[lane][r]
            assert torch.equal(p[:n], op[idx[lane][:n]]) and torch.equal(v[:n], ov[idx[lane][:n]]), (kind, "round", r, "lane", lane)
            assert bool((p[n:] == SENT).all()) and bool((v[n:] == SENT).all()), (kind, "round", r, "lane", lane, "rows beyond the count")


@pytest.mark.parametrize("value", ["0", "1"])
def test_forced_switch(value):
    """the cases above in a child process under AZ_GEMM_ROWS: 0 = 64 rows per block everywhere, 1 = the narrow forms wherever they exist"""
    if "AZ_GEMM_ROWS_CHILD" in os.environ:
        return
    env = dict(os.environ, AZ_GEMM_ROWS=value, AZ_GEMM_ROWS_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
