"""GPU: the lanes of one az_net (az_net_set_lanes / az_net_forward_lane) at the sizes a grouped az_engine_run puts on
them.  A slot group forwards on its own lane with beside = 1, and beside changes the kernel picks by the launch's size
(az_net_plan.h: plan_trunk, plan_dense; pinned without a GPU in test_net_plan_host.py).  OthelloNet 8x8, rows B of the launch, lone launch | beside:

  trunk   B <= 512 k_trunk_q | k_trunk_q;  513 .. 4095 k_trunk | k_trunk_quad;  from 4096 k_trunk2 | k_trunk2
  fc1     (K = 512, N = 1024)  B <= 1024 k_dense_frag | k_dense_frag;  1025 .. 3968 k_gemm<64,64> | k_gemm<64,64>;
          3969 .. 4100 k_gemm<128,64> on both sides (32 tile rows x 16 = 512 blocks)
  fc2     (K = 1024, N = 512)  B <= 1024 k_dense_frag | k_dense_frag;  1025 .. 1984 k_dense_frag | k_gemm<64,128>;
          1985 .. 2048 k_dense_frag | k_gemm<64,64> (32 tile rows x 8 = 256 blocks);  2049 .. 4100 k_gemm<64,64> | k_gemm<64,64>
  heads   k_heads2 at every size

othello6 (6x6 plane) has no quad form and runs k_trunk on either side; connect4 (7x6) runs k_trunk_quad on every k_trunk launch and
its fused tail (k_tail_mfma) in place of fc1 / fc2 / heads.  az_net_stage_kernel answers for the lone launch only, so the names above
are the thresholds read, not asserted (a kernel trace of the beside forwards at 1025, 1985 and 4095 rows listed exactly these).
Every kernel of a layer keeps each output element's k-ordered chain, so every comparison here is bit equality with the CPU oracle:
600 boards per network evaluated once, larger batches built from them by index.

One host thread drives the net throughout: az_net_forward_lane's contract (include/az_amd.h) is lanes on different streams issued from
one host thread, and two host threads on one az_net are not tested."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import TAGS
from oracle import oracle as O
from alphazero_amd import engine as E

pytestmark = pytest.mark.gpu
N_REF = 600
MAX_B = 4100
SENT = -7.0
_CTX = {}


def ctx(name):
    """per network, once: (HipNet of max_batch 4100, 600 canonical boards on the device, the oracle's probs and v for them, A).
    "<tag>": the closed-form weights of test_gpu_net.nets; "othello8-random": torch.manual_seed weights of OthelloNet"""
    if name not in _CTX:
        tag = name.split("-")[0]
        game, gid, H, W, A, n = TAGS[tag]
        if name.endswith("-random"):
            from alphazero_amd.games.othello import OthelloNet
            torch.manual_seed(20)
            sd = {k: v.detach().cpu().numpy() for k, v in OthelloNet(n=8).eval().state_dict().items() if not k.endswith("num_batches_tracked")}
            onet = O.ConvNet(gid, H, W, sd)
        else:
            from test_gpu_net import nets
            fx, sd, onet, other = nets(tag)
            other.close()
        grids, players, _ = O.random_positions(gid, H, W, 31, 80, 1500)
        assert len(players) >= N_REF
        canon = (grids * players[:, None]).astype(np.float32)[:N_REF]
        op, ov = onet.forward(canon)
        hnet = E.HipNet(gid, H, W, sd, max_batch=MAX_B)
        _CTX[name] = (hnet, torch.as_tensor(canon, device="cuda"), torch.as_tensor(op, device="cuda"), torch.as_tensor(ov, device="cuda"), A)
    return _CTX[name]


def index_map(rows, lane=0):
    """rows of the 600 reference boards for a batch: another stride and offset per lane"""
    return (torch.arange(rows, device="cuda") * (7, 11, 13, 17)[lane] + 3 + 31 * lane) % N_REF


def outputs(rows, A):
    return torch.full((rows, A), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda")


def launch(hnet, lane, beside, x, count, probs, v, stream=None):
    st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    E.check(E.lib().az_net_forward_lane(hnet.h, lane, beside, x.data_ptr(), count.data_ptr(), x.shape[0], probs.data_ptr(), v.data_ptr(), st))


def expect(got, op, ov, idx, count, what):
    """the oracle's bits on the rows before the count, the sentinel behind it"""
    probs, v = got
    m = min(count, probs.shape[0])
    assert torch.equal(probs[:m], op[idx[:m]]) and torch.equal(v[:m], ov[idx[:m]]), what
    assert bool((probs[m:] == SENT).all()) and bool((v[m:] == SENT).all()), (what, "rows behind the count")


SIZES = (1025, 1040, 1984, 1985, 2047, 2049, 3000, 3968, 3969, 4095, 4096, 4100)
FEW = (1025, 4095, 4096, 4100)


@pytest.mark.parametrize("name,sizes", [("othello8", SIZES), ("othello8-random", SIZES), ("connect4", FEW), ("othello6", FEW)])
def test_beside_picks_over_their_whole_range(name, sizes):
    """lane 0, launch size = row count: 1025 / 1040 leave k_dense_frag for both layers, 1984 | 1985 moves fc2 from the 64x128 to the
    64x64 tile, 2047 .. 3000 cross the lone launch's own fc2 limit, 3968 | 3969 moves fc1 to the 128x64 tile, 4095 | 4096 is
    k_trunk_quad | k_trunk2 under beside (k_trunk | k_trunk2 alone), 4100 a ragged k_trunk2 launch.  The oracle's bits under
    beside = 1 and under beside = 0."""
    hnet, x, op, ov, A = ctx(name)
    for B in sizes:
        idx = index_map(B)
        xx = x[idx].contiguous()
        c = torch.tensor([B], dtype=torch.int32, device="cuda")
        for beside in (1, 0):
            got = outputs(B, A)
            launch(hnet, 0, beside, xx, c, *got)
            expect(got, op, ov, idx, B, (name, B, "beside" if beside else "lone"))


@pytest.mark.parametrize("name", ["othello8", "othello8-random", "connect4", "othello6"])
def test_beside_device_counted_launch(name):
    """a 4095-row launch (the largest k_trunk_quad one, the dense layers on k_gemm<128,64> and k_gemm<64,64>) whose rows are a device
    counter: nothing, a ragged workgroup, a count inside and just past k_dense_frag's range (the picks follow the launch, not the
    count), all rows, and a count beyond the launch"""
    hnet, x, op, ov, A = ctx(name)
    idx = index_map(4095)
    xx = x[idx].contiguous()
    for count in (0, 3, 515, 1025, 4095, 5000):
        c = torch.tensor([count], dtype=torch.int32, device="cuda")
        for beside in (1, 0):
            got = outputs(4095, A)
            launch(hnet, 0, beside, xx, c, *got)
            expect(got, op, ov, idx, count, (name, count, "beside" if beside else "lone"))


ROUNDS = 10


@pytest.mark.parametrize("name,R,counts", [("othello8", 2048, (2048, 1885, 515, 0)), ("othello8", 1056, (1056, 1025, 1024, 7)),
                                           ("connect4", 2048, (2048, 2047, 513, 1)), ("othello6", 1056, (1056, 1025, 1024, 7))])
def test_four_forwards_in_flight(name, R, counts):
    """what four slot groups do to one az_net: lane l on stream l (stream 0 the current one, 1 .. 3 from the priority pool the engine
    takes its later groups' streams from), every lane its own input rows, device count and output buffers, beside = 1.  Ten rounds of
    four launches are issued back to back from this one host thread with no synchronisation anywhere between them (a lane's next
    round follows its last on its own stream); one synchronisation, then every lane of every round holds the oracle's bits on its
    own rows and the sentinel behind its count.  A lane that wrote another lane's activation rows would show here."""
    hnet, x, op, ov, A = ctx(name)
    E.check(E.lib().az_net_set_lanes(hnet.h, 4, R))
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream(priority=-1) for _ in range(3)]
    idx = [index_map(R, lane) for lane in range(4)]
    xs = [x[i].contiguous() for i in idx]
    cs = [torch.tensor([c], dtype=torch.int32, device="cuda") for c in counts]
    outs = [[outputs(R, A) for lane in range(4)] for _ in range(ROUNDS)]
    torch.cuda.synchronize()  # inputs and sentinels are in place before any stream reads them
    for r in range(ROUNDS):
        for lane in range(4):
            launch(hnet, lane, 1, xs[lane], cs[lane], *outs[r][lane], stream=streams[lane])
    torch.cuda.synchronize()
    for r in range(ROUNDS):
        for lane in range(4):
            expect(outs[r][lane], op, ov, idx[lane], counts[lane], (name, R, "round", r, "lane", lane))


def test_beside_reaches_the_launch_and_the_profile_slot():
    """beside travels from az_net_forward_lane to the stage's plan, and the plan's slot to az_net_profile: at 2048 rows a lone forward
    books fc2 under "small fc2" (k_dense_frag), a beside one under "k_gemm fc2" (the 64x64 tile); both book the trunk under "k_trunk"
    (k_trunk | k_trunk_quad) and fc1 under "k_gemm fc1".  Same bits from both, and they are the oracle's."""
    game, gid, H, W, A, n = TAGS["othello8"]
    from test_gpu_net import nets
    fx, sd, onet, other = nets("othello8")
    other.close()
    _, x, op, ov, _ = ctx("othello8")
    hnet = E.HipNet(gid, H, W, sd, max_batch=2048)
    idx = index_map(2048)
    xx = x[idx].contiguous()
    c = torch.tensor([2048], dtype=torch.int32, device="cuda")
    hnet.profile(True)
    lone = hnet.forward(xx)
    counts = {k: v[1] for k, v in hnet.profile_read().items()}
    assert counts == {"k_trunk2": 0, "k_gemm fc1": 1, "k_gemm fc2": 0, "k_heads": 1, "k_trunk": 1, "small fc1": 0, "small fc2": 1, "k_trunk_q": 0}, counts
    beside = outputs(2048, A)
    launch(hnet, 0, 1, xx, c, *beside)
    counts = {k: v[1] for k, v in hnet.profile_read().items()}
    assert counts == {"k_trunk2": 0, "k_gemm fc1": 2, "k_gemm fc2": 1, "k_heads": 2, "k_trunk": 2, "small fc1": 0, "small fc2": 1, "k_trunk_q": 0}, counts
    assert torch.equal(lone[0], beside[0]) and torch.equal(lone[1].reshape(-1), beside[1])
    expect(beside, op, ov, idx, 2048, "beside, profiled")
    hnet.close()


def test_set_lanes_bookkeeping():
    """lanes grow and are replaced by wider ones, never shrink or go away; what az_net_forward_lane and az_net_set_lanes refuse is
    AZ_EINVAL with its message and touches no output buffer"""
    game, gid, H, W, A, n = TAGS["othello6"]
    from test_gpu_net import nets
    fx, sd, onet, other = nets("othello6")
    other.close()
    _, x, op, ov, _ = ctx("othello6")
    hnet = E.HipNet(gid, H, W, sd, max_batch=1300)
    L = E.lib()

    def run(lane, rows):
        idx = index_map(rows, lane)
        got = outputs(rows, A)
        launch(hnet, lane, 1, x[idx].contiguous(), torch.tensor([rows], dtype=torch.int32, device="cuda"), *got)
        return got, idx

    def refused(lane, rows, message):
        got = outputs(rows, A)
        with pytest.raises(ValueError, match=message):
            launch(hnet, lane, 1, x[index_map(rows)].contiguous(), torch.tensor([rows], dtype=torch.int32, device="cuda"), *got)
        torch.cuda.synchronize()
        assert bool((got[0] == SENT).all()) and bool((got[1] == SENT).all()), message

    refused(1, 16, r"lane 1 of 1 \(az_net_set_lanes\)")  # a fresh net has lane 0 only
    E.check(L.az_net_set_lanes(hnet.h, 2, 600))
    got, idx = run(1, 600)
    expect(got, op, ov, idx, 600, "lane 1 of 2 at 600 rows")
    refused(2, 16, r"lane 2 of 2 \(az_net_set_lanes\)")
    refused(1, 601, r"batch 601 beyond the 600 rows of lane 1")
    E.check(L.az_net_set_lanes(hnet.h, 4, 1200))  # wider rows: lane 1 is replaced, lanes 2 and 3 are new
    for lane in (1, 2, 3):
        got, idx = run(lane, 1200)
        expect(got, op, ov, idx, 1200, ("lane", lane, "of 4 at 1200 rows"))
    E.check(L.az_net_set_lanes(hnet.h, 2, 100))  # fewer and narrower: nothing is given back
    got, idx = run(3, 1200)
    expect(got, op, ov, idx, 1200, "lane 3 at 1200 rows after set_lanes(2, 100)")
    refused(4, 16, r"lane 4 of 4 \(az_net_set_lanes\)")
    refused(1, 1201, r"batch 1201 beyond the 1200 rows of lane 1")
    with pytest.raises(ValueError, match=r"az_net_set_lanes: 5 lanes outside \[1, 4\]"):
        E.check(L.az_net_set_lanes(hnet.h, 5, 100))
    with pytest.raises(ValueError, match=r"az_net_set_lanes: 1301 rows outside \(0, max_batch=1300\]"):
        E.check(L.az_net_set_lanes(hnet.h, 2, 1301))
    got, idx = run(3, 1200)  # the refused calls changed nothing
    expect(got, op, ov, idx, 1200, "lane 3 after the refused calls")
    hnet.close()


def test_tictactoe_lanes_are_names():
    """k_mlp keeps no activation in memory, so a lane of the TicTacToe MLP has no rows: after az_net_set_lanes(2, 64) a lane-1
    forward gives lane 0's bits, which are the oracle's, and a lane that was never named is still refused"""
    from test_gpu_net import nets
    game, gid, H, W, A, n = TAGS["tictactoe"]
    fx, sd, onet, other = nets("tictactoe")
    other.close()
    hnet = E.HipNet(gid, H, W, sd, max_batch=64)
    grids, players, _ = O.random_positions(gid, H, W, 31, 40, 64)
    canon = (grids * players[:, None]).astype(np.float32)
    B = len(canon)
    assert B >= 40
    op, ov = onet.forward(canon)
    op, ov = torch.as_tensor(op, device="cuda"), torch.as_tensor(ov, device="cuda")
    x = torch.as_tensor(canon, device="cuda")
    c = torch.tensor([B - 3], dtype=torch.int32, device="cuda")
    idx = torch.arange(B, device="cuda")
    got = outputs(B, A)
    with pytest.raises(ValueError, match=r"lane 1 of 1 \(az_net_set_lanes\)"):
        launch(hnet, 1, 1, x, c, *got)
    E.check(E.lib().az_net_set_lanes(hnet.h, 2, 64))
    for lane in (0, 1):
        got = outputs(B, A)
        launch(hnet, lane, 1, x, c, *got)
        expect(got, op, ov, idx, B - 3, ("tictactoe lane", lane))
    got = outputs(B, A)
    with pytest.raises(ValueError, match=r"lane 2 of 2 \(az_net_set_lanes\)"):
        launch(hnet, 2, 1, x, c, *got)
    torch.cuda.synchronize()
    assert bool((got[0] == SENT).all()) and bool((got[1] == SENT).all())
    hnet.close()
