#!/usr/bin/env python3
"""Which matrix kernels of the forward share the chip, and which only take turns: every ordered pair (X, Y) of {trunk, fc1, fc2} of
OthelloNet 8x8 at 2048 rows with a device count of 1885 (a slot group of the headline), X on lane 0 and Y on lane 1, on two streams of
the two priority pools, under the beside flag -- az_net_stage_lane, the launch az_net_forward_lane makes for that stage.  Per pair: the
lone time of either stage (the other stream idle), then nX launches of X beside nY launches of Y, the counts chosen so that both
streams run equally long alone, and the wall time of that against nX tX + nY tY.  1.00 = the two take turns; 0.50 = they overlap
completely.  The switches (AZ_TRUNK_QUAD_STORES, AZ_TRUNK_QUAD_PREFETCH, AZ_GEMM_FORM, ...) pick the forms; the plan's answers are printed.
  python tools/beside_pairs.py [rows [count]]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from alphazero_amd import engine as E
from alphazero_amd.games.othello import OthelloNet

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
COUNT = int(sys.argv[2]) if len(sys.argv) > 2 else 1885
NAMES = ["trunk", "fc1", "fc2"]
torch.manual_seed(0)
hnet = OthelloNet(n=8).eval().to_hip(max_batch=ROWS)
L = E.lib()
E.check(L.az_net_set_lanes(hnet.h, 2, ROWS))
x = [torch.randint(-1, 2, (ROWS, 64), device="cuda").float() for _ in range(2)]
cnt = torch.tensor([COUNT], dtype=torch.int32, device="cuda")
pr = [torch.zeros((ROWS, hnet.A), device="cuda") for _ in range(2)]
va = [torch.zeros(ROWS, device="cuda") for _ in range(2)]
ss = [torch.cuda.Stream(), torch.cuda.Stream(priority=-1)]
for lane in (0, 1):  # every lane's activation rows hold a forward's values: the dense stages read what the stage before them wrote
    E.check(L.az_net_forward_lane(hnet.h, lane, 1, x[lane].data_ptr(), cnt.data_ptr(), ROWS, pr[lane].data_ptr(), va[lane].data_ptr(), C.c_void_p(ss[lane].cuda_stream)))
torch.cuda.synchronize()


def enqueue(lane, stage, n):
    for _ in range(n):
        E.check(L.az_net_stage_lane(hnet.h, lane, 1, stage, x[lane].data_ptr(), cnt.data_ptr(), ROWS, pr[lane].data_ptr(), va[lane].data_ptr(), C.c_void_p(ss[lane].cuda_stream)))


def lone(lane, stage, n=400):
    """us per launch of n back-to-back launches on the lane's stream, the other stream idle"""
    enqueue(lane, stage, 20)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(ss[lane]); enqueue(lane, stage, n); e1.record(ss[lane])
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def pair(sx, nx, sy, ny):
    """us from the first launch to the end of both streams: nx launches of sx on lane 0 beside ny of sy on lane 1, issued interleaved"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    gate = torch.cuda.current_stream()
    torch.cuda.synchronize()
    ev[0].record(gate)
    for s in ss:
        s.wait_event(ev[0])
    done = [0, 0]
    for i in range(max(nx, ny)):  # interleaved in proportion, so that neither stream waits for the host
        for lane, stage, n in ((0, sx, nx), (1, sy, ny)):
            want = (i + 1) * n // max(nx, ny)
            enqueue(lane, stage, want - done[lane])
            done[lane] = want
    ev[1].record(ss[0]); ev[2].record(ss[1])
    torch.cuda.synchronize()
    return 1e3 * max(ev[0].elapsed_time(ev[1]), ev[0].elapsed_time(ev[2]))


print(f"beside_pairs othello8 rows {ROWS} count {COUNT}  plan beside: " + " | ".join(f"{NAMES[s]} {hnet.stage_plan(s, ROWS, 1)}" for s in range(3)) + "  switches "
      + " ".join(f"{k}={v}" for k, v in sorted(os.environ.items()) if k.startswith("AZ_")), flush=True)
t_lone = [[min(lone(lane, st) for _ in range(2)) for st in range(3)] for lane in (0, 1)]
print("lone us, lane 0 / lane 1: " + "  ".join(f"{NAMES[s]} {t_lone[0][s]:.2f} / {t_lone[1][s]:.2f}" for s in range(3)), flush=True)
print(f"{'X (lane 0)':>10} {'Y (lane 1)':>10} {'nX':>5} {'nY':>5} {'pair us':>10} {'sum lone us':>12} {'pair / sum':>10}   three repeats")
for sx in range(3):
    for sy in range(3):
        tx, ty = t_lone[0][sx], t_lone[1][sy]
        nx, ny = (400, max(1, round(400 * tx / ty))) if tx >= ty else (max(1, round(400 * ty / tx)), 400)
        pair(sx, nx // 8, sy, ny // 8)
        got = [pair(sx, nx, sy, ny) for _ in range(3)]
        total = nx * tx + ny * ty
        print(f"{NAMES[sx]:>10} {NAMES[sy]:>10} {nx:>5} {ny:>5} {min(got):>10.1f} {total:>12.1f} {min(got) / total:>10.3f}   " + " ".join(f"{g / total:.3f}" for g in got), flush=True)
