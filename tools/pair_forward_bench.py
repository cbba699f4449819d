#!/usr/bin/env python3
"""Lone trunk stage times (az_net_time_stage at 600 / 1024 / 2048 / 4095 boards, three repeats) and the time of two whole forwards side
by side: two lanes on two streams under the beside flag of az_net_forward_lane, 2048-row launches with a device count of 1885 (the
headline's two slot groups without the engine).  AZ_TRUNK_QUAD=0 / 1 forces k_trunk / k_trunk_quad on the 8x8 and 7x6 planes.
  python tools/pair_forward_bench.py othello8|othello6|connect4|c4_7x7|c4_6x8"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from alphazero_amd import engine as E
from alphazero_amd.games.connect4 import Connect4Net
from alphazero_amd.games.othello import OthelloNet
tag = sys.argv[1]
torch.manual_seed(0)
nets = {"othello8": lambda: OthelloNet(n=8), "othello6": lambda: OthelloNet(n=6), "connect4": lambda: Connect4Net(7, 6),
        "c4_7x7": lambda: Connect4Net(7, 7), "c4_6x8": lambda: Connect4Net(8, 6)}
net = nets[tag]().eval()
hnet = net.to_hip(max_batch=4096)
L = E.lib()
lone = []
for rep in range(3):
    lone.append([round(1e3 * hnet.time_stage(0, B, 200), 2) for B in (600, 1024, 2048, 4095)])
E.check(L.az_net_set_lanes(hnet.h, 2, 2048))
P = hnet.H * hnet.W
x = [torch.randint(-1, 2, (2048, P), device="cuda").float() for _ in range(2)]
cnt = torch.tensor([1885], dtype=torch.int32, device="cuda")
pr = [torch.zeros((2048, hnet.A), device="cuda") for _ in range(2)]
va = [torch.zeros(2048, device="cuda") for _ in range(2)]
ss = [torch.cuda.Stream(), torch.cuda.Stream()]
def pair(n):
    for _ in range(n):
        for l in (0, 1):
            E.check(L.az_net_forward_lane(hnet.h, l, 1, x[l].data_ptr(), cnt.data_ptr(), 2048, pr[l].data_ptr(), va[l].data_ptr(), C.c_void_p(ss[l].cuda_stream)))
torch.cuda.synchronize(); pair(50); torch.cuda.synchronize()
pairs = []
for rep in range(3):
    t0 = time.perf_counter(); pair(400); torch.cuda.synchronize()
    pairs.append(round(1e6 * (time.perf_counter() - t0) / 400, 2))
print(tag, "AZ_TRUNK_QUAD=" + os.environ.get("AZ_TRUNK_QUAD", "-"), "lone trunk us at 600/1024/2048/4095 x3:", lone, "pair of 2048-row forwards (count 1885) us x3:", pairs, "kernel", hnet.stage_kernel(0, 2048),
      "k_trunk_quad prefetching form (AZ_TRUNK_QUAD_PREFETCH=" + os.environ.get("AZ_TRUNK_QUAD_PREFETCH", "-") + "): lone", hnet.trunk_prefetch(2048, 0), "pair", hnet.trunk_prefetch(2048, 1),
      "its vector stores (AZ_TRUNK_QUAD_STORES=" + os.environ.get("AZ_TRUNK_QUAD_STORES", "-") + "): lone", hnet.trunk_stores(2048, 0), "pair", hnet.trunk_stores(2048, 1))
