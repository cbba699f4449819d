#!/usr/bin/env python3
"""fc1 and fc2 of OthelloNet 8x8 on a 2048-row launch beside another chain (az_net_stage_lane, the launch az_net_forward_lane makes
for that stage) over device row counts, under both values of AZ_GEMM_ROWS: 0 = 64 rows per block whatever the count, 1 = the
count-following row forms of k_gemm's 64 x 64 tile.  Back-to-back launches between two HIP events, as
dense_bench.py times a stage; the switch is read once per process, so every leg is a child process, and the legs alternate.
  python tools/count_bench.py [--reps 3] [--launches 400] [counts ...]"""
import ctypes as C
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ROWS = 2048
COUNTS = [1, 64, 256, 512, 513, 1024, 1025, 1536, 2048]


def leg(counts, reps, launches):
    """one process, one value of the switch: {count: {stage: [us per launch, reps times]}} and what the plan says it ran"""
    import torch
    from alphazero_amd import engine as E
    from alphazero_amd.games.othello import OthelloNet
    torch.manual_seed(0)
    hnet = OthelloNet(n=8).eval().to_hip(max_batch=ROWS)
    L = E.lib()
    x = torch.randint(-1, 2, (ROWS, 64), device="cuda").float()
    cnt = torch.tensor([ROWS], dtype=torch.int32, device="cuda")
    pr, va = torch.zeros((ROWS, hnet.A), device="cuda"), torch.zeros(ROWS, device="cuda")
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)
    # the lane's activation rows hold a forward's values: the dense stages read what the stage before them wrote
    E.check(L.az_net_forward_lane(hnet.h, 0, 1, x.data_ptr(), cnt.data_ptr(), ROWS, pr.data_ptr(), va.data_ptr(), sp))
    torch.cuda.synchronize()

    def timed(stage, n):
        for _ in range(20):
            E.check(L.az_net_stage_lane(hnet.h, 0, 1, stage, x.data_ptr(), cnt.data_ptr(), ROWS, pr.data_ptr(), va.data_ptr(), sp))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(st)
        for _ in range(n):
            E.check(L.az_net_stage_lane(hnet.h, 0, 1, stage, x.data_ptr(), cnt.data_ptr(), ROWS, pr.data_ptr(), va.data_ptr(), sp))
        e1.record(st)
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n

    out = {"plan": [hnet.stage_plan(s, ROWS, 1) for s in (1, 2)], "us": {}, "rows": {}}
    for c in counts:
        cnt.fill_(c)
        out["rows"][c] = [hnet.gemm_rows(s, ROWS, 1, c) for s in (1, 2)]
        out["us"][c] = [[round(timed(s, launches), 2) for _ in range(reps)] for s in (1, 2)]
    print("LEG " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    reps, launches = 3, 400
    if "--reps" in args:
        i = args.index("--reps"); reps = int(args[i + 1]); del args[i:i + 2]
    if "--launches" in args:
        i = args.index("--launches"); launches = int(args[i + 1]); del args[i:i + 2]
    if args and args[0] == "--leg":
        return leg([int(a) for a in args[1:]], reps, launches)
    counts = [int(a) for a in args] or COUNTS
    legs = {"0": [], "1": []}
    for rnd in range(2):  # alternated: 0, 1, 0, 1
        for value in ("0", "1"):
            env = dict(os.environ, AZ_GEMM_ROWS=value)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(reps), "--launches", str(launches), "--leg", *map(str, counts)],
                               env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"leg AZ_GEMM_ROWS={value} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            legs[value].append(json.loads(next(l for l in r.stdout.splitlines() if l.startswith("LEG "))[4:]))
    for value in ("0", "1"):
        print(f"AZ_GEMM_ROWS={value}: fc1 {legs[value][0]['plan'][0]} | fc2 {legs[value][0]['plan'][1]}")
    print(f"{ROWS}-row beside launch, us per launch: min (max - min) over {2 * reps} repeats in two processes per leg")
    print(f"{'count':>6} {'rows/block':>10} | {'fc1 rows=64':>16} {'fc1 by count':>16} {'ratio':>6} | {'fc2 rows=64':>16} {'fc2 by count':>16} {'ratio':>6}")
    for c in counts:
        cell = {}
        for value in ("0", "1"):
            for s in (0, 1):
                t = [x for l in legs[value] for x in l["us"][str(c)][s]]
                cell[value, s] = (min(t), max(t) - min(t))
        rows = legs["1"][0]["rows"][str(c)]
        print(f"{c:>6} {rows[0]:>5}/{rows[1]:<4} | " + " | ".join(
            f"{cell['0', s][0]:>9.2f} ({cell['0', s][1]:.2f}) {cell['1', s][0]:>9.2f} ({cell['1', s][1]:.2f}) {cell['1', s][0] / cell['0', s][0]:>6.2f}" for s in (0, 1)), flush=True)


if __name__ == "__main__":
    main()
