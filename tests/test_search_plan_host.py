"""CPU: the launch sequence the engine plans for a search (alphazero_amd/csrc/az_search_plan.h: plan_search, plan_step), pinned without
a GPU.  tests/search_plan_table.cpp is compiled with the host C++ compiler and run as a child process.  What is pinned: the kernel
family per mode and its precedence, every launch's template pair and arguments, the forwards between them, the lock-steps a search
counts, the batch caps, the slot groups' ranges and measured rule, and that the graph keys keep different searches apart."""
import os
import shutil
import subprocess

import pytest

from alphazero_amd import gumbel as G
from conftest import ROOT

CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
ROOT_PASS = ["kernel k_root_prep", "forward ctr=2 step=-1 kt=0", "kernel k_root_init"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("search_plan") / "search_plan_table")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero_amd", "csrc"),
                           os.path.join(ROOT, "tests", "search_plan_table.cpp"), "-o", out])
    return out


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.splitlines()


def plan(exe, n_sim, rollout=0, gm=0, K=1, full=0, cap=0, forced=0):
    """the plan line's fields and the launch lines that follow it"""
    head, *seq = run(exe, "plan", rollout, gm, K, full, cap, forced, n_sim)
    word, family, *fields = head.split()
    assert word == "plan"
    return family, {k: int(v) for k, v in (f.split("=") for f in fields)}, seq


def lockstep_shape(kernel, args):
    """k_step's launch sequence at n_sim = 3 with `kernel`; args(t): the arguments of launch t"""
    return ROOT_PASS + [f"step {kernel}<0,1> {args(0)}", "forward ctr=0 step=0 kt=0", f"step {kernel}<1,1> {args(1)}", "forward ctr=1 step=1 kt=0",
                        f"step {kernel}<1,1> {args(2)}", "forward ctr=0 step=2 kt=0", f"step {kernel}<1,0> {args(3)}"]


@pytest.mark.parametrize("mode,kernel", [({}, "k_step"), ({"cap": 1}, "k_step_cap"), ({"forced": 1}, "k_step_forced"),
                                         ({"cap": 1, "forced": 1}, "k_step_cap_forced")])
def test_one_leaf_families(exe, mode, kernel):
    family, f, seq = plan(exe, 3, **mode)
    assert family == kernel and f == {"full": 0, "root_pass": 1, "L": 3, "launches": 4}
    assert seq == lockstep_shape(kernel, lambda t: f"{t} g0 g1")


def test_gumbel_has_k_steps_shape_and_n_sim_as_the_extra_argument(exe):
    for full in (0, 1):  # `full` changes the flag and nothing else
        family, f, seq = plan(exe, 3, gm=4, full=full)
        assert family == "k_step_gumbel" and f == {"full": full, "root_pass": 1, "L": 3, "launches": 4}
        assert seq == lockstep_shape("k_step_gumbel", lambda t: f"{t} 3 g0 g1")
    assert plan(exe, 3, full=1)[2] == plan(exe, 3)[2]


def test_precedence(exe):
    # rollout, then Gumbel with K > 1, then K > 1, then Gumbel, then forced (with or without the cap), then the cap, then plain
    assert plan(exe, 8, rollout=1, gm=4, K=4, cap=1, forced=1)[0] == "k_rollout_step"
    assert plan(exe, 8, gm=4, K=4, cap=1, forced=1)[0] == "k_step_gumbel_multi"
    assert plan(exe, 8, K=4, cap=1, forced=1)[0] == "k_step_multi"
    assert plan(exe, 8, gm=4, cap=1, forced=1)[0] == "k_step_gumbel"  # the setters never allow the combination
    assert plan(exe, 8, gm=4, cap=1)[0] == plan(exe, 8, gm=4, forced=1)[0] == "k_step_gumbel"
    assert plan(exe, 8, cap=1, forced=1)[0] == "k_step_cap_forced"
    assert plan(exe, 8, forced=1)[0] == "k_step_forced"
    assert plan(exe, 8, cap=1)[0] == "k_step_cap"
    assert plan(exe, 8)[0] == "k_step"


def steps_and_forwards(seq):
    assert seq[:3] == ROOT_PASS
    return [l for l in seq[3:] if l.startswith("step ")], [l for l in seq[3:] if l.startswith("forward ")]


def test_multi(exe):
    family, f, seq = plan(exe, 10, K=4)
    assert family == "k_step_multi" and f == {"full": 0, "root_pass": 1, "L": 3, "launches": 4}
    assert seq == ROOT_PASS + ["step k_step_multi<0,1> 0 0 4", "forward ctr=0 step=0 kt=4", "step k_step_multi<1,1> 1 4 4", "forward ctr=1 step=1 kt=4",
                               "step k_step_multi<1,1> 2 4 2", "forward ctr=0 step=2 kt=2", "step k_step_multi<1,0> 3 2 0"]
    _, f, seq = plan(exe, 8, K=4)
    assert f["L"] == 2 and f["launches"] == 3
    assert steps_and_forwards(seq) == (["step k_step_multi<0,1> 0 0 4", "step k_step_multi<1,1> 1 4 4", "step k_step_multi<1,0> 2 4 0"],
                                       ["forward ctr=0 step=0 kt=4", "forward ctr=1 step=1 kt=4"])
    _, f, seq = plan(exe, 1, K=16)
    assert f["L"] == 1 and f["launches"] == 2
    assert steps_and_forwards(seq) == (["step k_step_multi<0,1> 0 0 1", "step k_step_multi<1,0> 1 1 0"], ["forward ctr=0 step=0 kt=1"])


@pytest.mark.parametrize("n,m,K", [(16, 16, 16), (16, 4, 4), (7, 4, 4), (100, 16, 8), (50, 16, 16), (8, 4, 2)])
def test_gumbel_multi(exe, n, m, K):
    L = G.locksteps(n, m, K)
    assert run(exe, "locksteps", n, m, K) == [str(L)]
    for full in (0, 1):
        family, f, seq = plan(exe, n, gm=m, K=K, full=full)
        assert family == "k_step_gumbel_multi" and f == {"full": full, "root_pass": 1, "L": L, "launches": L + 1}
        steps, forwards = steps_and_forwards(seq)
        pair = lambda t: "<0,1>" if t == 0 else ("<1,1>" if t < L else "<1,0>")
        assert steps == [f"step k_step_gumbel_multi{pair(t)} {t} {n}" for t in range(L + 1)]
        assert forwards == [f"forward ctr={t & 1} step={t} kt={K}" for t in range(L)]
        assert seq[-1] == f"step k_step_gumbel_multi<1,0> {L} {n}"  # the last launch: a backup, no forward behind it


def test_rollout(exe):
    for n in (1, 3, 8):
        family, f, seq = plan(exe, n, rollout=1)
        assert family == "k_rollout_step" and f == {"full": 0, "root_pass": 0, "L": 0, "launches": n}
        assert seq == [f"step k_rollout_step {s}" for s in range(n)]  # no root pass, no forward


def test_no_launch_without_backup_and_select(exe):
    for mode in ({}, {"cap": 1}, {"forced": 1}, {"cap": 1, "forced": 1}, {"gm": 4}, {"gm": 4, "full": 1}, {"K": 4}, {"gm": 4, "K": 2}, {"gm": 16, "K": 16}):
        for n in (1, 2, 8, 33):
            _, f, seq = plan(exe, n, **mode)
            steps, forwards = steps_and_forwards(seq)
            assert len(steps) == f["launches"] == f["L"] + 1 and len(forwards) == f["L"]
            assert not any("<0,0>" in s for s in steps)
            assert "<0,1>" in steps[0] and "<1,0>" in steps[-1] and all("<1,1>" in s for s in steps[1:-1])


@pytest.mark.parametrize("W,K,active,cap,quantised", [(4096, 1, 4095, 4095, 4096), (4096, 1, 100, 100, 512), (4096, 1, 0, 4096, 4096),
                                                      (8192, 1, 5000, 5000, 8192), (2048, 1, 100, 100, 2048), (2048, 2, 100, 200, 512)])
def test_batch_caps(exe, W, K, active, cap, quantised):
    assert run(exe, "cap", W, K, active) == [f"{cap} {quantised}"]


def test_group_ranges(exe):
    assert run(exe, "range", 40, 4) == ["0 16", "16 32", "32 40", "40 40"]
    assert run(exe, "range", 4096, 2) == ["0 2048", "2048 4096"]
    assert run(exe, "range", 17, 2) == ["0 16", "16 17"]


def test_groups_auto(exe):
    NET, FAKE, OTHELLO, CONNECT4 = 0, 1, 0, 1
    auto = lambda *a: int(run(exe, "auto", *a)[0])
    assert [auto(NET, OTHELLO, 8, 8, G_) for G_ in (4095, 4096, 8191, 8192, 32767, 32768)] == [1, 2, 2, 1, 1, 2]
    assert [auto(NET, CONNECT4, 6, 7, G_) for G_ in (8191, 8192)] == [1, 4]
    assert [auto(FAKE, OTHELLO, 8, 8, 4096), auto(FAKE, CONNECT4, 6, 7, 8192)] == [1, 1]
    assert [auto(NET, OTHELLO, 6, 6, G_) for G_ in (4096, 32768)] == [1, 1]


def test_graph_keys(exe):
    def cmp(a, b):
        return run(exe, "keycmp", *a, *b)[0]
    # rollout, gm, K, full, cap, forced | n_sim, rows, g0, g1
    plain = (0, 0, 1, 0, 0, 0, 8, 32, 0, 32)
    others = {"cap": (0, 0, 1, 0, 1, 0, 8, 32, 0, 32), "forced": (0, 0, 1, 0, 0, 1, 8, 32, 0, 32), "cap+forced": (0, 0, 1, 0, 1, 1, 8, 32, 0, 32),
              "gumbel": (0, 4, 1, 0, 0, 0, 8, 32, 0, 32), "gumbel full": (0, 4, 1, 1, 0, 0, 8, 32, 0, 32), "multi": (0, 0, 4, 0, 0, 0, 8, 32, 0, 32),
              "gumbel multi": (0, 4, 2, 0, 0, 0, 8, 32, 0, 32), "gumbel multi full": (0, 4, 2, 1, 0, 0, 8, 32, 0, 32), "rollout": (1, 0, 1, 0, 0, 0, 8, 32, 0, 32),
              "n_sim": (0, 0, 1, 0, 0, 0, 9, 32, 0, 32), "cap rows": (0, 0, 1, 0, 0, 0, 8, 16, 0, 32), "g0": (0, 0, 1, 0, 0, 0, 8, 32, 16, 32),
              "g1": (0, 0, 1, 0, 0, 0, 8, 32, 0, 16)}
    assert cmp(plain, plain) == "=="
    every = [plain, *others.values()]
    for i, a in enumerate(every):
        assert cmp(a, a) == "=="
        for b in every[i + 1:]:
            assert {cmp(a, b), cmp(b, a)} == {"<", ">"}, (a, b)  # unequal, and ordered one way: what the map of graphs needs
