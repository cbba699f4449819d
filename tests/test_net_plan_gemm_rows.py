"""CPU: the rows per block of k_gemm's 64 x 64 tile (alphazero_amd/csrc/az_net_plan.h: gemm_rows_per_block, StagePlan::gemm_rows,
NetTuning::gemm_rows), pinned without a GPU in the manner of test_net_plan_gemm_form.py.  tests/net_plan_gemm_rows.cpp is compiled with
the host C++ compiler and run as a child process; AZ_GEMM_ROWS goes through the child's environment.  What is pinned: the thresholds of
the rule for 17, 32 and 33 row bands; where the plan lets the rows follow the count (OthelloNet 8x8, beside launches of the 64 x 64
tile, in either form), the switch's three settings, and that kernel, tile, family name, profile slot and form are the same under
every setting at every row count test_net_plan_gemm_form.py lists."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

OTH8, OTH6, C4, C4_56 = (0, 8, 8), (0, 6, 6), (1, 6, 7), (1, 5, 6)
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
ROWS = (1, 128, 129, 256, 257, 512, 513, 1024, 1025, 1984, 1985, 2048, 2049, 3968, 3969, 4095, 4096, 4100, 8064, 8065, 8191, 8192, 16128, 16129, 16256,
        16257, 16383, 16384, 32512, 32513, 32767, 32768)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("net_plan_gemm_rows") / "net_plan_gemm_rows")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero_amd", "csrc"),
                           os.path.join(ROOT, "tests", "net_plan_gemm_rows.cpp"), "-o", out])
    return out


def run(exe, args, **switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("AZ_")}
    env.update({k: str(v) for k, v in switches.items()})
    return subprocess.run([exe, *map(str, args)], env=env, capture_output=True, text=True, check=True).stdout.splitlines()


def table(exe, net, rows, beside, **switches):
    """{(stage, B): (kernel, tile, family name, slot, form, rows)} of one child process; no AZ_* variable but `switches` reaches it"""
    got = {}
    for line in run(exe, ["plan", *net, beside, *rows], **switches):
        stage, B, kernel, tile, family, slot, form, follow = line.split("\t")
        got[int(stage), int(B)] = (kernel, tile, family, int(slot), form, follow)
    assert len(got) == 2 * len(rows)
    return got


def rule(exe, follow, gy, ms):
    got = {}
    for line in run(exe, ["rule", follow, gy, *ms]):
        g, m, r = map(int, line.split("\t"))
        assert g == gy
        got[m] = r
    return got


@pytest.mark.parametrize("gy", [17, 32, 33])
def test_thresholds(exe, gy):
    """16 rows per block while ceil(M / 16) <= GY, 32 while ceil(M / 32) <= GY, else 64; a count of 0 is a 16-row launch whose every
    block leaves; 17 bands: a 1025-row launch, 32: 1985 .. 2048 rows, 33: 2049 rows"""
    ms = [0, 1, 15, 16, 17, 16 * gy - 1, 16 * gy, 16 * gy + 1, 32 * gy - 1, 32 * gy, 32 * gy + 1, 64 * gy - 1, 64 * gy]
    on, off = rule(exe, 1, gy, ms), rule(exe, 0, gy, ms)
    for m in ms:
        assert on[m] == (16 if m <= 16 * gy else 32 if m <= 32 * gy else 64), (gy, m)
        assert off[m] == 64, (gy, m)
        assert on[m] * gy >= m, "the bands cover the count"
    assert {17: (272, 544), 32: (512, 1024), 33: (528, 1056)}[gy] == (16 * gy, 32 * gy)


def test_rule_othello8(exe):
    """the rows follow the count on every beside launch of OthelloNet 8x8 that runs the 64 x 64 tile, fc1 in the double-buffer form
    (1025 .. 3968 rows) and fc2 in the ring form (1985 .. 2048) or the double buffer (from 2049); on no other tile and no lone launch"""
    b, lone = table(exe, OTH8, ROWS, 1), table(exe, OTH8, ROWS, 0)
    for key in b:
        kernel, tile = b[key][:2]
        assert b[key][5] == (("1" if tile == "64x64" else "0") if kernel == "k_gemm" else "-"), (key, b[key])
        assert lone[key][5] == ("0" if lone[key][0] == "k_gemm" else "-"), (key, lone[key])
    assert b[1, 2048] == ("k_gemm", "64x64", "k_gemm", 1, "0", "1") and b[2, 2048] == ("k_gemm", "64x64", "k_gemm", 2, "1", "1")
    assert b[1, 1025][5] == "1" and b[2, 1025][:2] + b[2, 1025][5:] == ("k_gemm", "64x128", "0") and b[2, 1985][4:] == ("1", "1")
    assert b[1, 1024][0] == "k_dense_frag" and b[2, 2049][4:] == ("0", "1") and b[1, 3969][1:2] + b[1, 3969][5:] == ("128x64", "0")


def test_rule_is_the_measured_shape(exe):
    """other nets and planes reach the narrow forms through the switch only, and only where they exist: the 64 x 64 tile with
    K = 512 (double buffer) or 1024 (either form) -- othello6's fc2; Connect4's K = 192 and 64 have none"""
    for net, sw in ((OTH6, {}), (C4, {"AZ_NO_FUSED_TAIL": 1}), (C4_56, {})):
        for beside in (0, 1):
            assert {v[5] for v in table(exe, net, ROWS, beside, **sw).values()} <= {"0", "-"}, net
            on = table(exe, net, ROWS, beside, AZ_GEMM_ROWS=1, **sw)
            for (stage, B), v in on.items():
                exists = net == OTH6 and stage == 2 and v[:2] == ("k_gemm", "64x64")
                assert v[5] == (("1" if exists else "0") if v[0] == "k_gemm" else "-"), (net, stage, B, v)
    assert table(exe, OTH6, (2048,), 1, AZ_GEMM_ROWS=1)[2, 2048] == ("k_gemm", "64x64", "k_gemm", 2, "0", "1")
    # the ring form has the narrow forms for K = 1024 only: OthelloNet 8x8's fc1 (K = 512) forced onto the ring keeps 64 rows
    forced = table(exe, OTH8, (2048,), 1, AZ_GEMM_FORM=1)
    assert forced[1, 2048][4:] == ("1", "0") and forced[2, 2048][4:] == ("1", "1")


@pytest.mark.parametrize("beside", [0, 1])
@pytest.mark.parametrize("net", [OTH8, OTH6, C4, C4_56])
def test_switch_and_names(exe, net, beside):
    """AZ_GEMM_ROWS: 0 = 64 rows everywhere; 1 = the narrow forms wherever they exist, lone launches included; unset = the rule.
    Kernel, tile, family name, profile slot and form do not move with it."""
    sw = {"AZ_NO_FUSED_TAIL": 1} if net == C4 else {}
    by_rule, off, on = (table(exe, net, ROWS, beside, **sw, **f) for f in ({}, {"AZ_GEMM_ROWS": 0}, {"AZ_GEMM_ROWS": 1}))
    for key in by_rule:
        assert by_rule[key][:5] == off[key][:5] == on[key][:5], key
        kernel, tile = by_rule[key][:2]
        assert off[key][5] == ("0" if kernel == "k_gemm" else "-"), key
        if net == OTH8:
            assert on[key][5] == (("1" if tile == "64x64" else "0") if kernel == "k_gemm" else "-"), key
        if not beside:
            assert by_rule[key][5] == off[key][5], key
    # any other value of the switch that is not 0 counts as 1
    assert table(exe, OTH8, (2048,), 0, AZ_GEMM_ROWS=7)[1, 2048][5] == "1"
