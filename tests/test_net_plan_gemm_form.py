"""CPU: which form of k_gemm the forward plans for a dense stage (alphazero_amd/csrc/az_net_plan.h: plan_dense, StagePlan::gemm_form,
NetTuning::gemm_form), pinned without a GPU in the manner of test_net_plan_host.py.  tests/net_plan_gemm_form.cpp is compiled with the
host C++ compiler and run as a child process; AZ_GEMM_FORM goes through the child's environment.  What is pinned: the rows and beside
values at which the rule picks the ring form (OthelloNet 8x8, beside launches on the 64 x 64 tile at one block per CU), the switch's
three settings, and that kernel, tile, family name and profile slot are the same under every setting at every row count
test_net_plan_host.py lists (test_rows_cover_the_host_test reads them from that file)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

OTH8, OTH6, C4, C4_56 = (0, 8, 8), (0, 6, 6), (1, 6, 7), (1, 5, 6)
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
# every row count of test_net_plan_host.py, with the thresholds of the 64 x 64 tile beside another chain
ROWS = (1, 128, 129, 256, 257, 512, 513, 1024, 1025, 1984, 1985, 2048, 2049, 3968, 3969, 4095, 4096, 4100, 8064, 8065, 8191, 8192, 16128, 16129, 16256,
        16257, 16383, 16384, 32512, 32513, 32767, 32768)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("net_plan_gemm_form") / "net_plan_gemm_form")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero_amd", "csrc"),
                           os.path.join(ROOT, "tests", "net_plan_gemm_form.cpp"), "-o", out])
    return out


def table(exe, net, rows, beside, **switches):
    """{(stage, B): (kernel, tile, family name, slot, form)} of one child process; no AZ_* variable but `switches` reaches it"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("AZ_")}
    env.update({k: str(v) for k, v in switches.items()})
    out = subprocess.run([exe, *map(str, net), str(beside), *map(str, rows)], env=env, capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines():
        stage, B, kernel, tile, family, slot, form = line.split("\t")
        got[int(stage), int(B)] = (kernel, tile, family, int(slot), form)
    assert len(got) == 2 * len(rows)
    return got


def test_rows_cover_the_host_test():
    """ROWS holds every row count test_net_plan_host.py passes to its table: the tuples it names `rows` or TRUNK_ROWS and the ones
    written into a table(...) call"""
    src = open(os.path.join(ROOT, "tests", "test_net_plan_host.py")).read()
    tuples = re.findall(r"ROWS = \(([\d, ]+)\)|rows = \(([\d, ]+)\)|table\(exe, \w+, \(([\d, ]+)\)", src)
    listed = {int(x) for groups in tuples for g in groups for x in g.replace(" ", "").split(",") if x}
    assert len(tuples) >= 20 and {8064, 16129, 32513} <= listed
    assert listed <= set(ROWS), sorted(listed - set(ROWS))


def test_rule_othello8(exe):
    """beside another chain the 64 x 64 tile runs from one block per CU up, and at one block per CU (at most 256 blocks) it takes the
    ring form: fc2 (K = 1024, N = 512) from 1985 rows, the first size on the tile, to 2048, the headline's group.  Everything else stays
    on the double buffer: fc2 above 2048 rows (264 blocks and more), fc1 (N = 1024: 272 blocks at its first size on the tile, 1025
    rows), every other tile, every lone launch."""
    b = table(exe, OTH8, ROWS, 1)
    lone = table(exe, OTH8, ROWS, 0)
    for B in ROWS:
        for stage in (1, 2):
            kernel, tile, family, slot, form = b[stage, B]
            ring = (kernel, tile) == ("k_gemm", "64x64") and stage == 2 and B <= 2048
            assert form == ("1" if ring else ("0" if kernel == "k_gemm" else "-")), (stage, B, b[stage, B])
            assert lone[stage, B][4] == ("0" if lone[stage, B][0] == "k_gemm" else "-"), (stage, B, lone[stage, B])
    assert [b[1, B][:2] + b[1, B][4:] for B in (1024, 1025, 2048, 3968, 3969)] == [("k_dense_frag", "-", "-"), ("k_gemm", "64x64", "0"), ("k_gemm", "64x64", "0"), ("k_gemm", "64x64", "0"), ("k_gemm", "128x64", "0")]
    assert [b[2, B][:2] + b[2, B][4:] for B in (1025, 1984, 1985, 2048, 2049, 4096)] == [("k_gemm", "64x128", "0"), ("k_gemm", "64x128", "0"), ("k_gemm", "64x64", "1"), ("k_gemm", "64x64", "1"), ("k_gemm", "64x64", "0"), ("k_gemm", "64x64", "0")]
    # the headline's two groups: the dense launches of a 2048-row group
    assert b[1, 2048] == ("k_gemm", "64x64", "k_gemm", 1, "0") and b[2, 2048] == ("k_gemm", "64x64", "k_gemm", 2, "1")
    # the same rows alone: fc1 on the tile in the double-buffer form, fc2 on k_dense_frag
    assert lone[1, 2048] == ("k_gemm", "64x64", "k_gemm", 1, "0") and lone[2, 2048][0] == "k_dense_frag"


def test_rule_is_the_measured_shape(exe):
    """the rule names what was measured, OthelloNet 8x8 beside k_trunk_quad<8,8,2>, and nothing else: othello6 (fc1: K = 128; fc2 the
    same K = 1024, N = 512 as 8x8, beside another trunk), Connect4 6x7 without the fused tail (fc1: K = 192) and on the 5x6 plane (K = 64,
    64 x 64 tiles for fc1 only, N = 64: one block per row band) stay on the double buffer at every row count; the switch reaches every
    64 x 64 launch of theirs"""
    for net, sw in ((OTH6, {}), (C4, {"AZ_NO_FUSED_TAIL": 1}), (C4_56, {})):
        for t in (table(exe, net, ROWS, 1, **sw), table(exe, net, ROWS, 0, **sw)):
            assert {v[4] for v in t.values()} <= {"0", "-"}, net
    b = table(exe, OTH6, (1024, 1025, 2048), 1)
    assert b[1, 1024][0] == "k_dense_frag" and b[1, 1025] == ("k_gemm", "64x64", "k_gemm", 1, "0") and b[1, 2048][4] == "0"
    assert b[2, 2048] == ("k_gemm", "64x64", "k_gemm", 2, "0") and table(exe, OTH6, (2048,), 1, AZ_GEMM_FORM=1)[2, 2048][4] == "1"
    assert table(exe, C4, (321,), 1, AZ_NO_FUSED_TAIL=1, AZ_GEMM_FORM=1)[1, 321] == ("k_gemm", "64x64", "k_gemm", 1, "1")  # K = 192: k_gemm_ring<., 6>
    assert table(exe, OTH6, (1025,), 1, AZ_GEMM_FORM=1)[1, 1025] == ("k_gemm", "64x64", "k_gemm", 1, "1")
    assert table(exe, OTH6, (1025,), 0)[1, 1025] == ("k_gemm", "64x128", "k_gemm", 1, "0")  # alone: too few 64 x 64 blocks
    c = table(exe, C4_56, (129, 4096, 16385), 1, AZ_GEMM_FORM=1)
    for B in (129, 4096, 16385):
        assert c[1, B][:2] == ("k_gemm", "64x64") and c[1, B][4] == "1", c[1, B]  # K = 64: the shortest ring
        assert c[2, B][:2] == ("k_gemm", "128x32") and c[2, B][4] == "0", c[2, B]  # no ring form off the 64 x 64 tile


@pytest.mark.parametrize("beside", [0, 1])
@pytest.mark.parametrize("net", [OTH8, OTH6, C4, C4_56])
def test_switch_and_names(exe, net, beside):
    """AZ_GEMM_FORM: 0 = the double buffer everywhere; 1 = the ring wherever it exists (every 64 x 64 launch), lone launches included;
    unset = the rule.  Kernel, tile, family name and slot do not move with it."""
    sw = {"AZ_NO_FUSED_TAIL": 1} if net == C4 else {}
    rule, off, on = (table(exe, net, ROWS, beside, **sw, **f) for f in ({}, {"AZ_GEMM_FORM": 0}, {"AZ_GEMM_FORM": 1}))
    for key in rule:
        assert rule[key][:4] == off[key][:4] == on[key][:4], key
        kernel, tile = rule[key][:2]
        assert off[key][4] == ("0" if kernel == "k_gemm" else "-"), key
        assert on[key][4] == (("1" if tile == "64x64" else "0") if kernel == "k_gemm" else "-"), key
        if not beside:
            assert rule[key][4] == off[key][4], key
    # another value of the switch is the rule's "not 1": the double buffer
    assert table(exe, net, (2048,), 1, AZ_GEMM_FORM=7, **sw)[1, 2048][4] in ("0", "-")
