"""CPU: where the forward plans k_trunk_quad's prefetching form (alphazero_amd/csrc/az_net_plan.h: plan_trunk, StagePlan::quad_prefetch,
NetTuning::trunk_quad_prefetch), pinned without a GPU in the manner of test_net_plan_gemm_form.py.  tests/net_plan_trunk_prefetch.cpp is
compiled with the host C++ compiler and run as a child process; AZ_TRUNK_QUAD_PREFETCH goes through the child's environment.  What is
pinned: the rows and beside values at which the rule answers 1 (OthelloNet 8x8 beside another chain, every row count that runs
k_trunk_quad there), the switch's three settings, that lone launches, other nets and other planes stay at 0, and that kernel, variant,
family name and profile slot of every stage are the same under every setting at every row count test_net_plan_host.py lists."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_net_plan_gemm_form import ROWS

OTH8, OTH6, C4, C4_56 = (0, 8, 8), (0, 6, 6), (1, 6, 7), (1, 5, 6)
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
SW = "AZ_TRUNK_QUAD_PREFETCH"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("net_plan_trunk_prefetch") / "net_plan_trunk_prefetch")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero_amd", "csrc"),
                           os.path.join(ROOT, "tests", "net_plan_trunk_prefetch.cpp"), "-o", out])
    return out


def table(exe, net, rows, beside, **switches):
    """{(stage, B): (kernel, variant, family name, slot, prefetch)} of one child process; no AZ_* variable but `switches` reaches it"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("AZ_")}
    env.update({k: str(v) for k, v in switches.items()})
    out = subprocess.run([exe, *map(str, net), str(beside), *map(str, rows)], env=env, capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines():
        stage, B, kernel, variant, family, slot, pf = line.split("\t")
        got[int(stage), int(B)] = (kernel, variant, family, int(slot), pf)
    assert len(got) == 4 * len(rows)
    return got


def test_rule_othello8(exe):
    """beside another chain OthelloNet 8x8 runs k_trunk_quad form 2 from 513 to 4095 boards, and every one of those launches takes the
    prefetching form; the dense stages and the heads carry no flag; a lone launch is k_trunk and carries none either"""
    b, lone = table(exe, OTH8, ROWS, 1), table(exe, OTH8, ROWS, 0)
    for B in ROWS:
        quad = 513 <= B <= 4095
        assert (b[0, B][0] == "k_trunk_quad") == quad, (B, b[0, B])
        assert b[0, B][4] == ("1" if quad else "-"), (B, b[0, B])
        assert lone[0, B][0] != "k_trunk_quad" and lone[0, B][4] == "-", (B, lone[0, B])
        for stage in (1, 2, 3):
            assert b[stage, B][4] == "-" and lone[stage, B][4] == "-"
    # the headline's two groups: the trunk of a 2048-row group, and the smallest and largest launches on the kernel
    for B in (513, 2048, 4095):
        assert b[0, B] == ("k_trunk_quad", "wino form=2 lds_blocks=0", "k_trunk", 4, "1")
    assert b[0, 512][0] == "k_trunk_q" and b[0, 4096][0] == "k_trunk2"


def test_switch(exe):
    """AZ_TRUNK_QUAD_PREFETCH: 0 = k_trunk_quad as it was everywhere; 1 = the prefetching form on every k_trunk_quad launch that has an
    instantiation (8x8, form 2), lone launches forced onto k_trunk_quad included; unset = the rule; another value = the rule's "not 1\""""
    for B in (513, 2048, 4095):
        assert table(exe, OTH8, (B,), 1, **{SW: 0})[0, B] == ("k_trunk_quad", "wino form=2 lds_blocks=0", "k_trunk", 4, "0")
        assert table(exe, OTH8, (B,), 1, **{SW: 1})[0, B][4] == "1"
        assert table(exe, OTH8, (B,), 1, **{SW: 7})[0, B][4] == "0"
        # a lone launch forced onto k_trunk_quad: the rule says 0 (not the measured regime), the switch reaches it
        assert table(exe, OTH8, (B,), 0, AZ_TRUNK_QUAD=1)[0, B] == ("k_trunk_quad", "wino form=2 lds_blocks=0", "k_trunk", 4, "0")
        assert table(exe, OTH8, (B,), 0, AZ_TRUNK_QUAD=1, **{SW: 1})[0, B][4] == "1"
        # forms 0 and 1 have no prefetching instantiation: 0 under every setting
        for form in (0, 1):
            for sw in ({}, {SW: 0}, {SW: 1}):
                assert table(exe, OTH8, (B,), 1, AZ_TRUNK_QUAD_FORM=form, **sw)[0, B][4] == "0", (B, form, sw)
    # without the Winograd conv2 there is no k_trunk_quad
    assert table(exe, OTH8, (2048,), 1, AZ_WINOGRAD=0, **{SW: 1})[0, 2048][4] == "-"


def test_rule_is_the_measured_shape(exe):
    """other nets and planes stay at 0 under every setting: Connect4 7x6 runs k_trunk_quad form 1 alone and beside, for which the form
    is not built; the 6x6 plane and the 5x6 plane have no k_trunk_quad; forcing form 2 on 7x6 does not find an instantiation either"""
    for beside in (0, 1):
        for sw in ({}, {SW: 0}, {SW: 1}):
            c4 = table(exe, C4, ROWS, beside, **sw)
            assert {c4[0, B][4] for B in ROWS if 513 <= B <= 4095} == {"0"} and c4[0, 2048][:2] == ("k_trunk_quad", "wino form=1 lds_blocks=3")
            for net in (OTH6, C4_56):
                t = table(exe, net, ROWS, beside, **sw)
                assert {v[4] for v in t.values()} == {"-"}, (net, beside, sw)
    assert table(exe, C4, (2048,), 1, AZ_TRUNK_QUAD_FORM=2, **{SW: 1})[0, 2048][4] == "0"


@pytest.mark.parametrize("beside", [0, 1])
@pytest.mark.parametrize("net", [OTH8, OTH6, C4, C4_56])
def test_names_do_not_move(exe, net, beside):
    """kernel, variant string, family name and profile slot of every stage at every row count of test_net_plan_host.py (ROWS: checked
    against that file by test_net_plan_gemm_form.py) are the same under the rule, 0 and 1"""
    rule, off, on = (table(exe, net, ROWS, beside, **f) for f in ({}, {SW: 0}, {SW: 1}))
    for key in rule:
        assert rule[key][:4] == off[key][:4] == on[key][:4], key
        assert off[key][4] in ("0", "-") and (off[key][4] == "-") == (rule[key][0] != "k_trunk_quad"), key
