"""CPU: where the forward plans k_trunk_quad's prefetching form with vector stores (alphazero_amd/csrc/az_net_plan.h: plan_trunk,
StagePlan::quad_stores, NetTuning::trunk_quad_stores), pinned without a GPU in the manner of test_net_plan_trunk_prefetch.py.
tests/net_plan_trunk_stores.cpp is compiled with the host C++ compiler and run as a child process; AZ_TRUNK_QUAD_STORES goes through
the child's environment.  What is pinned: the rule answers 1 for exactly the launches that take the prefetching form by its rule
(OthelloNet 8x8 beside another chain, 513 .. 4095 boards) and 0 for every other net, plane, row count and lone launch; the switch
forces 0 / 1, and 1 reaches only launches that run the prefetching form; kernel, variant, family name, profile slot and the prefetch
flag of every stage are the same under every setting at every row count test_net_plan_host.py lists.  The offset-addressed form of
k_gemm that the same work measured lost in the headline and left no plan field: the dense stages' variants are
compared with the switch to show that nothing of theirs moves."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_net_plan_gemm_form import ROWS

OTH8, OTH6, C4, C4_56 = (0, 8, 8), (0, 6, 6), (1, 6, 7), (1, 5, 6)
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
SW, PF = "AZ_TRUNK_QUAD_STORES", "AZ_TRUNK_QUAD_PREFETCH"
QUAD2 = ("k_trunk_quad", "wino form=2 lds_blocks=0", "k_trunk", 4)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("net_plan_trunk_stores") / "net_plan_trunk_stores")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero_amd", "csrc"),
                           os.path.join(ROOT, "tests", "net_plan_trunk_stores.cpp"), "-o", out])
    return out


def table(exe, net, rows, beside, **switches):
    """{(stage, B): (kernel, variant, family name, slot, prefetch, stores)} of one child process; no AZ_* variable but `switches` reaches it"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("AZ_")}
    env.update({k: str(v) for k, v in switches.items()})
    out = subprocess.run([exe, *map(str, net), str(beside), *map(str, rows)], env=env, capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines():
        stage, B, kernel, variant, family, slot, pf, st = line.split("\t")
        got[int(stage), int(B)] = (kernel, variant, family, int(slot), pf, st)
    assert len(got) == 4 * len(rows)
    return got


def test_rule_othello8(exe):
    """beside another chain OthelloNet 8x8 runs k_trunk_quad form 2 from 513 to 4095 boards in the prefetching form, and every one of
    those launches stores vectors; no other stage carries the flag; a lone launch is not k_trunk_quad and carries none"""
    b, lone = table(exe, OTH8, ROWS, 1), table(exe, OTH8, ROWS, 0)
    for B in ROWS:
        quad = 513 <= B <= 4095
        assert b[0, B][4:] == (("1", "1") if quad else ("-", "-")), (B, b[0, B])
        assert lone[0, B][4:] == ("-", "-"), (B, lone[0, B])
        for stage in (1, 2, 3):
            assert b[stage, B][4:] == ("-", "-") and lone[stage, B][4:] == ("-", "-")
    for B in (513, 2048, 4095):  # the smallest launch on the kernel, the headline's group, the largest
        assert b[0, B] == QUAD2 + ("1", "1")
    assert b[0, 512][0] == "k_trunk_q" and b[0, 4096][0] == "k_trunk2"


def test_switch(exe):
    """AZ_TRUNK_QUAD_STORES: 0 = scalar stores everywhere; 1 = vector stores wherever the prefetching form runs, a lone launch forced
    onto it included, and nowhere else; unset = the rule; another value = the rule's "not 1\""""
    for B in (513, 2048, 4095):
        assert table(exe, OTH8, (B,), 1, **{SW: 0})[0, B] == QUAD2 + ("1", "0")
        assert table(exe, OTH8, (B,), 1, **{SW: 1})[0, B] == QUAD2 + ("1", "1")
        assert table(exe, OTH8, (B,), 1, **{SW: 7})[0, B] == QUAD2 + ("1", "0")
        # without the prefetching form there is nothing to store vectors from: its switch at 0, forms 0 and 1
        for sw in ({}, {SW: 1}):
            assert table(exe, OTH8, (B,), 1, **{PF: 0}, **sw)[0, B] == QUAD2 + ("0", "0"), (B, sw)
            for form in (0, 1):
                assert table(exe, OTH8, (B,), 1, AZ_TRUNK_QUAD_FORM=form, **sw)[0, B][4:] == ("0", "0"), (B, form, sw)
        # a lone launch forced onto k_trunk_quad: the rule says 0 for both; each switch reaches its own form
        assert table(exe, OTH8, (B,), 0, AZ_TRUNK_QUAD=1)[0, B] == QUAD2 + ("0", "0")
        assert table(exe, OTH8, (B,), 0, AZ_TRUNK_QUAD=1, **{SW: 1})[0, B] == QUAD2 + ("0", "0")
        assert table(exe, OTH8, (B,), 0, AZ_TRUNK_QUAD=1, **{PF: 1})[0, B] == QUAD2 + ("1", "0")
        assert table(exe, OTH8, (B,), 0, AZ_TRUNK_QUAD=1, **{PF: 1, SW: 1})[0, B] == QUAD2 + ("1", "1")
    assert table(exe, OTH8, (2048,), 1, AZ_WINOGRAD=0, **{SW: 1})[0, 2048][4:] == ("-", "-")  # no Winograd conv2, no k_trunk_quad


def test_rule_is_the_measured_shape(exe):
    """other nets and planes stay at 0 under every setting: Connect4 7x6 runs k_trunk_quad form 1, for which neither form is built;
    the 6x6 and 5x6 planes have no k_trunk_quad"""
    for beside in (0, 1):
        for sw in ({}, {SW: 0}, {SW: 1}, {SW: 1, PF: 1}):
            c4 = table(exe, C4, ROWS, beside, **sw)
            assert {c4[0, B][4:] for B in ROWS if 513 <= B <= 4095} == {("0", "0")} and c4[0, 2048][:2] == ("k_trunk_quad", "wino form=1 lds_blocks=3")
            for net in (OTH6, C4_56):
                t = table(exe, net, ROWS, beside, **sw)
                assert {v[4:] for v in t.values()} == {("-", "-")}, (net, beside, sw)


@pytest.mark.parametrize("beside", [0, 1])
@pytest.mark.parametrize("net", [OTH8, OTH6, C4, C4_56])
def test_names_do_not_move(exe, net, beside):
    """kernel, variant string (the dense stages' tile and form among them), family name, profile slot and prefetch flag of every stage
    at every row count of test_net_plan_host.py (ROWS: checked against that file by test_net_plan_gemm_form.py) are the same under the
    rule, 0 and 1"""
    rule, off, on = (table(exe, net, ROWS, beside, **f) for f in ({}, {SW: 0}, {SW: 1}))
    for key in rule:
        assert rule[key][:5] == off[key][:5] == on[key][:5], key
        assert off[key][5] in ("0", "-") and (off[key][5] == "-") == (rule[key][0] != "k_trunk_quad"), key
        if not beside:
            assert rule[key][5] == off[key][5], key
