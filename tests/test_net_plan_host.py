"""CPU: which kernel the network forward plans for a stage (alphazero_amd/csrc/az_net_plan.h: plan_stage, NetTuning), pinned without a
GPU.  tests/net_plan_table.cpp is compiled with the host C++ compiler and run as a child process; an AZ_* switch goes through the
child's environment, so every case reads its switches afresh (the library reads them once per process).  What is pinned: the kernel and
its variant per (net, stage, rows, lone | beside), the family name az_net_stage_kernel returns, and the az_net_profile slot."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

OTH8, OTH6, C4, C4_56 = (0, 8, 8), (0, 6, 6), (1, 6, 7), (1, 5, 6)  # game id, H, W; Connect4's plane is W x H: 7x6 and 6x5
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("net_plan") / "net_plan_table")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero_amd", "csrc"),
                           os.path.join(ROOT, "tests", "net_plan_table.cpp"), "-o", out])
    return out


def table(exe, net, rows, beside=0, qd=0, **switches):
    """{(stage, B): (kernel, variant, family name, slot)} of one child process; no AZ_* variable but `switches` reaches it"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("AZ_")}
    env.update({k: str(v) for k, v in switches.items()})
    out = subprocess.run([exe, *map(str, net), str(qd), str(beside), *map(str, rows)], env=env, capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines():
        stage, B, kernel, variant, family, slot = line.split("\t")
        got[int(stage), int(B)] = (kernel, variant, family, int(slot))
    assert len(got) == 4 * len(rows)
    return got


TRUNK_ROWS = (1, 256, 257, 512, 513, 4095, 4096, 32768)


@pytest.mark.parametrize("beside", [0, 1])
@pytest.mark.parametrize("net,form", [(OTH8, "wino"), (OTH6, "direct"), (C4, "wino")])
def test_trunk_of_the_tuned_planes(exe, net, form, beside):
    t = table(exe, net, TRUNK_ROWS, beside)
    for B in (1, 256):
        assert t[0, B] == ("k_trunk_q", f"{form} waves=8", "k_trunk_q", 7)
    for B in (257, 512):
        assert t[0, B] == ("k_trunk_q", f"{form} waves=4", "k_trunk_q", 7)
    for B in (513, 4095):
        if net == C4:  # the shared-row-tile form, lone and beside: four passes, U one k-step ahead, the padded LDS request
            assert t[0, B] == ("k_trunk_quad", "wino form=1 lds_blocks=3", "k_trunk", 4)
        elif net == OTH8 and beside:  # four passes, U two k-steps ahead, the kernel's natural LDS size
            assert t[0, B] == ("k_trunk_quad", "wino form=2 lds_blocks=0", "k_trunk", 4)
        else:
            assert t[0, B] == ("k_trunk", f"{form} lds_blocks=3", "k_trunk", 4)
    for B in (4096, 32768):
        if form == "wino":
            assert t[0, B] == ("k_trunk2", "wino waves=4", "k_trunk2<Winograd conv2>", 0)
        else:
            assert t[0, B] == ("k_trunk2", "direct waves=8", "k_trunk2", 0)


@pytest.mark.parametrize("beside", [0, 1])
def test_trunk_of_another_plane(exe, beside):
    t = table(exe, C4_56, (1, 512, 513, 4096), beside)
    for B in (1, 512, 513, 4096):
        assert t[0, B] == ("k_trunk", "direct lds_blocks=3", "k_trunk", 4)


def kernels(t, stage, rows):
    return [t[stage, B][0] for B in rows]


@pytest.mark.parametrize("beside", [0, 1])
def test_othello8_fc1(exe, beside):
    rows = (1, 1024, 1025, 8064, 8065, 16128, 16129, 32768)
    t = table(exe, OTH8, rows, beside)
    assert kernels(t, 1, rows) == ["k_dense_frag"] * 2 + ["k_gemm"] * 2 + ["k_gemm_solo_t"] * 2 + ["k_gemm_solo"] * 2
    assert [t[1, B][3] for B in rows] == [5, 5, 1, 1, 1, 1, 1, 1]
    assert all(t[1, B][2] == t[1, B][0] for B in rows)  # the family name is the kernel's


def test_othello8_fc2_lone(exe):
    rows = (1, 2048, 2049, 16256, 16257, 32512, 32513)
    t = table(exe, OTH8, rows)
    assert kernels(t, 2, rows) == ["k_dense_frag"] * 2 + ["k_gemm"] * 2 + ["k_gemm_solo_t"] * 2 + ["k_gemm_solo"]
    assert [t[2, B][3] for B in rows] == [6, 6, 2, 2, 2, 2, 2]
    assert t[2, 2049][1] == "64x128"


def test_othello8_fc2_beside(exe):
    rows = (1, 1024, 1025, 1984, 1985, 2048, 2049)
    t = table(exe, OTH8, rows, beside=1)
    assert kernels(t, 2, rows) == ["k_dense_frag"] * 2 + ["k_gemm"] * 5
    assert [t[2, B][1] for B in rows[2:]] == ["64x128", "64x128", "64x64", "64x64", "64x64"]
    assert [t[2, B][3] for B in rows] == [6, 6, 2, 2, 2, 2, 2]


@pytest.mark.parametrize("beside", [0, 1])
def test_othello6_fc1(exe, beside):
    t = table(exe, OTH6, (1, 1024, 1025), beside)
    assert kernels(t, 1, (1, 1024, 1025)) == ["k_dense_frag", "k_dense_frag", "k_gemm"]


@pytest.mark.parametrize("net,nt", [(OTH8, 5), (OTH6, 3)])
def test_othello_heads(exe, net, nt):
    for beside in (0, 1):
        t = table(exe, net, (1, 128, 4096), beside)
        for B in (1, 128, 4096):
            assert t[3, B] == ("k_heads2", f"nt={nt} rh=1", "k_heads2", 3)


@pytest.mark.parametrize("beside", [0, 1])
def test_connect4_fused_tail(exe, beside):
    t = table(exe, C4, (1, 128, 129, 4096), beside)
    for B in (1, 128, 129, 4096):
        assert t[1, B] == ("k_tail_mfma", "-", "k_tail_mfma", 1)  # the fc1 tiled slot
        for stage in (2, 3):
            assert t[stage, B] == ("nothing", "-", "k_tail_mfma", 1)


def test_connect4_5x6(exe):
    t = table(exe, C4_56, (128, 129))
    assert t[1, 128] == ("k_dense_small", "-", "k_dense_small", 5) and t[1, 129] == ("k_gemm", "64x64", "k_gemm", 1)
    assert t[2, 128] == ("k_dense_small", "-", "k_dense_small", 6) and t[2, 129] == ("k_gemm", "128x32", "k_gemm", 2)
    assert t[3, 128] == ("k_heads_small", "-", "k_heads_small", 3) and t[3, 129] == ("k_heads", "nt=1", "k_heads", 3)


def test_fixed_point_dense_layers(exe):
    rows = (1, 512, 513, 3968, 3969, 8064, 8065)
    t = table(exe, OTH8, rows, qd=1)
    both = "k_q_rows + k_qgemm"
    for B in (1, 512):
        assert t[1, B] == ("k_qdense_small", "-", "k_qdense_small", 5) and t[2, B] == ("k_qdense_small", "-", "k_qdense_small", 6)
    assert [t[1, B] for B in rows[2:]] == [(both, "<2,4,1,1>", both, 1)] * 2 + [(both, "<4,2,1,2>", both, 1)] * 3
    assert [t[2, B] for B in rows[2:]] == [(both, "<2,4,1,1>", both, 2)] * 4 + [(both, "<4,2,1,2>", both, 2)]


# ---- overrides, one child each ----

def test_trunk_v1_never_k_trunk2(exe):
    for net in (OTH8, OTH6, C4):
        for beside in (0, 1):
            t = table(exe, net, (4096, 32768), beside, AZ_TRUNK_V1=1)
            assert all(k in ("k_trunk", "k_trunk_quad") for k in kernels(t, 0, (4096, 32768)))
            assert all(t[0, B][2:] == ("k_trunk", 4) for B in (4096, 32768))


def test_trunk_q_max_0_never_k_trunk_q(exe):
    for net in (OTH8, OTH6, C4):
        t = table(exe, net, (1, 256, 512), AZ_TRUNK_Q_MAX=0)
        assert kernels(t, 0, (1, 256, 512)) == ["k_trunk_quad" if net == C4 else "k_trunk"] * 3


def test_trunk_quad_forces_the_form_on_8x8_and_7x6_only(exe):
    for net in (OTH8, C4):
        for beside in (0, 1):
            assert table(exe, net, (513,), beside, AZ_TRUNK_QUAD=0)[0, 513][0] == "k_trunk"
            assert table(exe, net, (513,), beside, AZ_TRUNK_QUAD=1)[0, 513][0] == "k_trunk_quad"
    assert table(exe, OTH8, (513,), AZ_TRUNK_QUAD=1)[0, 513] == ("k_trunk_quad", "wino form=2 lds_blocks=0", "k_trunk", 4)
    for net in (OTH6, C4_56):
        assert table(exe, net, (513,), 1, AZ_TRUNK_QUAD=1)[0, 513][0] == "k_trunk"


def test_trunk_quad_form_0_has_the_padded_lds_request(exe):
    assert table(exe, C4, (513,), AZ_TRUNK_QUAD_FORM=0)[0, 513] == ("k_trunk_quad", "wino form=0 lds_blocks=3", "k_trunk", 4)
    assert table(exe, OTH8, (513,), 1, AZ_TRUNK_QUAD_FORM=0)[0, 513] == ("k_trunk_quad", "wino form=0 lds_blocks=3", "k_trunk", 4)


def test_winograd_0_is_the_direct_form_and_no_quad(exe):
    for net in (OTH8, C4):
        t = table(exe, net, (256, 513, 4096), 1, AZ_WINOGRAD=0)
        assert t[0, 256] == ("k_trunk_q", "direct waves=8", "k_trunk_q", 7)
        assert t[0, 513] == ("k_trunk", "direct lds_blocks=3", "k_trunk", 4)
        assert t[0, 4096] == ("k_trunk2", "direct waves=8", "k_trunk2", 0)


def test_dense_frag_max_0(exe):
    rows = (1, 128, 129, 256, 257, 1024)
    t = table(exe, OTH8, rows, AZ_DENSE_FRAG_MAX=0)
    assert kernels(t, 1, rows) == ["k_dense_small"] * 2 + ["k_gemm"] * 4  # K = 512
    assert kernels(t, 2, rows) == ["k_dense_small"] * 4 + ["k_gemm"] * 2  # K = 1024


def test_gemm_solo_0(exe):
    t = table(exe, OTH8, (32768,), AZ_GEMM_SOLO=0)
    assert t[1, 32768][0] == "k_gemm" and t[2, 32768][0] == "k_gemm"


def test_heads_v1_and_its_name(exe):
    t = table(exe, OTH8, (1, 4096), AZ_HEADS_V1=1)
    assert t[3, 1] == t[3, 4096] == ("k_heads", "nt=5", "k_heads", 3)


def test_no_fused_tail(exe):
    t = table(exe, C4, (128, 129), AZ_NO_FUSED_TAIL=1)
    assert [t[s, 128][0] for s in (1, 2, 3)] == ["k_dense_small", "k_dense_small", "k_heads_small"]
    assert [t[s, 129][0] for s in (1, 2, 3)] == ["k_gemm", "k_gemm", "k_heads"]
    assert [t[s, 129][3] for s in (1, 2, 3)] == [1, 2, 3]


def test_tail_v1(exe):
    t = table(exe, C4, (128, 8192), AZ_TAIL_V1=1)
    for B in (128, 8192):
        assert t[1, B] == ("k_tail_small", "R=4", "k_tail_small", 1)
        assert t[2, B] == t[3, B] == ("nothing", "-", "k_tail_small", 1)
