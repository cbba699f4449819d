"""CPU: the rule of the heads inside the search step kernel (alphazero_amd/csrc/az_search_plan.h: step_heads_served, step_heads_auto,
step_heads_in_force), pinned without a GPU.  tests/step_heads_table.cpp is compiled with the host C++ compiler and
run as a child process.  What is pinned: where the form is served, what every value of AZ_ENGINE_STEP_HEADS answers there, the shapes
the measured rule turns it on at (profiles/r30_step_heads.txt) and that every other shape stays off, that every unserved search mode
leaves k_step's kernel family (the only one the form is launched from), and that header and binding name the entry points."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
UNSET, NEVER, WHEREVER = -1, 0, 1
NET, FAKE, ROLLOUT, EXTERNAL = 0, 1, 2, 3
OTHELLO, CONNECT4, TICTACTOE = 0, 1, 2
# (game, H, W, slots) of the table below that the rule turns the form on at: Othello 8x8 from 512 slots (measured: +2.3 %) through
# 4096 (+2.0 %) up to 8191; 32768 was measured and lost, 8192 .. 32767 were not measured
MEASURED_ON = ((OTHELLO, 8, 8, 512), (OTHELLO, 8, 8, 2112), (OTHELLO, 8, 8, 4095), (OTHELLO, 8, 8, 4096), (OTHELLO, 8, 8, 8191))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("step_heads") / "step_heads_table")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero_amd", "csrc"),
                           os.path.join(ROOT, "tests", "step_heads_table.cpp"), "-o", out])
    return out


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.split()


def rule(exe, request, evaluator=NET, game=OTHELLO, H=8, W=8, G=4096, plain=1, shape=1, profiled=0):
    in_force, auto, served = map(int, run(exe, "rule", request, evaluator, game, H, W, G, plain, shape, profiled))
    return bool(in_force), bool(auto), bool(served)


def test_the_rule_turns_the_form_on_at_the_measured_shapes_only(exe):
    for game, H, W in ((OTHELLO, 8, 8), (OTHELLO, 6, 6), (CONNECT4, 6, 7), (TICTACTOE, 3, 3)):
        for G in (1, 16, 512, 2112, 4095, 4096, 8191, 8192, 32768, 65536):
            on = (game, H, W, G) in MEASURED_ON
            assert rule(exe, UNSET, game=game, H=H, W=W, G=G) == (on, on, True), (game, H, W, G)
    for shape in MEASURED_ON:
        assert shape[0] == OTHELLO  # k_heads2's shapes are OthelloNet's: nothing else can have been measured


def test_the_switch_where_the_form_is_served(exe):
    for G in (1, 17, 4096, 32768):
        assert rule(exe, WHEREVER, G=G)[0] is True
        assert rule(exe, NEVER, G=G)[0] is False
    assert rule(exe, WHEREVER, game=OTHELLO, H=6, W=6, G=48)[0] is True  # wherever served: the 48-logit heads too


@pytest.mark.parametrize("evaluator,plain,shape,profiled", [(FAKE, 1, 1, 0), (ROLLOUT, 1, 1, 0), (EXTERNAL, 1, 1, 0), (NET, 0, 1, 0), (NET, 1, 0, 0),
                                                            (NET, 1, 1, 1), (NET, 0, 0, 1)])
def test_refusals(exe, evaluator, plain, shape, profiled):
    """another evaluator, a mode beyond the plain one-leaf search, a net whose heads k_heads2 has no instantiation for and a net under
    az_net_profile: off whatever the switch says"""
    for request in (UNSET, NEVER, WHEREVER):
        for G in (16, 4096):
            in_force, _, served = rule(exe, request, evaluator=evaluator, G=G, plain=plain, shape=shape, profiled=profiled)
            assert (in_force, served) == (False, False), (request, G)


def test_unserved_modes_leave_the_family_the_form_is_launched_from(exe):
    family = lambda **kw: run(exe, "family", *[kw.get(k, d) for k, d in (("cap", 0), ("forced", 0), ("exact", 0), ("proof", 0), ("puct", 0), ("gm", 0), ("K", 1))])[0]  # noqa: E731
    assert family() == "k_step"
    for kw in ({"cap": 1}, {"forced": 1}, {"cap": 1, "forced": 1}, {"exact": 6}, {"proof": 1}, {"proof": 1, "exact": 6}, {"puct": 1}, {"gm": 4}, {"K": 2},
               {"gm": 4, "K": 2}):
        assert family(**kw) != "k_step", kw


def test_header_binding_and_sources_name_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_net_forward_lane_fc2\(az_net \*net, int lane, int beside, const float \*d_input, const int32_t \*d_count, int max_B, void \*stream\);", hdr)
    assert re.search(r"int az_net_heads_view\(az_net \*net, int lane, const float \*\*d_h2, const float \*\*d_hwq, const float \*\*d_hb, int32_t \*NH, int32_t \*F2\);", hdr)
    assert re.search(r"int az_engine_step_heads\(az_engine \*e, int32_t \*in_force, int32_t \*used\);", hdr)
    from alphazero_amd import _lib
    assert {"az_net_forward_lane_fc2", "az_net_heads_view", "az_engine_step_heads"} <= set(_lib.SYMBOLS)
    L = _lib.lib()
    assert L.az_version() >= 117
    assert L.az_net_heads_view(None, 0, None, None, None, None, None) == _lib.AZ_EINVAL
    assert L.az_engine_step_heads(None, None, None) == _lib.AZ_EINVAL
    # the block routine shares the deterministic exp / tanh with k_heads2: it includes them, it does not restate them
    blk = open(os.path.join(ROOT, "alphazero_amd", "csrc", "az_heads_block.h")).read()
    assert '#include "az_device.h"' in blk and "az_det_expf(" in blk and "az_det_tanhf(" in blk
    assert not re.search(r"float\s+az_det_(expf|tanhf)\s*\(", blk)
