"""CPU: proof backup in the search plan (alphazero_amd/csrc/az_search_plan.h: SF_STEP_PROOF, SearchMode.proof, SearchPlan.exact,
proof_backup_refusal), pinned without a GPU.  tests/search_plan_proof.cpp is compiled with the host C++ compiler and run as a child
process.  What is pinned: where the mode is served and what every refusal answers; that a proof search is ONE family whose exact
variant is a property of the plan (and whose cached variant is, as for every one-leaf family, the chain's); its launch sequence; and
that its graph key differs from a plain and from an exact search's."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
NET, FAKE, ROLLOUT, EXTERNAL = 0, 1, 2, 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("plan_proof") / "search_plan_proof")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero_amd", "csrc"),
                           os.path.join(ROOT, "tests", "search_plan_proof.cpp"), "-o", out])
    return out


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.strip().split("\n")


def refusal(exe, evaluator=NET, sym=0, symr=0, leaf_batch=1, gm=0, cap=0, forced=0):
    return run(exe, "refusal", evaluator, sym, symr, leaf_batch, gm, cap, forced)[0]


def test_served_in_the_plain_search_of_net_and_fake_engines(exe):
    assert refusal(exe, NET) == "served" and refusal(exe, FAKE) == "served"


@pytest.mark.parametrize("kw,name", [
    (dict(evaluator=EXTERNAL), "AZ_EVAL_EXTERNAL"), (dict(evaluator=ROLLOUT), "AZ_EVAL_ROLLOUT"),
    (dict(sym=1), "az_engine_set_symmetry)"), (dict(symr=1), "az_engine_set_symmetry_random"),
    (dict(leaf_batch=2), "leaf_batch > 1"), (dict(leaf_batch=16), "leaf_batch > 1"), (dict(gm=1), "Gumbel"), (dict(gm=16), "Gumbel"),
    (dict(cap=1), "playout cap"), (dict(forced=1), "forced playouts")])
def test_every_refusal_names_its_mode(exe, kw, name):
    for evaluator in ((NET, FAKE) if "evaluator" not in kw else (kw["evaluator"],)):
        why = refusal(exe, **{**kw, "evaluator": evaluator})
        assert why != "served" and name in why, why


def test_the_family_and_its_launch_sequence(exe):
    plain, proof = run(exe, "plan", 0, 0, 0, 0, 0, 1, 5), run(exe, "plan", 1, 0, 0, 0, 0, 1, 5)
    assert plain[0] == "k_step 5 6 1 0" and proof[0] == "k_step_proof 5 6 1 0"
    assert plain[1:] == proof[1:]  # the same lock-steps: (backup, select, t, counter) per launch
    assert proof[1] == "0 1 0 0" and proof[5] == "1 1 4 0" and proof[6] == "1 0 5 1"
    # exact endgames under proof backup: the same family, a property of the plan; without it, the exact family as before
    for e in (1, 6, 10):
        assert run(exe, "plan", 1, e, 0, 0, 0, 1, 8)[0] == "k_step_proof 8 9 1 1"
        assert run(exe, "plan", 0, e, 0, 0, 0, 1, 8)[0] == "k_step_exact 8 9 1 0"
    # the modes it is refused beside keep their own families whatever the field says (the setters never let both be on)
    assert run(exe, "plan", 1, 0, 1, 0, 0, 1, 5)[0].startswith("k_step_cap ")
    assert run(exe, "plan", 1, 0, 0, 1, 0, 1, 5)[0].startswith("k_step_forced ")
    assert run(exe, "plan", 1, 0, 0, 0, 4, 1, 5)[0].startswith("k_step_gumbel ")
    assert run(exe, "plan", 1, 0, 0, 0, 0, 4, 5)[0].startswith("k_step_multi ")


def test_a_proof_plans_graph_key_is_its_own(exe):
    assert run(exe, "keycmp", 1, 0, 0, 0, 24, 512, 0, 512) == ["!="]  # against the plain search
    assert run(exe, "keycmp", 1, 6, 0, 6, 24, 512, 0, 512) == ["!="]  # against the exact search
    assert run(exe, "keycmp", 1, 0, 0, 6, 24, 512, 0, 512) == ["!="]
    assert run(exe, "keycmp", 1, 0, 1, 0, 24, 512, 0, 512) == ["=="]
    assert run(exe, "keycmp", 1, 0, 1, 6, 24, 512, 0, 512) == ["=="]  # the limit is a launch argument: a change drops every graph instead
