"""CPU: the PUCT exploration settings in the search plan (alphazero_amd/csrc/az_search_plan.h: SF_STEP_PUCT, SearchMode.puct,
puct_refusal, the ranges), pinned without a GPU.  tests/search_plan_puct.cpp is compiled with the host C++ compiler and run as a child
process.  What is pinned: the mode's plan is k_step_puct with L = n_sim and L + 1 launches, the lock-steps of the plain search; every
other mode's plan is what it was, whatever the new field says; puct_refusal names each refusing mode; the graph key of a search under
the settings is not the plain search's; the ranges of the three settings and the neutral triple."""
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
    out = str(tmp_path_factory.mktemp("plan_puct") / "search_plan_puct")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero_amd", "csrc"),
                           os.path.join(ROOT, "tests", "search_plan_puct.cpp"), "-o", out])
    return out


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.strip().split("\n")


def refusal(exe, evaluator=NET, sym=0, symr=0, leaf_batch=1, gm=0, cap=0, forced=0, exact=0, proof=0):
    return run(exe, "refusal", evaluator, sym, symr, leaf_batch, gm, cap, forced, exact, proof)[0]


def plan(exe, puct=0, proof=0, exact=0, cap=0, forced=0, gm=0, K=1, rollout=0, n_sim=5):
    return run(exe, "plan", puct, proof, exact, cap, forced, gm, K, rollout, n_sim)


def test_served_in_the_plain_search_of_net_and_fake_engines(exe):
    assert refusal(exe, NET) == "served" and refusal(exe, FAKE) == "served"


@pytest.mark.parametrize("kw,name", [
    (dict(evaluator=EXTERNAL), "AZ_EVAL_EXTERNAL"), (dict(evaluator=ROLLOUT), "AZ_EVAL_ROLLOUT"),
    (dict(sym=1), "az_engine_set_symmetry)"), (dict(symr=1), "az_engine_set_symmetry_random"),
    (dict(leaf_batch=2), "leaf_batch > 1"), (dict(leaf_batch=16), "leaf_batch > 1"), (dict(gm=1), "Gumbel"), (dict(gm=16), "Gumbel"),
    (dict(cap=1), "playout cap"), (dict(forced=1), "forced playouts"),
    (dict(exact=1), "exact endgames (az_engine_set_exact_endgame)"), (dict(exact=10), "exact endgames"),
    (dict(proof=1), "proof backup (az_engine_set_proof_backup)")])
def test_every_refusal_names_its_mode(exe, kw, name):
    for evaluator in ((NET, FAKE) if "evaluator" not in kw else (kw["evaluator"],)):
        why = refusal(exe, **{**kw, "evaluator": evaluator})
        assert why != "served" and name in why, why


@pytest.mark.parametrize("n_sim", [1, 5, 100])
def test_the_family_and_its_launch_sequence(exe, n_sim):
    plain, puct = plan(exe, n_sim=n_sim), plan(exe, puct=1, n_sim=n_sim)
    assert plain[0] == f"k_step {n_sim} {n_sim + 1} 1 0" and puct[0] == f"k_step_puct {n_sim} {n_sim + 1} 1 0"
    assert len(puct) == 1 + n_sim + 1 and plain[1:] == puct[1:]  # the same lock-steps: (backup, select, t, counter) per launch
    assert puct[1] == "0 1 0 0" and puct[-1] == f"1 0 {n_sim} {n_sim & 1}"


# (keywords, the first line of the plan at n_sim = 8) of every other mode: what it was, with the new field clear and, for the modes the
# setters never let stand beside it, set
OTHERS = [(dict(rollout=1), "k_rollout_step 0 8 0 0"), (dict(K=4), "k_step_multi 2 3 1 0"), (dict(gm=4), "k_step_gumbel 8 9 1 0"),
          (dict(gm=4, K=2), None), (dict(cap=1), "k_step_cap 8 9 1 0"), (dict(forced=1), "k_step_forced 8 9 1 0"),
          (dict(cap=1, forced=1), "k_step_cap_forced 8 9 1 0"), (dict(exact=6), "k_step_exact 8 9 1 0"),
          (dict(proof=1), "k_step_proof 8 9 1 0"), (dict(proof=1, exact=6), "k_step_proof 8 9 1 1")]


@pytest.mark.parametrize("kw,first", OTHERS)
def test_every_other_modes_plan_is_what_it_was(exe, kw, first):
    off, on = plan(exe, n_sim=8, **kw), plan(exe, puct=1, n_sim=8, **kw)
    assert off == on
    if first is not None:
        assert off[0] == first
    else:
        assert off[0].startswith("k_step_gumbel_multi ")


def test_the_graph_key_is_its_own(exe):
    assert run(exe, "keycmp", 1, 0, 24, 512, 0, 512) == ["!="]
    assert run(exe, "keycmp", 1, 1, 24, 512, 0, 512) == ["=="]  # the settings are launch arguments: a change drops every graph instead
    assert run(exe, "keycmp", 0, 0, 24, 512, 0, 512) == ["=="]


@pytest.mark.parametrize("triple,want", [
    ((1.0, 0, -1), "1 1 1 1"), ((1.0, 0, -0.5), "1 1 1 1"), ((1.25, 19652, 0.25), "1 1 1 0"), ((1.0, 0, 0), "1 1 1 0"),
    ((64, 1, 4), "1 1 1 0"), ((64.5, 0.5, 4.5), "0 0 0 0"), ((0, 1e9, 0), "0 1 1 0"), ((1, 2e9, -7), "1 0 1 0"),
    (("nan", "nan", "nan"), "0 0 0 0"), (("inf", "inf", "inf"), "0 0 0 0"), ((-1, -1, "-inf"), "0 0 1 0")])
def test_the_ranges_and_the_neutral_triple(exe, triple, want):
    assert run(exe, "ranges", *triple) == [want]
