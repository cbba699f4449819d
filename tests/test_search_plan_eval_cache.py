"""CPU: the leaf evaluation cache's measured rule and key arithmetic (alphazero_amd/csrc/az_search_plan.h: eval_cache_*, ec_*), pinned
without a GPU.  tests/eval_cache_table.cpp is compiled with the host C++ compiler and run as a child process.  What is pinned: where the
cache is served and what every request answers there, the rule's shapes, the setter's argument checks, that equal keys give equal
buckets inside the table, the stone limit, the stamp's order, the row encoding, and a host model of one group's table whose every hit is
checked against a plain map."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
AUTO, OFF, ON = -1, 0, 1
NET, FAKE, ROLLOUT, EXTERNAL = 0, 1, 2, 3
OTHELLO, CONNECT4, TICTACTOE = 0, 1, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert CXX, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("eval_cache") / "eval_cache_table")
    subprocess.check_call([CXX, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "alphazero_amd", "csrc"),
                           os.path.join(ROOT, "tests", "eval_cache_table.cpp"), "-o", out])
    return out


def run(exe, *args):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, check=True).stdout.split()


def rule(exe, request, evaluator=NET, game=OTHELLO, H=8, W=8, G=4096, beyond=0, profiled=0):
    in_force, auto, served = map(int, run(exe, "rule", request, evaluator, game, H, W, G, beyond, profiled))
    return bool(in_force), bool(auto), bool(served)


def test_the_rule_serves_the_measured_shapes_only(exe):
    for G, on in ((16, False), (511, False), (512, True), (2112, True), (4096, True), (8192, True), (32768, True)):
        assert rule(exe, AUTO, G=G) == (on, on, True), G
    for G, on in ((512, False), (4096, False), (8191, False), (8192, True), (32768, True)):
        assert rule(exe, AUTO, game=CONNECT4, H=6, W=7, G=G) == (on, on, True), G
    for game, H, W in ((OTHELLO, 6, 6), (OTHELLO, 4, 4), (CONNECT4, 7, 7), (TICTACTOE, 3, 3)):
        for G in (512, 4096, 8192, 32768):
            assert rule(exe, AUTO, game=game, H=H, W=W, G=G) == (False, False, True), (game, H, G)


def test_requests_where_the_cache_is_served(exe):
    for G in (16, 4096):
        assert rule(exe, ON, G=G)[0] is True
        assert rule(exe, OFF, G=G)[0] is False
    assert rule(exe, ON, game=CONNECT4, H=6, W=7, G=64)[0] is True  # on wherever served: every game's plain search


@pytest.mark.parametrize("evaluator,beyond,profiled", [(FAKE, 0, 0), (ROLLOUT, 1, 0), (EXTERNAL, 1, 0), (NET, 1, 0), (NET, 0, 1), (NET, 1, 1)])
def test_refusals(exe, evaluator, beyond, profiled):
    """the fake / rollout / external evaluators, a mode beyond the plain search (symmetry, leaf_batch > 1, Gumbel) and a net under
    az_net_profile: off whatever is asked for"""
    for request in (AUTO, OFF, ON):
        in_force, _, served = rule(exe, request, evaluator=evaluator, beyond=beyond, profiled=profiled)
        assert (in_force, served) == (False, False), request


def test_setter_arguments(exe):
    ok = lambda c, l: tuple(map(int, run(exe, "args", c, l)))  # noqa: E731
    for c in (0, 1, 2, 8, 1 << 18, 1 << 22):
        assert ok(c, 0) == (1, 1), c
    for c in (-1, 3, 12, (1 << 18) + 1, 1 << 23):
        assert ok(c, 0)[0] == 0, c
    for lim, good in ((0, 1), (1, 1), (12, 1), (64, 1), (65, 0), (-1, 0)):
        assert ok(0, lim)[1] == good, lim


def test_equal_keys_give_equal_buckets_inside_the_table(exe):
    start = ("0000001008000000", "0000000810000000")  # Othello's opening: four stones
    seen = set()
    for cap in (1, 8, 1 << 18):
        for p1, m1 in (start, start[::-1], ("ff", "ff00")):
            for player in (1, -1):
                a = run(exe, "key", p1, m1, player, cap, 12)
                assert a == run(exe, "key", p1, m1, player, cap, 12)
                h, buckets = int(a[0]), list(map(int, a[1:5]))
                assert all(0 <= b < cap for b in buckets)
                assert buckets == [(h + j) % cap for j in range(4)]
                if cap == 1 << 18:
                    seen.add(h)
    assert len(seen) == 6  # the side to move and the colours are part of the key's hash


def test_the_stone_limit(exe):
    in_limit = lambda p1, m1, lim: int(run(exe, "key", p1, m1, 1, 8, lim)[5])  # noqa: E731
    assert in_limit("0000001008000000", "0000000810000000", 4) == 1
    assert in_limit("0000001008000000", "0000000810000000", 3) == 0
    assert in_limit("fff", "1000", 12) == 0 and in_limit("fff", "1000", 13) == 1
    assert in_limit("ffffffff00000000", "00000000ffffffff", 64) == 1 and in_limit("ffffffff00000000", "00000000ffffffff", 63) == 0


def test_stamps_grow_along_a_stream_and_tags_are_never_empty(exe):
    tag = lambda h, serial, sim: run(exe, "tag", h, serial, sim)  # noqa: E731
    serial, last = 0, 0
    for _ply in range(3):
        for sim in range(0, 5):  # n_sim = 4: kernels sim 0 .. 4, the last one the ply's closing backup
            stamp = int(tag(0, serial, sim)[0])
            assert stamp > last
            last = stamp
        serial = last  # the closing backup stores its own stamp
    for h in (0, 1, 0xFFFFFFFF):
        stamp, word, s2, h2 = tag(h, 0, 0)
        assert int(stamp) == 1 and int(word, 16) != 0 and int(s2) == 1 and int(h2) == h


def test_the_row_encoding_round_trips(exe):
    for entry in (0, 1, 7, (1 << 22) - 1):
        row, is_entry, back = map(int, run(exe, "row", entry))
        assert row < 0 and is_entry == 1 and back == entry
    assert run(exe, "stride", 65) == ["68"] and run(exe, "stride", 7) == ["8"] and run(exe, "stride", 9) == ["12"]


@pytest.mark.parametrize("capacity,limit", [(1 << 10, 12), (8, 12), (1, 12), (1 << 10, 4), (1 << 10, 64), (2, 64)])
def test_host_model_of_a_table(exe, capacity, limit):
    """a full table, an exhausted probe and every stone limit: hits are exact (the program checks each against a map), a table never
    holds more claims than entries, and nothing is looked up beyond the limit"""
    lookups, hits, claims, no_room, out, small = map(int, run(exe, "play", capacity, limit, 4000, 7))
    assert lookups == 4000 == hits + claims + no_room + out
    assert hits + claims + no_room == small  # exactly the draws of at most `limit` stones reach the table
    assert claims <= capacity
    if limit == 64:
        assert out == 0
    if limit == 4:
        assert 0 < small < lookups  # the pool holds four-stone positions and larger ones
    if capacity >= 1 << 10 and limit >= 12:
        assert hits > 0 and no_room < lookups // 4


def test_header_and_binding_name_the_setter():
    hdr = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_engine_set_eval_cache\(az_engine \*e, int32_t mode, int32_t capacity, int32_t stone_limit\);", hdr)
    assert re.search(r"int az_engine_eval_cache_stats\(az_engine \*e, int32_t \*in_force, int64_t \*hits\);", hdr)
    from alphazero_amd import _lib
    assert {"az_engine_set_eval_cache", "az_engine_eval_cache_stats"} <= set(_lib.SYMBOLS)
