"""GPU: resignation in the self-play wave (k_move, k_resign_value; az_engine_set_resign).

  1. whole az_engine_run waves are the host model's (tests/resign_model.py) bit for bit: the samples with z, the counters, every log
     row and low as float64 -- three boards, both tie modes, windows of one and of two values, resigned games, holdout games with
     and without a trigger, false positives;
  2. the same games under 1, 2 and 4 slot groups: samples, log and counters;
  3. with the playout cap: the wave is the composed model's, a fast ply is untested and leaves the window alone;
  4. record-only (p_holdout = 1.0) keeps the samples, array by array and unsorted, in the plain search and under leaf_batch 4, the
     Gumbel search, exact endgames with proof backup, and the cap; every log row is consistent with itself;
  5. on the HIP network with production noise, p_holdout = 0: a resigned game is a prefix of its mode-off twin with z of the
     resignation, every other game is its twin;
  6. resign_values() after set_roots + search is az_resign_value of the root's N and Q, NaN for a slot without a game;
  7. on, off, run is an untouched engine, graph replays included; advance() never resigns and leaves the log empty;
  8. every refusal: the ranges, an open search;
  9. one trainer iteration with calibrate: the next threshold is resign.calibrate of that wave's log.
"""
import math

import numpy as np
import pytest
import torch

import playout_cap_model as PM
import resign_model as M
from alphazero_amd import _lib
from alphazero_amd import engine as E
from alphazero_amd import resign as R
from alphazero_amd.games.othello import OthelloNet
from leaf_batch_model import make_board
from tools import closed_form as cf

pytestmark = pytest.mark.gpu

GAMES = {"othello6": ("othello", 0, 6, 6), "connect4": ("connect4", 1, 6, 7), "tictactoe": ("tictactoe", 2, 3, 3)}
N_SIM, CAP, NOISE, TMAX, TMIN = 12, (4, 0.4), (0.03, 0.25), 2, 7  # temperatures 1, 0.8, 0.6, 0.4, 0.2, 0 over plies 2 .. 7
SEED, FIRST, N_GAMES, N_SLOTS = 11, 1000, 28, 20
SETTINGS = {"A": (-0.05, 1, 4, 0.5), "B": (-0.05, 2, 4, 0.5)}  # (v_resign, consecutive, min_ply, p_holdout)
TIES = {"lowest": E.TIE_LOWEST, "random": E.TIE_RANDOM}
KEYS = ("state", "pi", "visits", "z", "meta")
COUNTERS = ("resigned", "holdout_games", "holdout_triggered", "holdout_false_positives")
CASES = [(tag, tie, "A") for tag in GAMES for tie in TIES] + [("othello6", tie, "B") for tie in TIES]
_CACHE = {}


def spec(setting):
    return dict(zip(("threshold", "consecutive", "min_ply", "holdout"), setting))


def model_wave(tag, tie, setting, cap=None, n_games=N_GAMES):
    key = (tag, tie, setting, cap, n_games)
    if key not in _CACHE:
        game, _, H, W = GAMES[tag]
        _CACHE[key] = M.play_wave(game, H, W, SEED, FIRST, n_games, N_SIM, SETTINGS[setting], cap, NOISE, tie, TMAX, TMIN)
    return _CACHE[key]


def fake_engine(tag, tie, n_slots, **kw):
    _, gid, H, W = GAMES[tag]
    return E.SelfPlayEngine(gid, H, W, n_slots=n_slots, n_sim=N_SIM, evaluator=E.EVAL_FAKE, tie_mode=TIES[tie], noise_mode=E.NOISE_HASH,
                            dirichlet_alpha=NOISE[0], dirichlet_epsilon=NOISE[1], temp_max_step=TMAX, temp_min_step=TMIN, seed=SEED,
                            node_capacity=8192, **kw)


def ordered(smp):
    """samples as numpy arrays sorted by (game id, move idx)"""
    a = {k: v.cpu().numpy() for k, v in smp.items()}
    order = np.lexsort((a["meta"][:, 1], a["meta"][:, 0]))
    return {k: v[order] for k, v in a.items()}


def same_rows(got, want, what, keys=KEYS):
    for k in keys:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (what, k)


def log_of(eng):
    log = eng.game_log()
    rows, low = log["rows"].cpu().numpy(), log["low"].cpu().numpy()
    for i, k in enumerate(E.SelfPlayEngine.GAME_LOG_COLUMNS):
        assert np.array_equal(log[k].cpu().numpy(), rows[:, i]), k
    assert rows.dtype == np.int32 and low.dtype == np.float64
    return rows, low


def same_log(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "rows", got[0][(got[0] != want[0]).any(axis=1)], want[0][(got[0] != want[0]).any(axis=1)])
    assert got[1].shape == want[1].shape and np.array_equal(got[1].view(np.int64), want[1].view(np.int64)), (what, "low")


def consistent(rows, low, thr):
    """each log row against itself: a trigger exists iff the trigger player's low is below the threshold -- and no side's otherwise"""
    for row, lo in zip(rows, low):
        if row[5] >= 0:
            assert row[6] in (1, -1) and lo[0 if row[6] == 1 else 1] < thr, row
        else:
            assert row[6] == 0 and not (lo < thr).any(), (row, lo)
        assert row[3] in (0, 1) and row[4] in (0, 1) and row[7] == 0 and row[2] in (-1, 0, 1) and row[1] > 0
        if row[3]:
            assert not row[4] and row[1] == row[5] + 1 and row[2] == -row[6], row


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("tag,tie,setting", CASES)
def test_a_wave_is_the_host_models(tag, tie, setting):
    want, ctr, rows, low = model_wave(tag, tie, setting)
    assert ctr["resigned"] >= 1 and ctr["holdout_triggered"] >= 1, ctr  # from the model alone: neither branch goes untested
    eng = fake_engine(tag, tie, N_SLOTS)  # 20 slots: a full block and a ragged one; 28 games: slots are refilled, after resignations too
    eng.set_resign(spec(SETTINGS[setting]))
    got = ordered(eng.run(N_GAMES, first_game_id=FIRST))
    same_rows(got, want, (tag, tie, setting))
    st, rs = eng.stats(), eng.resign_stats()
    assert rs == {k: ctr[k] for k in COUNTERS}
    assert (st["samples"], st["plies"], st["games_done"], st["net_evals"]) == (ctr["samples"], ctr["plies"], N_GAMES, ctr["rows"])
    assert st["error_flags"] == 0 and st["graph_replays"] > 0
    got_log = log_of(eng)
    same_log(got_log, (rows, low), (tag, tie, setting))
    consistent(got_log[0], got_log[1], SETTINGS[setting][0])
    eng.close()


def test_the_cases_cover_false_positives_and_games_without_a_trigger():
    """over all cases of test 1, from the model's own output"""
    fp = sum(model_wave(*c)[1]["holdout_false_positives"] for c in CASES)
    quiet = sum(int((model_wave(*c)[2][:, 5] < 0).sum()) for c in CASES)
    assert fp >= 1 and quiet >= 1, (fp, quiet)
    for c in CASES:
        rows = model_wave(*c)[2]
        assert 0 < rows[:, 4].sum() < N_GAMES, c  # holdout and other games in every case


# ------------------------------------------------------------------------------------------------------------------ 2
def test_slot_groups_play_the_same_games():
    n_games = 56
    outs = []
    for n in (1, 2, 4):
        eng = fake_engine("othello6", "random", 48)  # three blocks: groups of 48 | 32 + 16 | 16 + 16 + 16 + 0
        eng.set_resign(spec(SETTINGS["A"]))
        eng.set_groups(n)
        assert eng.groups() == n
        got = ordered(eng.run(n_games, first_game_id=FIRST))
        st, rs = eng.stats(), eng.resign_stats()
        assert st["error_flags"] == 0 and st["games_done"] == n_games
        outs.append((got, {k: st[k] for k in ("samples", "plies", "net_evals", "games_done")}, rs, log_of(eng)))
        eng.close()
    for got, st, rs, log in outs[1:]:
        same_rows(got, outs[0][0], "groups")
        assert st == outs[0][1] and rs == outs[0][2]
        same_log(log, outs[0][3], "groups")
    got, st, rs, log = outs[0]
    assert rs["resigned"] > 0 and rs["holdout_triggered"] > 0 and list(log[0][:, 0]) == list(range(FIRST, FIRST + n_games))
    # the first 28 of these games are the wave of test 1: a game depends on (seed, game id, the settings) only
    want, _, rows, low = model_wave("othello6", "random", "A")
    first = got["meta"][:, 0] < FIRST + N_GAMES
    same_rows({k: v[first] for k, v in got.items()}, want, "groups against the model")
    same_log((log[0][:N_GAMES], log[1][:N_GAMES]), (rows, low), "groups against the model")


# ------------------------------------------------------------------------------------------------------------------ 3
def test_with_the_playout_cap_a_fast_ply_is_untested():
    want, ctr, rows, low = model_wave("othello6", "random", "A", cap=CAP)
    plain = model_wave("othello6", "random", "A")
    assert ctr["fast_plies"] > 0 and ctr["resigned"] >= 1 and ctr["holdout_triggered"] >= 1, ctr
    assert not np.array_equal(rows, plain[2])  # the cap changes the games: the composed model is another wave
    eng = fake_engine("othello6", "random", N_SLOTS)
    eng.set_playout_cap(CAP)
    eng.set_resign(spec(SETTINGS["A"]))
    got = ordered(eng.run(N_GAMES, first_game_id=FIRST))
    same_rows(got, want, "cap")
    st, cs = eng.stats(), eng.playout_cap_stats()
    assert eng.resign_stats() == {k: ctr[k] for k in COUNTERS}
    assert cs == {"full_plies": ctr["full_plies"], "fast_plies": ctr["fast_plies"]}
    assert st["samples"] == cs["full_plies"] == ctr["samples"] and st["plies"] == cs["full_plies"] + cs["fast_plies"] == ctr["plies"]
    assert st["net_evals"] == ctr["rows"] and st["error_flags"] == 0
    got_log = log_of(eng)
    same_log(got_log, (rows, low), "cap")
    # a trigger sits on a full ply: a fast one is untested
    for row in got_log[0]:
        if row[5] >= 0:
            assert PM.coin_full(SEED, int(row[0]), int(row[5]), CAP[1]), row
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4
MODES = {"plain": lambda e: None, "leaf_batch": lambda e: e.set_leaf_batch(4), "gumbel": lambda e: e.set_gumbel(8),
         "exact_proof": lambda e: (e.set_exact_endgame(6), e.set_proof_backup(True)), "cap": lambda e: e.set_playout_cap(CAP)}


@pytest.mark.parametrize("mode", list(MODES))
def test_record_only_keeps_the_samples(mode):
    thr = -0.05
    outs = []
    for on in (False, True):
        eng = fake_engine("othello6", "random", N_SLOTS)
        MODES[mode](eng)
        if on:
            eng.set_resign({"threshold": thr, "consecutive": 2, "min_ply": 4, "holdout": 1.0})
        got = {k: v.cpu().numpy() for k, v in eng.run(N_GAMES, first_game_id=FIRST).items()}  # unsorted: the same launches, the same order
        st, rs = eng.stats(), eng.resign_stats()
        assert st["error_flags"] == 0 and st["games_done"] == N_GAMES
        if on:
            rows, low = log_of(eng)
            assert rs["resigned"] == 0 and rs["holdout_games"] == N_GAMES and rs["holdout_triggered"] == int((rows[:, 5] >= 0).sum()) > 0
            assert list(rows[:, 0]) == list(range(FIRST, FIRST + N_GAMES)) and not rows[:, 3].any() and rows[:, 4].all()
            consistent(rows, low, thr)
            # the log against the samples: the winner is z * player of any sample, the game is at least as long as its last sample
            for row in rows:
                mine = got["meta"][:, 0] == row[0]
                assert mine.any() and np.all(got["z"][mine] * got["meta"][mine][:, 2] == row[2]) and got["meta"][mine][:, 1].max() < row[1]
        else:
            assert rs == dict.fromkeys(COUNTERS, 0) and eng.game_log()["rows"].shape == (0, 8) and eng.game_log()["low"].shape == (0, 2)
        outs.append((got, st))
        eng.close()
    same_rows(outs[1][0], outs[0][0], mode)
    for k in ("samples", "plies", "net_evals", "lockstep_iters", "graph_replays", "games_done", "max_nodes_used"):
        assert outs[1][1][k] == outs[0][1][k], (mode, k)


# ------------------------------------------------------------------------------------------------------------------ 5
def othello6_net():
    if "net" not in _CACHE:
        net = OthelloNet(6, device="cuda")
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.tensor(v) for k, v in cf.closed_form_state_dict(shapes).items()})
        net.eval()
        _CACHE["net"] = net.to_hip(max_batch=64)
    return _CACHE["net"]


def net_run(resign, n_games=32, seed=23):
    """32 games on 20 slots of a production engine (Philox Dirichlet noise, random ties, the HIP network)"""
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=20, n_sim=N_SIM, net=othello6_net(), seed=seed, node_capacity=8192)
    if resign is not None:
        eng.set_resign(resign)
    got = ordered(eng.run(n_games, first_game_id=50))
    st, rs = eng.stats(), eng.resign_stats()
    log = log_of(eng) if resign is not None else None
    assert st["error_flags"] == 0 and st["games_done"] == n_games
    eng.close()
    return got, st, rs, log


def test_production_noise_on_the_network():
    off, st_off, rs_off, _ = net_run(None)
    assert rs_off == dict.fromkeys(COUNTERS, 0)
    # the threshold is an input: a record-only wave gives every game's low, and their median makes about half of the games resign
    rec, _, rs_rec, (rows_rec, low_rec) = net_run({"threshold": -0.05, "consecutive": 1, "min_ply": 4, "holdout": 1.0})
    same_rows(rec, off, "record-only")
    assert rs_rec["resigned"] == 0 and rs_rec["holdout_games"] == 32
    thr = float(np.median(low_rec.min(axis=1)))
    assert -1.0 <= thr < 0.0
    on, st, rs, (rows, low) = net_run({"threshold": thr, "consecutive": 1, "min_ply": 4, "holdout": 0.0})
    print("threshold", thr, rs, "plies", st["plies"], "of", st_off["plies"])
    assert rs["holdout_games"] == rs["holdout_triggered"] == rs["holdout_false_positives"] == 0 and not rows[:, 4].any()
    assert 0 < rs["resigned"] == int(rows[:, 3].sum()) < 32 and st["plies"] < st_off["plies"] and st["samples"] == st["plies"] == int(rows[:, 1].sum())
    assert np.array_equal(rows[:, 3] == 1, low_rec.min(axis=1) < thr)  # a side triggers at a threshold t exactly when its low < t
    consistent(rows, low, thr)
    for row in rows:
        mine, twin = on["meta"][:, 0] == row[0], off["meta"][:, 0] == row[0]
        n = int(mine.sum())
        assert n == row[1]
        if row[3]:  # a prefix of the mode-off game, bit for bit but for z: the mover of the trigger ply lost
            assert n <= int(twin.sum()) and row[5] >= 4
            same_rows({k: on[k][mine] for k in KEYS}, {k: off[k][twin][:n] for k in KEYS}, ("prefix", int(row[0])), keys=("state", "pi", "visits", "meta"))
            assert np.array_equal(on["z"][mine], (-row[6] * on["meta"][mine][:, 2]).astype(np.int8)), row
            assert on["meta"][mine][-1, 2] == row[6]  # the last recorded ply is the one the resigning side moved on
        else:
            assert row[5] < 0
            same_rows({k: on[k][mine] for k in KEYS}, {k: off[k][twin] for k in KEYS}, ("twin", int(row[0])))


# ------------------------------------------------------------------------------------------------------------------ 6
def _roots(n):
    """Othello 6x6 positions after 0 .. n - 1 seeded random moves, each at its own ply"""
    rng, out = np.random.default_rng(4), []
    for plies in range(n):
        b = make_board("othello", 6, 6)
        for _ in range(plies):
            moves = sorted(b.get_moves(), key=lambda m: cf.move_to_action("othello", m, 6))
            b.play_move(moves[int(rng.integers(len(moves)))])
        assert not b.is_game_over()
        out.append(b)
    return out


@pytest.mark.parametrize("mode_on", [False, True])
def test_resign_values_are_the_host_arithmetic_of_the_readout(mode_on):
    roots = _roots(7)
    eng = fake_engine("othello6", "random", 10)  # slots 7 .. 9 hold no game
    if mode_on:
        eng.set_resign(spec(SETTINGS["A"]))
    eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8),
                  game_ids=(300 + np.arange(7)).astype(np.uint32), plies=np.arange(7).astype(np.int32))
    v = eng.resign_values()
    assert v.dtype == torch.float64 and v.shape == (10,) and bool(torch.isnan(v).all())  # no root is expanded yet
    for n in (1, N_SIM):  # after one simulation a root has one visited child; then a searched root
        eng.search(n)
        v = eng.resign_values().cpu().numpy()
        ro = {k: t.cpu().numpy() for k, t in eng.root_readout().items()}
        for s in range(7):
            held = ro["child"][s].astype(bool)  # the children in child order: ascending actions
            a, N, Q, _, _ = eng.root_children(s)
            assert list(a) == list(np.nonzero(held)[0]) and list(N) == list(ro["visits"][s][held])
            want = E.SelfPlayEngine.resign_value(ro["visits"][s][held], ro["Q"][s][held])
            model = M.value(N, Q)
            if model is None:  # no child visited yet
                assert n == 1 and math.isnan(want) and math.isnan(v[s]), (n, s, v[s], want)
                continue
            assert np.array([v[s]]).view(np.int64)[0] == np.array([want]).view(np.int64)[0], (n, s, v[s], want)
            assert np.array([want]).view(np.int64)[0] == np.array([model]).view(np.int64)[0]
        assert np.isnan(v[7:]).all()
    assert eng.resign_stats() == dict.fromkeys(COUNTERS, 0) and eng.stats()["error_flags"] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 7
def test_off_is_off():
    outs = []
    for detour in (False, True):
        eng = fake_engine("othello6", "random", N_SLOTS)
        if detour:
            eng.set_resign(spec(SETTINGS["A"]))
            eng.set_resign(spec(SETTINGS["A"]))  # the same setting again: nothing to do
            eng.set_resign(spec(SETTINGS["B"]))
            eng.set_resign(None)
            eng.set_resign(None)
        got = {k: v.cpu().numpy() for k, v in eng.run(N_GAMES, first_game_id=FIRST).items()}  # unsorted: the same launches, the same order
        st = eng.stats()
        assert eng.resign_stats() == dict.fromkeys(COUNTERS, 0) and st["samples"] == st["plies"] and eng.game_log()["rows"].shape[0] == 0
        outs.append((got, st))
        eng.close()
    same_rows(outs[1][0], outs[0][0], "on, off, run")
    for k in ("samples", "plies", "net_evals", "lockstep_iters", "graph_replays", "games_done", "max_nodes_used"):
        assert outs[1][1][k] == outs[0][1][k], k
    assert outs[0][1]["graph_replays"] > 0


def test_a_run_with_the_mode_off_empties_the_log():
    eng = fake_engine("tictactoe", "random", 8, sample_capacity=30 * 9)
    eng.set_resign(spec(SETTINGS["A"]))
    eng.run(12, first_game_id=FIRST)
    assert eng.game_log()["rows"].shape == (12, 8)
    eng.run(30, first_game_id=FIRST)  # more games than before: the log grows
    rows, low = log_of(eng)
    assert list(rows[:, 0]) == list(range(FIRST, FIRST + 30)) and eng.resign_stats()["resigned"] == int(rows[:, 3].sum())
    eng.set_resign(None)
    eng.run(12, first_game_id=FIRST)
    assert eng.game_log()["rows"].shape == (0, 8) and eng.resign_stats() == dict.fromkeys(COUNTERS, 0)
    eng.close()


def test_advance_never_resigns():
    roots = _roots(10)
    eng = fake_engine("othello6", "random", 10)
    # every tested value below 0 would trigger, from ply 0 on, in no holdout game
    eng.set_resign({"threshold": R.BELOW_ZERO, "consecutive": 1, "min_ply": 0, "holdout": 0.0})
    eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8),
                  game_ids=(300 + np.arange(10)).astype(np.uint32), plies=np.arange(10).astype(np.int32))
    for _ in range(3):
        eng.search(N_SIM)
        v = eng.resign_values().cpu().numpy()
        assert (v < 0.0).any()  # az_engine_run would resign these slots' games here
        eng.advance()
    st = eng.stats()
    assert st["plies"] == 30 and st["games_done"] == 0 and st["error_flags"] == 0  # every slot still holds its game
    assert eng.resign_stats() == dict.fromkeys(COUNTERS, 0) and eng.game_log()["rows"].shape == (0, 8)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 8
def test_refusals():
    eng = fake_engine("othello6", "random", 4)
    L, nan = _lib.lib(), float("nan")
    for bad in ((0.0, 1, 0, 0.1), (0.5, 1, 0, 0.1), (-1.01, 1, 0, 0.1), (float("-inf"), 1, 0, 0.1), (-0.5, 0, 0, 0.1), (-0.5, 5, 0, 0.1),
                (-0.5, -1, 0, 0.1), (-0.5, 1, -1, 0.1), (-0.5, 1, 0, -0.01), (-0.5, 1, 0, 1.01), (-0.5, 1, 0, nan)):
        assert L.az_engine_set_resign(eng.h, *bad) == _lib.AZ_EINVAL, bad
    assert eng.resign_stats() == dict.fromkeys(COUNTERS, 0)
    with pytest.raises(ValueError, match=r"az_engine_set_resign: v_resign must be in \[-1, 0\)"):
        _lib.check(L.az_engine_set_resign(eng.h, 0.25, 1, 0, 0.1))
    with pytest.raises(ValueError, match=r"az_engine_set_resign: consecutive must be in \[1, 4\]"):
        _lib.check(L.az_engine_set_resign(eng.h, -0.5, 7, 0, 0.1))
    with pytest.raises(ValueError, match=r"az_engine_set_resign: min_ply must be >= 0"):
        _lib.check(L.az_engine_set_resign(eng.h, -0.5, 1, -3, 0.1))
    with pytest.raises(ValueError, match=r"az_engine_set_resign: p_holdout must be in \[0, 1\]"):
        _lib.check(L.az_engine_set_resign(eng.h, -0.5, 1, 0, 2.0))
    assert L.az_engine_set_resign(eng.h, nan, 99, -5, nan) == _lib.AZ_OK  # off: the other three are not looked at
    for ok in ((-1.0, 1, 0, 0.0), (R.BELOW_ZERO, 4, 1000, 1.0)):  # the ends of every range
        assert L.az_engine_set_resign(eng.h, *ok) == _lib.AZ_OK, ok
    b = make_board("othello", 6, 6)
    eng.set_roots(np.tile(b.grid.astype(np.int8)[None], (4, 1, 1)), np.full(4, b.player, np.int8))
    eng.search_begin(4)
    for r in (spec(SETTINGS["A"]), None):
        with pytest.raises(_lib.AzError, match=r"\[-3\] az_engine_set_resign: a search begun"):
            eng.set_resign(r)
    with pytest.raises(_lib.AzError, match=r"\[-3\] az_engine_resign_stats"):
        eng.resign_stats()
    with pytest.raises(_lib.AzError, match=r"\[-3\] az_engine_game_log"):
        eng.game_log()
    with pytest.raises(_lib.AzError, match=r"\[-3\] az_engine_resign_values"):
        eng.resign_values()
    eng.search_end()
    eng.set_resign(None)
    assert eng.stats()["error_flags"] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 9
def test_one_trainer_iteration_with_calibrate(tmp_path):
    from alphazero_amd import base
    from alphazero_amd.games.othello import OthelloConfig
    from alphazero_amd.trainer import AlphaZeroTrainer
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    option = {"threshold": -0.05, "consecutive": 1, "min_ply": 4, "holdout": 0.5, "calibrate": 0.1}
    tr = AlphaZeroTrainer(verbose=False, engine_slots=16, seed=6, materialize_memory=False)
    tr.selfplay_resign = option  # assigned after construction: checked again, and its threshold taken, before the engine is built
    assert tr.resign_threshold is None
    tr.game = "othello"
    tr.config = OthelloConfig(board_size=6, simulations=8, episodes=16, epochs=1, batch_size=16, iterations=1, do_eval=False, device="cuda")
    torch.manual_seed(3)
    tr.setup()
    tr.self_play(0)
    eng = tr._engine
    rows, low = log_of(eng)
    assert rows.shape == (16, 8) and list(rows[:, 0]) == list(range(16)) and 0 < rows[:, 4].sum() < 16
    want = R.calibrate(low, rows[:, 2], 0.1, -0.05, holdout=rows[:, 4])
    sides = np.concatenate([low[(rows[:, 4] == 1) & (rows[:, 2] >= 0), 0], low[(rows[:, 4] == 1) & (rows[:, 2] <= 0), 1]])
    assert -1.0 <= want < 0.0 and int((sides < want).sum()) <= math.floor(0.1 * len(sides))
    st = tr.resign_stats[0]
    assert tr.resign_threshold == want == st["next_threshold"] and st["threshold"] == -0.05 and st["games"] == 16
    assert {k: st[k] for k in COUNTERS} == eng.resign_stats() and st["resigned"] == int(rows[:, 3].sum())
    assert len(tr.device_samples["z"]) == eng.stats()["samples"] == int(rows[:, 1].sum())
    assert tr._ensure_engine() is eng and eng._resign == {"threshold": want, "consecutive": 1, "min_ply": 4, "holdout": 0.5}  # the next wave's
