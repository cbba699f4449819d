"""GPU: playout cap randomization of the self-play wave (k_step_cap, k_root_prep, k_move; az_engine_set_playout_cap).

  1. whole az_engine_run waves are the host model's (tests/playout_cap_model.py) bit for bit: states, pi, visits, z, meta, samples and
     both counters, on three boards, both tie modes, hash noise, a fractional temperature schedule, a ragged block and slot refill;
  2. the same games under 1, 2 and 4 slot groups: the same rows, the same counters;
  3. set_roots / search / root_readout / advance: the budgets per slot, every search call again, children and node counts the model's;
  4. production noise on the HIP network: p_full = 1.0 is the engine with the mode off, a full ply 0 is the mode-off ply 0, every sample
     is a full ply by the coin and holds n_sim visits on top of what its root inherited;
  5. off is off: on, off, run -- the samples and the graph replays of an engine that never had it on; AZ_ESTATE while a search is open;
  6. every refusal names the mode: the cap's setter in the modes it is not served in, those modes' setters while the cap is on;
  7. one trainer iteration with selfplay_playout_cap: its memory holds the full plies of the engine run with the same seed.
"""
import numpy as np
import pytest
import torch

import playout_cap_model as M
from alphazero_amd import _lib
from alphazero_amd import engine as E
from alphazero_amd.games.othello import OthelloNet
from leaf_batch_model import Model, make_board
from tools import closed_form as cf

pytestmark = pytest.mark.gpu

GAMES = {"othello6": ("othello", 0, 6, 6), "connect4": ("connect4", 1, 6, 7), "tictactoe": ("tictactoe", 2, 3, 3)}
N_SIM, CAP, NOISE, TMAX, TMIN = 12, (4, 0.4), (0.03, 0.25), 2, 7  # temperatures 1, 0.8, 0.6, 0.4, 0.2, 0 over plies 2 .. 7
SEED, FIRST, N_GAMES, N_SLOTS = 11, 1000, 28, 20  # on the model every case plays fast and full plies (Othello 553 / 359 ... TicTacToe 117 / 63)
TIES = {"lowest": E.TIE_LOWEST, "random": E.TIE_RANDOM}
KEYS = ("state", "pi", "visits", "z", "meta")
_CACHE = {}


def model_wave(tag, tie, n_games=N_GAMES):
    key = ("wave", tag, tie, n_games)
    if key not in _CACHE:
        game, _, H, W = GAMES[tag]
        _CACHE[key] = M.play_wave(game, H, W, SEED, FIRST, n_games, N_SIM, CAP, NOISE, tie, TMAX, TMIN)
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


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("tie", ["lowest", "random"])
@pytest.mark.parametrize("tag", ["othello6", "connect4", "tictactoe"])
def test_a_wave_is_the_host_models(tag, tie):
    want, ctr = model_wave(tag, tie)
    assert 0 < ctr["fast_plies"] and 0 < ctr["full_plies"]  # neither branch goes untested
    eng = fake_engine(tag, tie, N_SLOTS)  # 20 slots: a full block and a ragged one; 28 games: 8 slots are refilled
    eng.set_playout_cap(CAP)
    got = ordered(eng.run(N_GAMES, first_game_id=FIRST))
    same_rows(got, want, (tag, tie))
    st, cs = eng.stats(), eng.playout_cap_stats()
    assert cs == {"full_plies": ctr["full_plies"], "fast_plies": ctr["fast_plies"]}
    assert (st["samples"], st["plies"], st["games_done"]) == (ctr["samples"], ctr["plies"], N_GAMES)
    assert st["samples"] == cs["full_plies"] and st["plies"] == cs["full_plies"] + cs["fast_plies"]
    assert st["net_evals"] == ctr["rows"]  # a slot past its budget takes no network row
    assert st["error_flags"] == 0 and st["graph_replays"] > 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 2
def test_slot_groups_play_the_same_games():
    n_games = 56
    outs = []
    for n in (1, 2, 4):
        eng = fake_engine("othello6", "random", 48)  # three blocks: groups of 48 | 32 + 16 | 16 + 16 + 16 + 0
        eng.set_playout_cap(CAP)
        eng.set_groups(n)
        assert eng.groups() == n
        got = ordered(eng.run(n_games, first_game_id=FIRST))
        st, cs = eng.stats(), eng.playout_cap_stats()
        assert st["error_flags"] == 0 and st["games_done"] == n_games
        outs.append((got, {k: st[k] for k in ("samples", "plies", "net_evals", "games_done")}, cs))
        eng.close()
    for got, st, cs in outs[1:]:
        same_rows(got, outs[0][0], "groups")
        assert st == outs[0][1] and cs == outs[0][2]
    got, st, cs = outs[0]
    assert 0 < cs["fast_plies"] and st["samples"] == cs["full_plies"] and st["plies"] == cs["full_plies"] + cs["fast_plies"]
    # the first 28 of these games are the wave of test 1: a game depends on (seed, game id) only
    want, _ = model_wave("othello6", "random")
    first = got["meta"][:, 0] < FIRST + N_GAMES
    same_rows({k: v[first] for k, v in got.items()}, want, "groups against the model")


# ------------------------------------------------------------------------------------------------------------------ 3
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


def _compare(eng, slot, m, what):
    a, N, Q, P, rootn = eng.root_children(slot)
    want = m.root_children()
    assert list(a) == [c[0] for c in want] and list(N) == [c[1] for c in want] and rootn == m.root.N, (what, list(N), [c[1] for c in want])
    assert np.array_equal(np.asarray(Q).view(np.int64), np.array([c[2] for c in want], np.float64).view(np.int64)), what
    assert np.array_equal(np.asarray(P).view(np.int64), np.array([c[3] for c in want], np.float64).view(np.int64)), what
    assert eng.nodes_used(slot) == m.node_count(), what


def test_budgets_through_the_finer_grained_api():
    roots = _roots(10)
    gids, plies = 300 + np.arange(10), np.arange(10)
    full = [M.coin_full(SEED, g, p, CAP[1]) for g, p in zip(gids, plies)]
    assert 2 <= sum(full) <= 8, full  # some roots at plies whose coin is fast, some full
    eng = fake_engine("othello6", "random", 10)
    eng.set_playout_cap(CAP)
    eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8), game_ids=gids.astype(np.uint32),
                  plies=plies.astype(np.int32))
    models = [Model(b, K=1, noise=None, tie="random", seed=SEED, game_id=int(g), ply=int(p)) for b, g, p in zip(roots, gids, plies)]
    grown = np.zeros(10, np.int64)
    for n in (9, 3, 7):  # above n_fast, below it, above it again: every search call walks the budget again
        eng.search(n)
        ro = eng.root_readout()
        for s, m in enumerate(models):
            assert M.search_call(m, n, CAP, NOISE) is full[s]
            grown[s] += n if full[s] else min(n, CAP[0])
            _compare(eng, s, m, ("search", n, s, full[s]))
        assert list(ro["root_N"].cpu().numpy()) == list(grown)  # fresh roots: the root's N is what the searches walked
        assert list(ro["visits"].sum(dim=1).cpu().numpy()) == list(grown)
    assert eng.playout_cap_stats() == {"full_plies": 0, "fast_plies": 0} and eng.stats()["samples"] == 0
    eng.advance()  # records the full slots only
    want = [M.advance(m, TMAX, TMIN, f) for m, f in zip(models, full)]
    want = [w for w in want if w is not None]
    got = ordered(eng.samples())
    assert eng.playout_cap_stats() == {"full_plies": sum(full), "fast_plies": 10 - sum(full)}
    assert eng.stats()["samples"] == sum(full) == len(got["z"]) and eng.stats()["plies"] == 10
    assert [int(g) for g in got["meta"][:, 0]] == [int(g) for g, f in zip(gids, full) if f]
    for k in ("state", "pi", "visits", "meta"):
        same_rows({k: got[k]}, {k: np.array([w[k] for w in want]).reshape(got[k].shape)}, ("advance", k), keys=(k,))
    assert eng.stats()["net_evals"] == sum(m.rows for m in models)
    eng.search(N_SIM)  # the next ply, on the subtree the move kept: new coins, a full ply inherits what a fast one grew
    for s, m in enumerate(models):
        M.search_call(m, N_SIM, CAP, NOISE)
        _compare(eng, s, m, ("after the move", s))
    assert eng.stats()["error_flags"] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4
def othello6_net():
    if "net" not in _CACHE:
        net = OthelloNet(6, device="cuda")
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.tensor(v) for k, v in cf.closed_form_state_dict(shapes).items()})
        net.eval()
        _CACHE["net"] = net.to_hip(max_batch=64)
    return _CACHE["net"]


def net_run(cap, n_games=32, seed=23):
    """32 games on 20 slots of a production engine (Philox Dirichlet noise, random ties, the HIP network): (sorted samples, stats, cap stats)"""
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=20, n_sim=N_SIM, net=othello6_net(), seed=seed, node_capacity=8192)
    if cap is not None:
        eng.set_playout_cap(cap)
    got = ordered(eng.run(n_games, first_game_id=50))
    st, cs = eng.stats(), eng.playout_cap_stats()
    assert st["error_flags"] == 0 and st["games_done"] == n_games
    eng.close()
    return got, st, cs


def test_production_noise_on_the_network():
    off, st_off, cs_off = net_run(None)
    assert cs_off == {"full_plies": 0, "fast_plies": 0}  # counted while the mode is on
    for n_fast in (1, 4, N_SIM - 1):  # p_full = 1.0: every ply is full, whatever n_fast
        one, st, cs = net_run((n_fast, 1.0))
        same_rows(one, off, ("p_full 1.0", n_fast))
        assert cs == {"full_plies": st_off["plies"], "fast_plies": 0}
        assert (st["samples"], st["plies"], st["net_evals"]) == (st_off["samples"], st_off["plies"], st_off["net_evals"])
    cap, st, cs = net_run(CAP)
    assert 0 < cs["fast_plies"] and st["samples"] == cs["full_plies"] == len(cap["z"]) and st["plies"] == cs["full_plies"] + cs["fast_plies"]
    assert st["net_evals"] < st_off["net_evals"]
    meta, vsum = cap["meta"], cap["visits"].sum(axis=1)
    # every sample is a full ply by the coin
    assert all(E.SelfPlayEngine.playout_cap_full(23, g, p, CAP[1]) and M.coin_full(23, g, p, CAP[1]) for g, p in meta[:, :2])
    # a full ply 0 saw what the mode-off engine saw: the same sample (z aside: the games part ways at the first fast ply)
    zero = 0
    for i in np.nonzero(meta[:, 1] == 0)[0]:
        j = np.nonzero((off["meta"][:, 0] == meta[i, 0]) & (off["meta"][:, 1] == 0))[0][0]
        same_rows({k: cap[k][i:i + 1] for k in KEYS}, {k: off[k][j:j + 1] for k in KEYS}, ("ply 0", int(meta[i, 0])), keys=("state", "pi", "visits", "meta"))
        zero += 1
    assert zero == sum(M.coin_full(23, g, 0, CAP[1]) for g in range(50, 82)) > 0
    # visits = n_sim + what the root inherited.  A fresh root (ply 0) inherits nothing.  A root that was the child played on a recorded
    # ply had visits[action] there, one of them its own evaluation: it inherits visits[action] - 1.  Behind fast plies the inherited
    # count is bounded by what those plies could add: n_fast each, on top of the last recorded ply's (or nothing).
    for i in range(len(vsum)):
        g, p = int(meta[i, 0]), int(meta[i, 1])
        if p == 0:
            assert vsum[i] == N_SIM
            continue
        prev = i - 1 if i > 0 and meta[i - 1, 0] == g else None
        if prev is not None and meta[prev, 1] == p - 1:
            assert vsum[i] == N_SIM + cap["visits"][prev, meta[prev, 3]] - 1, (g, p)
        else:
            last = -1 if prev is None else int(meta[prev, 1])
            base = 0 if prev is None else int(cap["visits"][prev, meta[prev, 3]])
            assert N_SIM <= vsum[i] <= N_SIM + base + CAP[0] * (p - 1 - last), (g, p)


# ------------------------------------------------------------------------------------------------------------------ 5
def test_off_is_off():
    outs = []
    for detour in (False, True):
        eng = fake_engine("othello6", "random", N_SLOTS)
        if detour:
            eng.set_playout_cap(CAP)
            eng.set_playout_cap(CAP)  # the same setting again: nothing to do
            eng.set_playout_cap(None)
            eng.set_playout_cap(None)
        got = {k: v.cpu().numpy() for k, v in eng.run(N_GAMES, first_game_id=FIRST).items()}  # unsorted: the same launches, the same order
        st = eng.stats()
        assert eng.playout_cap_stats() == {"full_plies": 0, "fast_plies": 0} and st["samples"] == st["plies"]
        outs.append((got, st))
        eng.close()
    same_rows(outs[1][0], outs[0][0], "on, off, run")
    for k in ("samples", "plies", "net_evals", "lockstep_iters", "graph_replays", "games_done", "max_nodes_used"):
        assert outs[1][1][k] == outs[0][1][k], k
    assert outs[0][1]["graph_replays"] > 0


def test_the_setter_waits_for_an_open_search():
    eng = fake_engine("othello6", "random", 4)
    b = make_board("othello", 6, 6)
    eng.set_roots(np.tile(b.grid.astype(np.int8)[None], (4, 1, 1)), np.full(4, b.player, np.int8))
    eng.search_begin(4)
    for cap in (CAP, None):
        with pytest.raises(_lib.AzError, match=r"\[-3\] az_engine_set_playout_cap: a search begun"):
            eng.set_playout_cap(cap)
    with pytest.raises(_lib.AzError, match=r"\[-3\] az_engine_playout_cap_stats"):
        eng.playout_cap_stats()
    eng.search_end()
    eng.set_playout_cap(CAP)
    eng.search_begin(4)
    eng.search_end()
    assert eng.stats()["error_flags"] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 6
def test_refusals_name_the_mode():
    eng = fake_engine("othello6", "random", 4)
    for bad in ((N_SIM, 0.4), (N_SIM + 5, 0.4)):
        with pytest.raises(ValueError, match=r"n_fast must be in \[1, n_sim = 12\)"):
            eng.set_playout_cap(bad)
    assert _lib.lib().az_engine_set_playout_cap(eng.h, 4, 0.0) == _lib.AZ_EINVAL and _lib.lib().az_engine_set_playout_cap(eng.h, -1, 0.5) == _lib.AZ_EINVAL
    assert _lib.lib().az_engine_set_playout_cap(eng.h, 4, float("nan")) == _lib.AZ_EINVAL
    eng.set_leaf_batch(2)
    with pytest.raises(ValueError, match=r"playout cap is not served for leaf_batch > 1"):
        eng.set_playout_cap(CAP)
    eng.set_leaf_batch(1)
    eng.set_gumbel(8)
    with pytest.raises(ValueError, match=r"playout cap is not served for the Gumbel search"):
        eng.set_playout_cap(CAP)
    eng.set_gumbel(None)
    eng.set_playout_cap(CAP)  # and the other way round, while the cap is on
    with pytest.raises(ValueError, match=r"az_engine_set_leaf_batch: the playout cap is on"):
        eng.set_leaf_batch(2)
    with pytest.raises(ValueError, match=r"az_engine_set_gumbel: the playout cap is on"):
        eng.set_gumbel(8)
    eng.set_leaf_batch(1)
    eng.set_gumbel(None)
    eng.set_gumbel_batch(4)      # in force with the Gumbel mode only: accepted
    eng.set_gumbel_batch(1)
    eng.close()
    net = E.SelfPlayEngine(0, 6, 6, n_slots=4, n_sim=N_SIM, net=othello6_net(), seed=1)
    for sym, name in (("all", "the symmetry ensemble"), ("random", "the random symmetry mode")):
        net.set_symmetry(sym)
        with pytest.raises(ValueError, match=f"playout cap is not served for {name}"):
            net.set_playout_cap(CAP)
        net.set_symmetry(None)
    net.set_playout_cap(CAP)
    with pytest.raises(ValueError, match=r"az_engine_set_symmetry: the playout cap is on"):
        net.set_symmetry("all")
    with pytest.raises(ValueError, match=r"az_engine_set_symmetry_random: the playout cap is on"):
        net.set_symmetry("random")
    net.close()
    for ev, name in ((E.EVAL_ROLLOUT, "AZ_EVAL_ROLLOUT"), (E.EVAL_EXTERNAL, "AZ_EVAL_EXTERNAL")):
        other = E.SelfPlayEngine(0, 6, 6, n_slots=4, n_sim=N_SIM, evaluator=ev, seed=1)
        with pytest.raises(ValueError, match=f"playout cap is not served for .*{name}"):
            other.set_playout_cap(CAP)
        other.set_playout_cap(None)  # off stays off everywhere
        other.close()


# ------------------------------------------------------------------------------------------------------------------ 7
def test_one_trainer_iteration(tmp_path):
    from alphazero_amd import base
    from alphazero_amd.games.othello import OthelloConfig
    from alphazero_amd.trainer import AlphaZeroTrainer
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    tr = AlphaZeroTrainer(verbose=False, engine_slots=16, seed=6, materialize_memory=True, selfplay_playout_cap=(4, 0.4))
    tr.game = "othello"
    tr.config = OthelloConfig(board_size=6, simulations=8, episodes=16, epochs=1, batch_size=16, iterations=1, do_eval=False, device="cuda")
    torch.manual_seed(3)
    tr.setup()
    tr.self_play(0)
    cs = tr._engine.playout_cap_stats()
    got = {k: v.cpu().numpy() for k, v in tr.device_samples.items()}
    assert 0 < cs["fast_plies"] and 0 < cs["full_plies"] == len(got["z"]) == tr._engine.stats()["samples"]
    assert sum(1 for s in tr.memory if s.transformation is None) == cs["full_plies"]  # the base samples; the rest are their twins
    assert all(M.coin_full(6, g, p, 0.4) for g, p in got["meta"][:, :2])
    c = tr.config
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=16, n_sim=8, net=tr._hipnet, dirichlet_alpha=c.dirichlet_alpha, dirichlet_epsilon=c.dirichlet_epsilon,
                           temp_max_step=c.temp_max_step, temp_min_step=c.temp_min_step, seed=6, max_plies=72, sample_capacity=16 * 72)
    eng.set_playout_cap((4, 0.4))
    want = ordered(eng.run(16, first_game_id=0))
    assert eng.playout_cap_stats() == cs
    eng.close()
    same_rows(got, want, "trainer")
    tr.optimize_network(0)
    tr.update_network(0)
    assert tr.loss_values[0] and tr.sgd_backend_used is not None
