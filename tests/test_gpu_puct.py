"""GPU: the PUCT exploration settings -- c_init, c_base and first-play urgency (k_step_puct, k_step_puct_cached; az_engine_set_puct;
DESIGN section 35).  Comparisons are bit for bit on the byte views of the arrays, against the host model (tests/puct_model.py).

  1. whole az_engine_run waves are the host model's: state, pi, visits, z, meta and net_evals, on three boards and both tie modes under
     (1.25, 8, 0.25), and under (2.5, 0, off), (1.0, 8, off) and (1.0, 0, 0.25) on Othello 6x6; hash noise, a fractional temperature
     schedule, a ragged block and slot refill;
  2. the same games under 1, 2 and 4 slot groups; with the evaluation cache forced on the samples are the bits they are without;
  3. set_roots / search / root_children / root_readout / advance: root N, Q and P after every search call, a readout's pi and action are
     what the advance that follows records; again on the inherited tree;
  4. a root with more than 16 children: the vis sum crosses the rounds of 16 lanes and the lane tree;
  5. production noise on the HIP network: every root grows by exactly n_sim visits, every recorded pi sums to 1 and is 0 wherever
     visits is 0; MCT(puct=...) and BatchedAlphaZeroPlayer(puct=...) play a few plies and equal each other's roots;
  6. off is off: on, off, run -- the samples and the graph replays of an engine that never had it on; set_puct(1.0, 0, -1) is the mode
     off; a change of the settings between two searches takes effect;
  7. every refusal, in both directions; the setter waits for an open search;
  8. one trainer iteration with selfplay_puct, and one BatchedArena match with search={"puct": ...} on one side.
(tests/test_puct_host.py checks on the model that every wave played here differs from the plain search's.)
"""
import numpy as np
import pytest
import torch

import playout_cap_model as PC
import puct_model as PM
from alphazero_amd import _lib
from alphazero_amd import engine as E
from alphazero_amd.games.othello import OthelloNet
from leaf_batch_model import make_board
from tools import closed_form as cf

pytestmark = pytest.mark.gpu

TIES = {"lowest": E.TIE_LOWEST, "random": E.TIE_RANDOM}
KEYS = ("state", "pi", "visits", "z", "meta")
_CACHE = {}


def fake_engine(tag, tie, n_slots, n_sim=None, **kw):
    _, gid, H, W = PM.GAMES[tag]
    kw.setdefault("node_capacity", 8192)
    kw.setdefault("sample_capacity", 4096)  # TicTacToe: 28 games of up to 9 plies on 20 slots outgrow the default
    return E.SelfPlayEngine(gid, H, W, n_slots=n_slots, n_sim=n_sim or PM.N_SIMS[tag], evaluator=E.EVAL_FAKE, tie_mode=TIES[tie],
                            noise_mode=E.NOISE_HASH, dirichlet_alpha=PM.NOISE[0], dirichlet_epsilon=PM.NOISE[1], temp_max_step=PM.TMAX,
                            temp_min_step=PM.TMIN, seed=PM.SEED, **kw)


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
@pytest.mark.parametrize("tag,tie,puct", PM.WAVES, ids=[f"{t}-{tie}-{p}" for t, tie, p in PM.WAVES])
def test_a_wave_is_the_host_models(tag, tie, puct):
    want, ctr = PM.wave(tag, tie, puct)
    eng = fake_engine(tag, tie, PM.N_SLOTS)  # 20 slots: a full block and a ragged one; 28 games: 8 slots are refilled
    eng.set_puct(*puct)
    assert eng.puct == tuple(puct)
    got = ordered(eng.run(PM.N_GAMES, first_game_id=PM.FIRST))
    same_rows(got, want, (tag, tie, puct))
    st = eng.stats()
    assert (st["samples"], st["plies"], st["games_done"], st["net_evals"]) == (ctr["samples"], ctr["plies"], PM.N_GAMES, ctr["rows"])
    assert st["error_flags"] == 0 and st["graph_replays"] > 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 2
def test_slot_groups_play_the_same_games():
    n_games = 56
    outs = []
    for n in (1, 2, 4):
        eng = fake_engine("othello6", "random", 48)  # three blocks: groups of 48 | 32 + 16 | 16 + 16 + 16 + 0
        eng.set_puct(*PM.FULL)
        eng.set_groups(n)
        assert eng.groups() == n
        got = ordered(eng.run(n_games, first_game_id=PM.FIRST))
        st = eng.stats()
        assert st["error_flags"] == 0 and st["games_done"] == n_games
        outs.append((got, {k: st[k] for k in ("samples", "plies", "net_evals", "games_done")}))
        eng.close()
    for got, st in outs[1:]:
        same_rows(got, outs[0][0], "groups")
        assert st == outs[0][1]
    # the first 28 of these games are the wave of test 1: a game depends on (seed, game id, the settings) only
    want, _ = PM.wave("othello6", "random", PM.FULL)
    got = outs[0][0]
    first = got["meta"][:, 0] < PM.FIRST + PM.N_GAMES
    same_rows({k: v[first] for k, v in got.items()}, want, "groups against the model")


N_SIM_NET = 12


def othello6_net():
    if "net" not in _CACHE:
        net = OthelloNet(6, device="cuda")
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.tensor(v) for k, v in cf.closed_form_state_dict(shapes).items()})
        net.eval()
        _CACHE["net"] = net.to_hip(max_batch=64)
    return _CACHE["net"]


def net_run(puct, n_games=32, seed=23, cache=None, groups=None):
    """32 games on 20 slots of a production engine (Philox Dirichlet noise, random ties, the HIP network)"""
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=20, n_sim=N_SIM_NET, net=othello6_net(), seed=seed, node_capacity=8192)
    if puct is not None:
        eng.set_puct(*puct)
    if cache is not None:
        eng.set_eval_cache(cache)
    if groups is not None:
        eng.set_groups(groups)
    got = ordered(eng.run(n_games, first_game_id=50))
    st, cs = eng.stats(), eng.eval_cache_stats()
    assert st["error_flags"] == 0 and st["games_done"] == n_games
    eng.close()
    return got, st, cs


def test_with_the_evaluation_cache_the_samples_stay():
    off, st_off, cs_off = net_run(PM.FULL, cache=False)
    assert not cs_off["in_force"] and cs_off["cache_hits"] == 0
    for groups in (1, 2):
        on, st, cs = net_run(PM.FULL, cache=True, groups=groups)
        assert cs["in_force"] and cs["cache_hits"] > 0
        same_rows(on, off, ("cache on", groups))
        assert (st["samples"], st["plies"], st["net_evals"]) == (st_off["samples"], st_off["plies"], st_off["net_evals"])


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


def _readout_is_the_models(eng, models):
    """root_readout's pi, action and visits against the model's move_policy (the settings do not touch it); the readout as numpy"""
    ro = {key: v.cpu().numpy() for key, v in eng.root_readout().items() if key in ("pi", "action", "visits", "root_N")}
    for s, m in enumerate(models):
        idx, pi = PC.move_policy(m, PC.linear_temp(m.ply, PM.TMAX, PM.TMIN))
        assert np.array_equal(ro["pi"][s].view(np.uint32), pi.view(np.uint32)), ("readout pi", s)
        assert int(ro["action"][s]) == m.root.children[idx].act, ("readout action", s)
        vis = np.zeros(m.A, np.int32)
        for c in m.root.children:
            vis[c.act] = c.N
        assert np.array_equal(ro["visits"][s], vis) and int(ro["root_N"][s]) == m.root.N
    return ro


def test_the_finer_grained_api():
    n = 6
    roots = _roots(n)
    gids, plies = 300 + np.arange(n), np.arange(n)  # plies 0 .. 5: temperatures 1 and fractional
    eng = fake_engine("othello6", "random", n, n_sim=12)
    eng.set_puct(*PM.FULL)
    eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8), game_ids=gids.astype(np.uint32),
                  plies=plies.astype(np.int32))
    models = [PM.PuctModel(b, K=1, noise=None, tie="random", seed=PM.SEED, game_id=int(g), ply=int(p), puct=PM.FULL)
              for b, g, p in zip(roots, gids, plies)]
    for round_ in range(2):  # fresh roots, then the roots the move left: inherited counts and an inherited root Q
        for sims in (9, 3, 7):
            eng.search(sims)
            for s, m in enumerate(models):
                PM.search_call(m, sims, PM.NOISE)
                _compare(eng, s, m, ("search", round_, sims, s))
        ro = _readout_is_the_models(eng, models)
        before = eng.stats()["samples"]
        eng.advance()
        got = {k: v.cpu().numpy()[before:] for k, v in eng.samples().items()}  # this ply's rows
        rows = {int(g): i for i, g in enumerate(got["meta"][:, 0].view(np.uint32))}
        assert sorted(rows) == [int(g) for g in gids]
        for s, m in enumerate(models):
            smp = PM.advance(m, PM.TMAX, PM.TMIN)
            i = rows[int(gids[s])]
            for k in ("state", "pi", "visits", "meta"):
                same_rows({k: got[k][i]}, {k: np.asarray(smp[k]).reshape(got[k][i].shape)}, ("advance", round_, s, k), keys=(k,))
            # what the readout showed is what the advance recorded and played
            assert np.array_equal(got["pi"][i].view(np.uint32), ro["pi"][s].view(np.uint32)) and int(got["meta"][i, 3]) == int(ro["action"][s])
            assert np.array_equal(got["visits"][i], ro["visits"][s])
        assert not any(m.root.board.is_game_over() for m in models)
        if round_ == 0:
            assert any(m.root.N > 0 and m.root.Q != 0.0 for m in models)  # the inherited root's Q is read by first-play urgency
    assert eng.stats()["error_flags"] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("tie", ["lowest", "random"])
def test_a_root_with_more_than_16_children(tie):
    sims = PM.WIDE_SIMS
    eng = E.SelfPlayEngine(0, 8, 8, n_slots=2, n_sim=sims, dirichlet_alpha=PM.NOISE[0], dirichlet_epsilon=PM.NOISE[1], temp_max_step=2, temp_min_step=7,
                           tie_mode=TIES[tie], noise_mode=E.NOISE_HASH, evaluator=E.EVAL_FAKE, seed=PM.WIDE_SEED, node_capacity=1 << 15)
    eng.set_puct(*PM.FULL)
    eng.set_roots(np.stack([PM.MANY_MOVES, PM.MANY_MOVES]), np.array([1, 1], np.int8), game_ids=np.array(PM.WIDE_GIDS, np.uint32))
    eng.search(sims)
    models = []
    for slot, gid in enumerate(PM.WIDE_GIDS):
        m = PM.wide_root(tie, gid)
        assert len(m.root.children) == 34 and m.high_fpu_picks > 0
        _compare(eng, slot, m, ("wide root", tie, slot))
        models.append(m)
    ro = {key: v.cpu().numpy() for key, v in eng.root_readout().items() if key in ("visits", "root_N")}
    for s, m in enumerate(models):
        assert int(ro["root_N"][s]) == sims and int(ro["visits"][s].sum()) == sims
    assert eng.stats()["error_flags"] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 5
def test_production_noise_on_the_network():
    off, st_off, _ = net_run(None)
    got, st, _ = net_run(PM.FULL)
    assert st["samples"] == st["plies"] == len(got["z"])
    assert got["visits"].shape != off["visits"].shape or (got["visits"] != off["visits"]).any()
    meta, vsum = got["meta"], got["visits"].sum(axis=1)
    # every root grows by exactly n_sim visits: a fresh root (ply 0) holds n_sim; a root that was the child played on the ply before
    # had visits[action] there, one of them its own evaluation, and inherits visits[action] - 1
    for i in range(len(vsum)):
        g, p = int(meta[i, 0]), int(meta[i, 1])
        if p == 0:
            assert vsum[i] == N_SIM_NET, (g, p)
        else:
            assert meta[i - 1, 0] == g and meta[i - 1, 1] == p - 1
            assert vsum[i] == N_SIM_NET + got["visits"][i - 1, meta[i - 1, 3]] - 1, (g, p)
    # a recorded pi: every entry is a double p_i rounded to float32 (off by at most p_i 2^-24) and the p_i sum to 1 within a few
    # 2^-53, so the float32 row sums to 1 within 2^-23; and it is 0 wherever visits is 0
    assert np.all(np.abs(got["pi"].astype(np.float64).sum(axis=1) - 1.0) <= 2.0 ** -23)
    assert np.all(got["pi"][got["visits"] == 0] == 0.0)


def test_mct_and_the_batched_player_search_the_same_roots():
    from alphazero_amd.mcts import MCT
    from alphazero_amd.players import BatchedAlphaZeroPlayer
    from leaf_batch_model import _act
    torch.manual_seed(4)
    nn = OthelloNet(n=6).eval()
    spec = {"c_init": PM.FULL[0], "c_base": PM.FULL[1], "fpu": PM.FULL[2]}
    n_sim, boards = 24, _roots(4)
    many = BatchedAlphaZeroPlayer(n_sim=n_sim, nn=nn, n_slots=4, puct=spec)
    many._tie_mode = E.TIE_LOWEST
    for ply in range(3):  # a few plies: the batched players' second and third searches run on the trees their moves left
        res = many.get_moves(boards, temps=0)
        assert many._engine.puct == PM.FULL
        for b, (move, probs, visits, _) in zip(boards, res):
            mct = MCT(eval_method="neural", nn=nn, puct=spec)
            mct._tie_mode = E.TIE_LOWEST
            mct.search(b, n_sim=n_sim)
            assert mct._engine.puct == PM.FULL
            if ply == 0:  # fresh roots on both sides: the same search, root for root
                p1, counts = mct.get_action_probs(b, 0)
                assert {_act(b, mv): n for mv, n in counts.items()} == {_act(b, mv): n for mv, n in visits.items()}
                best = {mv for mv, n in counts.items() if n == max(counts.values())}  # equal counts: each side draws its own move
                assert set(p1) <= best and move in best and probs == {move: 1}
            assert sum(visits.values()) >= n_sim
        for b, (move, _, _, _) in zip(boards, res):
            b.play_move(move)
        if any(b.is_game_over() for b in boards):
            break
    many.close()


# ------------------------------------------------------------------------------------------------------------------ 6
def test_off_is_off():
    outs = []
    for detour in (False, True):
        eng = fake_engine("othello6", "random", PM.N_SLOTS)
        if detour:
            eng.set_puct(*PM.FULL)
            eng.set_puct(*PM.FULL)  # the same setting again: nothing to do
            eng.set_puct(2.5)
            eng.set_puct(None)
            eng.set_puct(None)
        assert eng.puct == (1.0, 0.0, -1.0)
        got = {k: v.cpu().numpy() for k, v in eng.run(PM.N_GAMES, first_game_id=PM.FIRST).items()}  # unsorted: the same launches, the same order
        outs.append((got, eng.stats()))
        eng.close()
    same_rows(outs[1][0], outs[0][0], "on, off, run")
    for k in ("samples", "plies", "net_evals", "lockstep_iters", "graph_replays", "games_done", "max_nodes_used"):
        assert outs[1][1][k] == outs[0][1][k], k
    assert outs[0][1]["graph_replays"] > 0
    same_rows(ordered({k: torch.tensor(v) for k, v in outs[0][0].items()}), PM.plain_wave("othello6", "random")[0], "the plain wave")


def test_the_neutral_triple_is_the_mode_off():
    eng = fake_engine("othello6", "random", PM.N_SLOTS)
    eng.set_puct(*PM.FULL)
    eng.set_puct(1.0, 0, -1)
    assert eng.puct == (1.0, 0.0, -1.0)
    eng.set_puct(1.0, 0, -0.25)  # any negative fpu is off: reported as the canonical -1
    assert eng.puct == (1.0, 0.0, -1.0)
    eng.set_leaf_batch(2)        # nothing refuses beside the neutral triple
    eng.set_puct({"c_init": 1.0, "c_base": 0, "fpu": None})
    eng.set_leaf_batch(1)
    got = ordered(eng.run(PM.N_GAMES, first_game_id=PM.FIRST))
    same_rows(got, PM.plain_wave("othello6", "random")[0], "the neutral triple")
    assert eng.stats()["graph_replays"] > 0
    eng.close()


def test_a_change_between_two_searches_takes_effect():
    """two engines, graphs on: the second search of each runs under other settings than its first, and is the model's under them"""
    roots = _roots(4)
    for first, second in ((PM.FULL, (2.5, 0.0, -1.0)), ((1.0, 0.0, -1.0), PM.FULL), (PM.FULL, (1.0, 0.0, -1.0))):
        eng = fake_engine("othello6", "random", 4, n_sim=12)
        models = []
        for rep in range(2):  # the same pair of searches twice over fresh roots: the second time a captured graph could be replayed
            eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8),
                          game_ids=np.arange(40, 44).astype(np.uint32))
            models = [PM.PuctModel(b, K=1, noise=None, tie="random", seed=PM.SEED, game_id=40 + i) for i, b in enumerate(roots)]
            for puct in (first, second):
                eng.set_puct(*puct)
                eng.search(12)
                for s, m in enumerate(models):
                    m.puct = tuple(puct)
                    PM.search_call(m, 12, PM.NOISE)
                    _compare(eng, s, m, ("change", first, second, rep, s))
        assert eng.stats()["error_flags"] == 0
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ 7
def test_the_setter_waits_for_an_open_search():
    eng = fake_engine("othello6", "random", 4)
    b = make_board("othello", 6, 6)
    eng.set_roots(np.tile(b.grid.astype(np.int8)[None], (4, 1, 1)), np.full(4, b.player, np.int8))
    eng.search_begin(4)
    for spec in (PM.FULL, (1.0, 0.0, -1.0)):
        with pytest.raises(_lib.AzError, match=r"\[-3\] az_engine_set_puct: a search begun"):
            eng.set_puct(*spec)
    eng.search_end()
    eng.set_puct(*PM.FULL)
    eng.search_begin(4)
    eng.search_end()
    assert eng.stats()["error_flags"] == 0 and eng.puct == PM.FULL
    eng.close()


def test_refusals_name_the_mode_both_ways():
    eng = fake_engine("othello6", "random", 4)
    L = _lib.lib()
    for bad, msg in (((0.0, 0.0, -1.0), b"c_init must be finite and in (0, 64]"), ((64.5, 0.0, -1.0), b"c_init must be"), ((float("nan"), 0.0, -1.0), b"c_init must be"),
                     ((float("inf"), 0.0, -1.0), b"c_init must be"), ((1.0, 0.5, -1.0), b"c_base must be 0 (no growth) or finite and in [1, 1e9]"),
                     ((1.0, 2e9, -1.0), b"c_base must be"), ((1.0, float("nan"), -1.0), b"c_base must be"), ((1.0, -8.0, -1.0), b"c_base must be"),
                     ((1.0, 0.0, 4.5), b"fpu must be negative (off) or finite and in [0, 4]"), ((1.0, 0.0, float("nan")), b"fpu must be"),
                     ((1.0, 0.0, float("inf")), b"fpu must be")):
        assert L.az_engine_set_puct(eng.h, *bad) == _lib.AZ_EINVAL
        assert msg in L.az_last_error(), (bad, L.az_last_error())
    assert eng.puct == (1.0, 0.0, -1.0)
    eng.set_puct(64, 1e9, 4)
    eng.set_puct(None)
    # the other mode on first: the setter names it
    on_off = [("leaf_batch > 1", lambda: eng.set_leaf_batch(2), lambda: eng.set_leaf_batch(1)),
              ("the Gumbel search", lambda: eng.set_gumbel(8), lambda: eng.set_gumbel(None)),
              ("the playout cap", lambda: eng.set_playout_cap((4, 0.4)), lambda: eng.set_playout_cap(None)),
              ("forced playouts", lambda: eng.set_forced_playouts(2.0), lambda: eng.set_forced_playouts(None)),
              ("exact endgames", lambda: eng.set_exact_endgame(4), lambda: eng.set_exact_endgame(None)),
              ("proof backup", lambda: eng.set_proof_backup(True), lambda: eng.set_proof_backup(False))]
    for name, on, off in on_off:
        on()
        with pytest.raises(ValueError, match=f"az_engine_set_puct: PUCT exploration settings are not served for {name}"):
            eng.set_puct(*PM.FULL)
        eng.set_puct(None)  # off stays off beside everything
        off()
    # and the other way round, while the settings are on
    eng.set_puct(*PM.FULL)
    for setter, call in (("az_engine_set_leaf_batch", lambda: eng.set_leaf_batch(2)), ("az_engine_set_gumbel", lambda: eng.set_gumbel(8)),
                         ("az_engine_set_playout_cap", lambda: eng.set_playout_cap((4, 0.4))),
                         ("az_engine_set_forced_playouts", lambda: eng.set_forced_playouts(2.0)),
                         ("az_engine_set_exact_endgame", lambda: eng.set_exact_endgame(4)),
                         ("az_engine_set_proof_backup", lambda: eng.set_proof_backup(True))):
        with pytest.raises(ValueError, match=f"{setter}: PUCT exploration settings are on"):
            call()
    eng.set_groups(1)           # slot groups combine
    eng.set_leaf_batch(1)       # and every mode's off is served beside the settings
    eng.set_gumbel(None)
    eng.set_playout_cap(None)
    eng.set_forced_playouts(None)
    eng.set_exact_endgame(None)
    eng.set_proof_backup(False)
    eng.close()
    net = E.SelfPlayEngine(0, 6, 6, n_slots=4, n_sim=N_SIM_NET, net=othello6_net(), seed=1)
    for sym, name in (("all", "the symmetry ensemble"), ("random", "the random symmetry mode")):
        net.set_symmetry(sym)
        with pytest.raises(ValueError, match=f"PUCT exploration settings are not served for {name}"):
            net.set_puct(*PM.FULL)
        net.set_symmetry(None)
    net.set_puct(*PM.FULL)
    with pytest.raises(ValueError, match=r"az_engine_set_symmetry: PUCT exploration settings are on"):
        net.set_symmetry("all")
    with pytest.raises(ValueError, match=r"az_engine_set_symmetry_random: PUCT exploration settings are on"):
        net.set_symmetry("random")
    net.set_eval_cache(True)    # the evaluation cache combines
    net.close()
    for ev, name in ((E.EVAL_ROLLOUT, "AZ_EVAL_ROLLOUT"), (E.EVAL_EXTERNAL, "AZ_EVAL_EXTERNAL")):
        other = E.SelfPlayEngine(0, 6, 6, n_slots=4, n_sim=N_SIM_NET, evaluator=ev, seed=1)
        with pytest.raises(ValueError, match=f"PUCT exploration settings are not served for .*{name}"):
            other.set_puct(*PM.FULL)
        other.set_puct(None)  # off stays off everywhere
        other.close()


# ------------------------------------------------------------------------------------------------------------------ 8
def test_one_trainer_iteration(tmp_path):
    from alphazero_amd import base
    from alphazero_amd.games.othello import OthelloConfig
    from alphazero_amd.trainer import AlphaZeroTrainer
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    spec = {"c_init": 1.25, "c_base": 8, "fpu": 0.25}
    tr = AlphaZeroTrainer(verbose=False, engine_slots=16, seed=6, materialize_memory=True, selfplay_puct=spec)
    tr.game = "othello"
    tr.config = OthelloConfig(board_size=6, simulations=8, episodes=16, epochs=1, batch_size=16, iterations=1, do_eval=False, device="cuda")
    torch.manual_seed(3)
    tr.setup()
    tr.self_play(0)
    assert tr._engine.puct == PM.FULL
    got = ordered(tr.device_samples)
    assert len(got["z"]) == tr._engine.stats()["samples"]
    c = tr.config
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=16, n_sim=8, net=tr._hipnet, dirichlet_alpha=c.dirichlet_alpha, dirichlet_epsilon=c.dirichlet_epsilon,
                           temp_max_step=c.temp_max_step, temp_min_step=c.temp_min_step, seed=6, max_plies=72, sample_capacity=16 * 72)
    eng.set_puct(spec)
    want = ordered(eng.run(16, first_game_id=0))
    eng.set_puct(None)  # and the wave without the settings records other targets
    plain = ordered(eng.run(16, first_game_id=0))
    eng.close()
    same_rows(got, want, "trainer")
    assert plain["pi"].shape != want["pi"].shape or not np.array_equal(plain["pi"], want["pi"])
    tr.optimize_network(0)
    tr.update_network(0)
    assert tr.loss_values[0] and tr.sgd_backend_used is not None
    tr.selfplay_puct = None  # the next wave switches the engine back
    assert tr._ensure_engine().puct == (1.0, 0.0, -1.0)


def test_one_arena_match_with_the_settings_on_one_side():
    from alphazero_amd.arena import BatchedArena
    spec = {"c_init": 1.25, "c_base": 8, "fpu": 0.25}
    games = []
    for search in ({"puct": spec}, {}):
        arena = BatchedArena("othello", "fake", opponent="fake", n_sim=16, opponent_n_sim=12, seed=6, board_size=6, search=search, opening_plies=4)
        stats = arena.play_games(8, return_stats=True, record_moves=True)
        assert all(st["error_flags"] == 0 for st in arena.engine_stats)
        assert len(stats["player1"]) + len(stats["player2"]) + stats["draw"] == 8
        games.append([m.tolist() for m in arena.moves])
    assert games[0] != games[1]  # one side searched under the settings: other games than the plain pairing's
