"""GPU: exact endgames (az_solve.h; az_solve_batch, az_engine_set_exact_endgame).

  1. solve_batch is the host model's negamax (tests/exact_endgame_model.py), exactly, on winner and action: Othello 8x8 and 6x6 (256
     positions each from seeded random playouts stopped at 1 .. 8 empty cells, plus finished games and positions above the limit),
     the Othello 4x4 start at max_empties = 12, Connect4 6x7 and 4x4 at <= 10, TicTacToe from the empty board and along a playout;
     every candidate comes back solved, every non-candidate AZ_UNSOLVED / -1;
  2. node_budget = 1 on an 8-empties position with a legal move: AZ_UNSOLVED, AZ_OK, no error;
  3. whole az_engine_run waves are the host model's bit for bit (samples, plies, net_evals, solved_leaves): Othello 6x6 with slot refill,
     hash noise, both tie modes, E = 3 and 6; TicTacToe at E = 9;
  4. a property that needs no model: roots whose children are all within the limit take one network row per slot (the root prior),
     every visited root child's Q is exactly -1, 0 or +1 and is the negated solve_batch outcome of the child in its mover's frame;
  5. shape independence: the same games under 1, 2 and 4 slot groups and on fewer slots;
  6. with the leaf evaluation cache on and off: the same samples;
  7. off is off; 8. every refusal, both ways, by name; argument checks; AZ_ESTATE while a search is open and over searched trees.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_endgame_model as M
from alphazero_amd import _lib
from alphazero_amd import engine as E
from leaf_batch_model import _act, _move, make_board

pytestmark = pytest.mark.gpu

KEYS = ("state", "pi", "visits", "z", "meta")
TIES = {"lowest": E.TIE_LOWEST, "random": E.TIE_RANDOM}
SEED, FIRST = 11, 1000
POS_SEED = 1  # chosen on the CPU: both Othello sets hold all three outcomes, >= 3 draws and >= 4 forced passes (asserted below)


def gpu_solve(gid, H, W, boards, max_empties, budget=0):
    g, p = M.arrays(boards)
    w, a = E.solve_batch(gid, H, W, torch.from_numpy(g).cuda(), torch.from_numpy(p).cuda(), max_empties, budget)
    return list(zip(w.cpu().tolist(), a.cpu().tolist()))


def check_set(game, gid, H, W, boards, max_empties):
    memo = {}
    want = [M.solve_contract(b, max_empties, memo) for b in boards]
    got = gpu_solve(gid, H, W, boards, max_empties)
    bad = [(i, M.empties(boards[i]), want[i], got[i]) for i in range(len(boards)) if want[i] != got[i]]
    assert not bad, (game, H, W, len(bad), bad[:6])
    for b, (w, a) in zip(boards, got):  # every candidate solved, every non-candidate unsolved
        cand = b.is_game_over() or M.empties(b) <= max_empties
        assert (w in (-1, 0, 1)) == cand and (w == M.UNSOLVED and a == -1) == (not cand)
        assert (a == -1) == (b.is_game_over() or not cand)
    return want


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("n", [8, 6])
def test_solve_batch_othello_is_the_models(n):
    boards = M.positions("othello", n, n, POS_SEED, 256, 1, 8, n_over=8, n_above=8, above=12)
    want = check_set("othello", 0, n, n, boards, 8)
    live = [(b, w) for b, w in zip(boards[:256], want[:256]) if not b.is_game_over()]
    outcomes = [w[0] for _, w in live]
    assert {-1, 0, 1} <= set(outcomes) and outcomes.count(0) >= 3
    passes = [(b, w) for b, w in live if M.must_pass(b)]
    assert len(passes) >= 4 and all(w[1] == n * n for _, w in passes)
    assert sum(b.is_game_over() for b in boards) >= 8 and sum(M.empties(b) > 8 and not b.is_game_over() for b in boards) >= 1


def test_solve_batch_othello4_from_the_start():
    want = check_set("othello", 0, 4, 4, [make_board("othello", 4, 4)], 12)
    assert want == [(-1, 2)]  # the side that moves second wins, every first move loses: the lowest legal one


@pytest.mark.parametrize("H,W", [(6, 7), (4, 4)])
def test_solve_batch_connect4_is_the_models(H, W):
    boards = M.positions("connect4", H, W, POS_SEED, 64, 1, 10, n_over=4, n_above=4, above=14)
    want = check_set("connect4", 1, H, W, boards, 10)
    assert any(not b.is_game_over() and w[0] != M.UNSOLVED for b, w in zip(boards, want))


def test_solve_batch_tictactoe_is_the_models():
    assert check_set("tictactoe", 2, 3, 3, [make_board("tictactoe", 3, 3)], 9) == [(0, 0)]
    rng, b, along = np.random.default_rng(POS_SEED), make_board("tictactoe", 3, 3), []
    while not b.is_game_over():
        along.append(b.clone())
        acts = sorted(_act(b, m) for m in b.get_moves())
        b.play_move(_move(b, acts[int(rng.integers(len(acts)))]))
    along.append(b.clone())
    check_set("tictactoe", 2, 3, 3, along, 9)
    check_set("tictactoe", 2, 3, 3, along, 4)  # the early positions are above the limit


# ------------------------------------------------------------------------------------------------------------------ 2
def test_node_budget_one_is_unsolved_not_an_error():
    boards = [b for b in M.positions("othello", 8, 8, POS_SEED, 64, 8, 8) if not b.is_game_over() and not M.must_pass(b)][:4]
    assert boards and all(M.empties(b) == 8 for b in boards)
    g, p = M.arrays(boards)
    g, p = torch.from_numpy(g).cuda(), torch.from_numpy(p).cuda()
    w = torch.empty(len(boards), dtype=torch.int8, device="cuda")
    a = torch.empty(len(boards), dtype=torch.int32, device="cuda")
    rc = _lib.lib().az_solve_batch(0, 8, 8, g.data_ptr(), p.data_ptr(), len(boards), 8, 1, w.data_ptr(), a.data_ptr(), None,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.AZ_OK
    torch.cuda.synchronize()
    assert w.cpu().tolist() == [M.UNSOLVED] * len(boards) and a.cpu().tolist() == [-1] * len(boards)
    assert all(x[0] in (-1, 0, 1) for x in gpu_solve(0, 8, 8, boards, 8))  # the same positions without a budget


# ------------------------------------------------------------------------------------------------------------------ 3
GAMES = {"othello6": ("othello", 0, 6, 6), "tictactoe": ("tictactoe", 2, 3, 3)}
N_SIM = 24


def fake_engine(tag, tie, n_slots, **kw):
    _, gid, H, W = GAMES[tag]
    return E.SelfPlayEngine(gid, H, W, n_slots=n_slots, n_sim=N_SIM, evaluator=E.EVAL_FAKE, tie_mode=TIES[tie], noise_mode=E.NOISE_HASH,
                            dirichlet_alpha=M.NOISE[0], dirichlet_epsilon=M.NOISE[1], temp_max_step=M.TMAX, temp_min_step=M.TMIN, seed=SEED,
                            node_capacity=8192, sample_capacity=4096, **kw)  # room for every game of a wave that refills its slots


def ordered(smp):
    a = {k: v.cpu().numpy() for k, v in smp.items()}
    order = np.lexsort((a["meta"][:, 1], a["meta"][:, 0]))
    return {k: v[order] for k, v in a.items()}


def same_rows(got, want, what):
    for k in KEYS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)), (what, k)


@pytest.mark.parametrize("tag,tie,e", [("othello6", "lowest", 3), ("othello6", "random", 3), ("othello6", "lowest", 6),
                                       ("othello6", "random", 6), ("tictactoe", "lowest", 9), ("tictactoe", "random", 9)])
def test_a_wave_is_the_host_models(tag, tie, e):
    game, _, H, W = GAMES[tag]
    want, ctr = M.wave(game, H, W, SEED, FIRST, 16, N_SIM, e, tie)
    assert ctr["solved"] > 0
    eng = fake_engine(tag, tie, 8)  # 16 games on 8 slots: every slot is refilled
    eng.set_exact_endgame(e)
    got = ordered(eng.run(16, first_game_id=FIRST))
    same_rows(got, want, (tag, tie, e))
    st, xs = eng.stats(), eng.exact_endgame_stats()
    assert (st["samples"], st["plies"], st["games_done"], st["error_flags"]) == (ctr["samples"], ctr["plies"], 16, 0)
    assert st["net_evals"] == ctr["rows"] and xs["solved_leaves"] == ctr["solved"] and xs["solver_nodes"] >= xs["solved_leaves"]
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 4
def test_late_roots_take_one_network_row_and_exact_child_values():
    e = 6
    roots = [b for b in M.positions("othello", 6, 6, 7, 24, 3, e) if not b.is_game_over()][:16]
    assert len(roots) >= 8 and all(M.empties(b) <= e for b in roots)
    n = len(roots)
    g, p = M.arrays(roots)
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=n, n_sim=32, evaluator=E.EVAL_FAKE, tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF,
                           temp_max_step=-1, temp_min_step=0, seed=SEED, node_capacity=8192)
    eng.set_exact_endgame(e)
    eng.set_roots(g, p)
    eng.search(32)
    visited = 0
    for s, b in enumerate(roots):
        acts, N, Q, _, root_n = eng.root_children(s)
        assert root_n == 32
        kids = []
        for a in acts:
            c = b.clone()
            c.play_move(_move(c, int(a)))
            kids.append(c)
        sol = gpu_solve(0, 6, 6, kids, 8)
        for c, nv, q, (w, _) in zip(kids, N, Q, sol):
            if nv > 0:
                visited += 1
                assert q in (-1.0, 0.0, 1.0) and q == -float(int(c.player) * w), (s, nv, q, w, int(c.player))
    assert visited >= n
    assert eng.exact_endgame_stats()["solved_leaves"] > 0
    eng.advance()  # the move folds the slots' evaluation counts in
    st = eng.stats()
    assert st["net_evals"] == n and st["error_flags"] == 0  # the root prior alone: every leaf below these roots is solved or over
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 5
def test_slot_shape_does_not_change_a_game():
    outs = []
    for slots, groups in ((32, 1), (32, 2), (32, 4), (8, 1)):
        eng = fake_engine("othello6", "random", slots)
        eng.set_exact_endgame(6)
        eng.set_groups(groups)
        assert eng.groups() == groups
        got = ordered(eng.run(32, first_game_id=FIRST))
        st, xs = eng.stats(), eng.exact_endgame_stats()
        assert st["error_flags"] == 0 and st["games_done"] == 32
        outs.append((got, (st["samples"], st["plies"], st["net_evals"], xs["solved_leaves"])))
        eng.close()
    for got, counts in outs[1:]:
        same_rows(got, outs[0][0], "shape")
        assert counts == outs[0][1]
    want, _ = M.wave("othello", 6, 6, SEED, FIRST, 16, N_SIM, 6, "random")  # the first 16 games are test 3's wave
    first = outs[0][0]["meta"][:, 0] < FIRST + 16
    same_rows({k: v[first] for k, v in outs[0][0].items()}, want, "shape against the model")


# ------------------------------------------------------------------------------------------------------------------ 6
def othello6_net(max_batch):
    from alphazero_amd.games.othello import OthelloNet
    torch.manual_seed(0)
    net = OthelloNet(n=6).eval()
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    return E.HipNet(0, 6, 6, sd, max_batch=max_batch)


def test_with_the_evaluation_cache_the_samples_stay():
    net = othello6_net(32)
    outs = []
    for cache in (True, False):
        eng = E.SelfPlayEngine(0, 6, 6, n_slots=32, n_sim=16, net=net, seed=SEED)
        eng.set_exact_endgame(6)
        eng.set_eval_cache(cache)
        got = ordered(eng.run(32, first_game_id=FIRST))
        st, cs, xs = eng.stats(), eng.eval_cache_stats(), eng.exact_endgame_stats()
        assert st["error_flags"] == 0 and cs["in_force"] == cache and (cs["cache_hits"] > 0) == cache and xs["solved_leaves"] > 0
        outs.append((got, (st["samples"], st["plies"], st["net_evals"], xs["solved_leaves"])))
        eng.close()
    same_rows(outs[0][0], outs[1][0], "cache on / off")
    assert outs[0][1] == outs[1][1]
    net.close()


# ------------------------------------------------------------------------------------------------------------------ 7
def test_off_is_off():
    outs = []
    for touched in (True, False):
        eng = fake_engine("othello6", "random", 8)
        if touched:
            eng.set_exact_endgame(6)
            eng.set_exact_endgame(None)
        g, p = M.arrays([make_board("othello", 6, 6)] * 8)
        eng.set_roots(g, p)
        eng.search(N_SIM)
        kids = [eng.root_children(s) for s in range(8)]
        got = ordered(eng.run(16, first_game_id=FIRST))
        st = eng.stats()
        assert eng.exact_endgame_stats() == {"solved_leaves": 0, "solver_nodes": 0}
        outs.append((got, kids, {k: st[k] for k in ("samples", "plies", "net_evals", "games_done", "graph_replays", "lockstep_iters")}))
        eng.close()
    same_rows(outs[0][0], outs[1][0], "on, off, run")
    assert outs[0][2] == outs[1][2]
    for a, b in zip(outs[0][1], outs[1][1]):
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
    want, _ = M.wave("othello", 6, 6, SEED, FIRST, 16, N_SIM, 0, "random")
    same_rows(outs[0][0], want, "mode off against the model")


# ------------------------------------------------------------------------------------------------------------------ 8
def test_refusals_name_the_mode_both_ways():
    L = _lib.lib()
    net = othello6_net(64)

    def net_engine():
        return E.SelfPlayEngine(0, 6, 6, n_slots=8, n_sim=16, net=net, seed=SEED)

    modes = [("leaf_batch", lambda e: e.set_leaf_batch(2), lambda e: e.set_leaf_batch(1)),
             ("Gumbel", lambda e: e.set_gumbel(4), lambda e: e.set_gumbel(None)),
             ("symmetry ensemble", lambda e: e.set_symmetry("all"), lambda e: e.set_symmetry(None)),
             ("random symmetry", lambda e: e.set_symmetry("random"), lambda e: e.set_symmetry(None)),
             ("playout cap", lambda e: e.set_playout_cap((4, 0.5)), lambda e: e.set_playout_cap(None)),
             ("forced playouts", lambda e: e.set_forced_playouts(2.0), lambda e: e.set_forced_playouts(None))]
    for name, on, off in modes:
        eng = net_engine()
        on(eng)
        with pytest.raises(ValueError, match=f"exact endgames are not served for .*{name}"):
            eng.set_exact_endgame(6)
        off(eng)
        eng.set_exact_endgame(6)
        with pytest.raises(ValueError, match="exact endgames are on"):
            on(eng)
        eng.set_exact_endgame(None)
        on(eng)  # and with the mode off again the other one is accepted
        eng.close()
    for evaluator, name in ((E.EVAL_ROLLOUT, "AZ_EVAL_ROLLOUT"), (E.EVAL_EXTERNAL, "AZ_EVAL_EXTERNAL")):
        eng = E.SelfPlayEngine(0, 6, 6, n_slots=8, n_sim=16, evaluator=evaluator, seed=SEED)
        with pytest.raises(ValueError, match=f"exact endgames are not served for .*{name}"):
            eng.set_exact_endgame(6)
        eng.set_exact_endgame(None)  # off stays accepted
        eng.close()
    eng = fake_engine("othello6", "lowest", 8)
    for bad in (-1, 11, 64):
        assert L.az_engine_set_exact_endgame(eng.h, bad) == _lib.AZ_EINVAL and b"max_empties must be in [0, 10]" in L.az_last_error()
    assert L.az_engine_set_exact_endgame(None, 6) == _lib.AZ_EINVAL
    assert L.az_engine_exact_endgame_stats(eng.h, None, None) == _lib.AZ_EINVAL
    w = torch.empty(1, dtype=torch.int8, device="cuda")
    a = torch.empty(1, dtype=torch.int32, device="cuda")
    g = torch.zeros(36, dtype=torch.int8, device="cuda")
    p = torch.ones(1, dtype=torch.int8, device="cuda")
    for me, budget in ((0, 0), (13, 0), (8, -1)):
        assert L.az_solve_batch(0, 6, 6, g.data_ptr(), p.data_ptr(), 1, me, budget, w.data_ptr(), a.data_ptr(), None, None) == _lib.AZ_EINVAL
    assert L.az_solve_batch(0, 6, 6, None, p.data_ptr(), 1, 8, 0, w.data_ptr(), a.data_ptr(), None, None) == _lib.AZ_EINVAL
    assert L.az_solve_batch(0, 5, 5, g.data_ptr(), p.data_ptr(), 1, 8, 0, w.data_ptr(), a.data_ptr(), None, None) == _lib.AZ_EINVAL
    assert L.az_solve_batch(0, 6, 6, None, None, 0, 8, 0, None, None, None, None) == _lib.AZ_OK  # an empty batch
    # state: a search is open; the trees have been searched
    gr, pl = M.arrays([make_board("othello", 6, 6)] * 8)
    eng.set_roots(gr, pl)
    eng.search_begin(4)
    assert L.az_engine_set_exact_endgame(eng.h, 6) == _lib.AZ_ESTATE
    assert L.az_engine_exact_endgame_stats(eng.h, C.byref(C.c_int64()), C.byref(C.c_int64())) == _lib.AZ_ESTATE
    eng.search_end()
    assert L.az_engine_set_exact_endgame(eng.h, 6) == _lib.AZ_ESTATE and b"searched trees" in L.az_last_error()
    eng.set_roots(gr, pl)
    eng.set_exact_endgame(6)
    eng.search(4)
    assert L.az_engine_set_exact_endgame(eng.h, 3) == _lib.AZ_ESTATE and L.az_engine_set_exact_endgame(eng.h, 0) == _lib.AZ_ESTATE
    assert L.az_engine_set_exact_endgame(eng.h, 6) == _lib.AZ_OK  # no change: nothing to refuse
    eng.set_roots(gr, pl)
    eng.set_exact_endgame(None)
    eng.close()
    net.close()
