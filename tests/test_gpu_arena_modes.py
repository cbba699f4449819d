"""GPU: BatchedArena and the trainer's evaluation in every search mode.

  1. az_engine_player_moves: best_moves() with the mode off at temperature 0, root_readout's action at every temperature and in the
     Gumbel mode, the move advance() plays, -1 for slots not served, read-only, its refusals;
  2. the arena against the host model (tests/arena_modes_model.py) move for move with equal stats, every pairing with and without a
     seeded opening, overlapped and serial searches;
  3. the HIP network with one random symmetry per evaluation, and rounds played alone: the draws follow the game, not the slot;
  4. with the three keywords None the arena is the one built without naming them;
  5. plain launches against graph replay across the one set_gumbel of the opening;
  6. the trainer's evaluation with eval_search / eval_opening_plies equals the arena built by hand."""
import math

import numpy as np
import pytest
import torch

import arena_modes_model as AM
from alphazero_amd import base, engine as E, symmetry as S
from alphazero_amd._lib import AzError
from alphazero_amd.arena import BatchedArena
from gumbel_model import playout
from leaf_batch_model import make_board
from tools import closed_form as cf

pytestmark = pytest.mark.gpu

GAMES = {"othello6": ("othello", 0, 6, 6), "connect4": ("connect4", 1, 6, 7), "tictactoe": ("tictactoe", 2, 3, 3)}
TIES = {"lowest": E.TIE_LOWEST, "random": E.TIE_RANDOM}


def same_stats(a, b):
    return (a["draw"] == b["draw"] and sorted(a["player1"]) == sorted(b["player1"]) and sorted(a["player2"]) == sorted(b["player2"])
            and dict(a["player1_starts"]) == dict(b["player1_starts"]) and dict(a["player2_starts"]) == dict(b["player2_starts"]))


def games_of(arena, n):
    return [[int(m[g]) for m in arena.moves if m[g] >= 0] for g in range(n)]


# ------------------------------------------------------------------------------------------------------------------ 1
def arena_engine(tie, n_slots=37, seed=3, finish=True):
    """a 37-slot Othello 6x6 engine in arena mode on mid-game roots of mixed plies: even slots search for +1, odd ones for -1, so about
    half are not to move; the last three are brought one move from the end and finished with play()"""
    rng = np.random.default_rng(11)
    roots = []
    while len(roots) < n_slots:
        b = playout("othello", 6, 6, rng, int(rng.integers(0, 12)))
        if b is not None:
            roots.append(b)
    finals = []
    for i in range(3 if finish else 0):
        while True:
            b, last = make_board("othello", 6, 6), None
            while not b.is_game_over():
                moves = sorted(b.get_moves(), key=lambda m: cf.move_to_action("othello", m, 6))
                mv = moves[int(rng.integers(len(moves)))]
                last = (b.clone(), cf.move_to_action("othello", mv, 6))
                b.play_move(mv)
            if last is not None:
                break
        roots[n_slots - 1 - i] = last[0]
        finals.append((n_slots - 1 - i, last[1]))
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=n_slots, n_sim=16, evaluator=E.EVAL_FAKE, dirichlet_alpha=None, dirichlet_epsilon=None,
                           temp_max_step=-1, temp_min_step=0, tie_mode=TIES[tie], noise_mode=E.NOISE_OFF, seed=seed, max_plies=160,
                           sample_capacity=4 * n_slots)
    eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8),
                  game_ids=(500 + np.arange(n_slots)).astype(np.uint32), plies=np.arange(n_slots, dtype=np.int32) % 7)
    sides = np.where(np.arange(n_slots) % 2 == 0, 1, -1).astype(np.int8)
    eng.set_sides(sides)
    to_move = np.array([b.player for b in roots], np.int8) == sides
    if finals:
        mv = np.full(n_slots, -1, np.int32)
        for s, a in finals:
            mv[s] = a
            to_move[s] = False
        eng.play(mv)
    return eng, to_move


@pytest.mark.parametrize("tie", ["lowest", "random"])
def test_player_moves_is_best_moves_and_the_readout_s_action(tie):
    eng, to_move = arena_engine(tie)
    assert (eng.player_moves() == -1).all()  # no root is expanded yet
    eng.search(16)
    best = eng.best_moves()
    assert np.array_equal(eng.player_moves(0.0), best) and np.array_equal(eng.player_moves(), best)
    assert np.array_equal(best >= 0, to_move) and to_move.sum() > 8 and (~to_move).sum() > 8
    _, over, _, _ = eng.root_status()
    assert over[-3:].all() and (best[-3:] == -1).all()
    seen = []
    for temp in (0.0, 0.5, 1.0):
        want = eng.root_readout(temps=temp)["action"].cpu().numpy()
        got = eng.player_moves(temp)
        assert got.dtype == np.int32 and np.array_equal(got, want), temp
        assert np.array_equal(got >= 0, to_move)
        seen.append(got)
    assert not np.array_equal(seen[0], seen[2])  # the sampled move is another one somewhere
    assert eng.stats()["error_flags"] == 0
    eng.close()


def test_player_moves_in_the_gumbel_mode_is_the_move_advance_plays():
    n = 37
    rng = np.random.default_rng(5)
    roots = []
    while len(roots) < n:
        b = playout("othello", 6, 6, rng, int(rng.integers(0, 12)))
        if b is not None:
            roots.append(b)
    eng = E.SelfPlayEngine(0, 6, 6, n_slots=n, n_sim=16, evaluator=E.EVAL_FAKE, dirichlet_alpha=None, dirichlet_epsilon=None,
                           tie_mode=E.TIE_LOWEST, noise_mode=E.NOISE_OFF, seed=7, max_plies=160, sample_capacity=4 * n)
    eng.set_gumbel(16)
    eng.set_roots(np.array([b.grid for b in roots], np.int8), np.array([b.player for b in roots], np.int8),
                  game_ids=(900 + np.arange(n)).astype(np.uint32))
    eng.search(16)
    want = eng.root_readout(temps=0)["action"].cpu().numpy()
    for temp in (0.0, 0.5, 1.0):  # the Gumbel move, whatever the temperature
        assert np.array_equal(eng.player_moves(temp), want), temp
    assert (want >= 0).all() and not np.array_equal(want, eng.best_moves())  # best_moves() is another player's move
    eng.advance()
    meta = eng.samples()["meta"].cpu().numpy()
    played = {int(g): int(a) for g, _, _, a in meta}
    assert [played[900 + i] for i in range(n)] == want.tolist()
    assert eng.stats()["error_flags"] == 0
    eng.close()


def test_player_moves_changes_nothing():
    outs = []
    for call in (False, True):
        eng, _ = arena_engine("random", finish=False)
        eng.search(16)
        if call:
            for temp in (0.0, 1.0, 0.25):
                eng.player_moves(temp)
        eng.search(12)
        ro = {k: v.cpu().numpy() for k, v in eng.root_readout(temps=1.0, pv_len=4).items()}
        outs.append((ro, eng.stats()))
        eng.close()
    for k in outs[0][0]:
        assert np.array_equal(outs[0][0][k].view(np.uint8), outs[1][0][k].view(np.uint8)), k
    assert outs[0][1] == outs[1][1]


def test_player_moves_refusals():
    eng, _ = arena_engine("lowest", n_slots=4, finish=False)
    for bad in (-1.0, -1e-300, math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="negative or not finite"):
            eng.player_moves(bad)
    from alphazero_amd._lib import AZ_EINVAL, lib
    assert lib().az_engine_player_moves(eng.h, 0.0, None) == AZ_EINVAL and lib().az_engine_player_moves(None, 0.0, None) == AZ_EINVAL
    eng.search_begin(4)
    with pytest.raises(AzError, match="has not been ended"):
        eng.player_moves(0.0)
    eng.search_end()
    assert eng.player_moves(1e300).shape == (4,)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ 2
PAIRINGS = {
    "gumbel16_vs_puct": ({"gumbel": 16}, "fake", None, "lowest"),
    "gumbel4x4full_vs_leafbatch4": ({"gumbel": 4, "gumbel_batch": 4, "gumbel_full": True}, "fake", {"leaf_batch": 4}, "random"),
    "gumbel16x16full_vs_gumbel16": ({"gumbel": 16, "gumbel_batch": 16, "gumbel_full": True}, "fake",
                                    {"gumbel": 16, "gumbel_batch": 1, "gumbel_full": False}, "lowest"),
    "leafbatch8_vs_greedy": ({"leaf_batch": 8}, "greedy", None, "lowest"),
    "leafbatch8_vs_random": ({"leaf_batch": 8}, "random", None, "random"),
}
ROUNDS = {"othello6": 8, "tictactoe": 8, "connect4": 4}
_MODEL = {}


def model_games(tag, pairing, opening, seed=2, rounds=None):
    key = (tag, pairing, opening, seed, None if rounds is None else tuple(rounds))
    if key not in _MODEL:  # computed once, shared by the overlapped and the serial arena
        game, _, H, W = GAMES[tag]
        search, opp, opp_search, tie = PAIRINGS[pairing]
        _MODEL[key] = AM.arena_games(game, H, W, 16, 12, seed, ROUNDS[tag], search=search, opponent=opp, opponent_search=opp_search,
                                     opening_plies=opening, tie=tie, rounds=rounds)
    return _MODEL[key]


def run_arena(tag, pairing, opening, overlap, seed=2):
    game, _, H, W = GAMES[tag]
    search, opp, opp_search, tie = PAIRINGS[pairing]
    arena = BatchedArena(game, "fake", opponent=opp, n_sim=16, opponent_n_sim=12, seed=seed, board_size=6, search=search,
                         opponent_search=opp_search, opening_plies=opening)
    arena.tie_mode, arena.overlap = TIES[tie], overlap
    stats = arena.play_games(ROUNDS[tag], return_stats=True, record_moves=True)
    assert all(st["error_flags"] == 0 for st in arena.engine_stats)
    return games_of(arena, ROUNDS[tag]), stats, arena


@pytest.mark.parametrize("pairing", list(PAIRINGS))
@pytest.mark.parametrize("tag", list(GAMES))
def test_the_arena_equals_the_model(tag, pairing):
    for opening in (None, 3):
        moves, _, _, mstats = model_games(tag, pairing, opening)
        for overlap in (True, False):
            got, stats, _ = run_arena(tag, pairing, opening, overlap)
            for g in range(ROUNDS[tag]):
                assert got[g] == moves[g], (tag, pairing, opening, overlap, g)
            assert same_stats(stats, mstats), (tag, pairing, opening, overlap)
    assert model_games(tag, pairing, None)[0] != model_games(tag, pairing, 3)[0]
    if tag == "othello6":  # the eight rounds go through a forced pass (action 36): passes count as plies of the opening
        assert any(36 in mv for mv in model_games(tag, pairing, 3)[0])


# ------------------------------------------------------------------------------------------------------------------ 3
def othello6_nets():
    from alphazero_amd.games.othello import OthelloNet
    out = []
    for seed in (31, 32):
        torch.manual_seed(seed)
        net = OthelloNet(n=6, device="cuda").eval()
        out.append((net, net.to_hip(max_batch=8)))
    return out


def test_the_hip_network_with_a_random_symmetry_follows_the_game_not_the_slot():
    (net1, hip1), (net2, hip2) = othello6_nets()
    members = S.members("othello", 6, 6, "all")

    def plain(hip):
        def net(grid, player, A):
            x = torch.tensor((player * np.asarray(grid)).astype(np.float32).reshape(1, -1), device="cuda")
            p, v = hip.forward(x)
            return p[0].cpu().numpy(), float(v[0].cpu())
        return net

    def drawn(model):  # every row in the one member drawn for (seed, game id, root ply, the row's simulation)
        def net(grid, player, A):
            code = S.random_code(model.seed, model.gid, model.ply, model.s, members)
            x = torch.tensor((player * np.asarray(grid)).astype(np.float32).reshape(1, -1), device="cuda")
            p, v = hip1.forward_sym_codes(x, [code])
            return p[0].cpu().numpy(), float(v[0].cpu())
        return net
    search = {"gumbel": 16, "gumbel_batch": 4, "gumbel_full": True, "symmetry": "random"}
    kw = dict(opponent=net2, n_sim=16, opponent_n_sim=12, seed=4, board_size=6, search=search, opening_plies=3)
    arena = BatchedArena("othello", net1, **kw)
    arena.tie_mode = E.TIE_LOWEST
    stats = arena.play_games(4, return_stats=True, record_moves=True)
    got = games_of(arena, 4)
    moves, _, _, mstats = AM.arena_games("othello", 6, 6, 16, 12, 4, 4, search=search, opponent="net", opening_plies=3, tie="lowest",
                                         bind1=drawn, net2=plain(hip2))
    assert got == moves and same_stats(stats, mstats)
    # rounds {0..7} at once, and rounds {5, 2} alone in slots 0 and 1
    arena = BatchedArena("othello", net1, **kw)
    arena.tie_mode = E.TIE_LOWEST
    arena.play_games(8, record_moves=True)
    eight = games_of(arena, 8)
    assert eight[:4] == got  # ... and no function of the number of rounds
    side = np.array([-1, 1], np.int8)  # round 5 is started by player 2, round 2 by player 1
    arena.moves = []
    arena._play(2, side, np.array([5, 2], np.uint32), record_moves=True)
    assert games_of(arena, 2) == [eight[5], eight[2]]
    hip1.close(); hip2.close()


# ------------------------------------------------------------------------------------------------------------------ 4
def test_off_is_off():
    runs = []
    for kw in ({}, dict(search=None, opponent_search=None, opening_plies=None)):
        for opp in ("fake", "greedy"):
            arena = BatchedArena("othello", "fake", opponent=opp, n_sim=16, opponent_n_sim=12, seed=6, board_size=6, **kw)
            stats = arena.play_games(8, return_stats=True, record_moves=True)
            runs.append(([m.tolist() for m in arena.moves], arena.engine_stats, {k: (dict(v) if hasattr(v, "items") else v) for k, v in stats.items()}))
            assert arena._modes is False
    assert runs[0] == runs[2] and runs[1] == runs[3]
    # an empty dict is a mode request: the same players, their moves through player_moves()
    arena = BatchedArena("othello", "fake", opponent="fake", n_sim=16, opponent_n_sim=12, seed=6, board_size=6, search={})
    arena.play_games(8, record_moves=True)
    assert arena._modes is True and [m.tolist() for m in arena.moves] == runs[0][0]


# ------------------------------------------------------------------------------------------------------------------ 5
def test_plain_launches_equal_graph_replay_across_the_switch_of_the_opening(monkeypatch):
    outs = []
    for graphs in ("1", "0"):
        monkeypatch.setenv("AZ_ENGINE_GRAPHS", graphs)  # read when an engine is created
        got, stats, arena = run_arena("othello6", "gumbel4x4full_vs_leafbatch4", 3, True)
        assert (arena.engine_stats[0]["graph_replays"] > 0) == (graphs == "1")
        outs.append((got, {k: (dict(v) if hasattr(v, "items") else v) for k, v in stats.items()}))
    assert outs[0] == outs[1]
    assert outs[0][0] == model_games("othello6", "gumbel4x4full_vs_leafbatch4", 3)[0]


# ------------------------------------------------------------------------------------------------------------------ 6
def test_the_trainer_evaluates_in_the_modes_of_its_self_play(tmp_path):
    from alphazero_amd.games.othello import OthelloConfig
    from alphazero_amd.trainer import AlphaZeroTrainer
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    spec = {"symmetry": None, "gumbel": 8, "gumbel_batch": 4, "gumbel_full": True}

    def trainer(opponent, **kw):
        tr = AlphaZeroTrainer(verbose=False, engine_slots=8, seed=3, materialize_memory=False, selfplay_gumbel=8, selfplay_gumbel_batch=4,
                              selfplay_gumbel_full=True, **kw)
        tr.game = "othello"
        tr.config = OthelloConfig(board_size=6, simulations=8, episodes=8, epochs=1, batch_size=32, iterations=1, do_eval=True,
                                  eval_opponent=opponent, eval_episodes=8, device="cuda")
        torch.manual_seed(2)
        tr.setup()
        return tr

    def by_hand(tr, opponent, it, **kw):
        arena = BatchedArena("othello", tr.nn, opponent=opponent, n_sim=8, seed=tr.seed + it, board_size=6, **kw)
        stats = arena.play_games(8, return_stats=True)
        return {k: dict(v) for k, v in stats.items() if k.endswith("_starts")}

    tr = trainer("previous", eval_search="selfplay", eval_opening_plies=2)
    first = tr.nn
    tr.self_play(0); tr.optimize_network(0); tr.update_network(0)
    tr.evaluate(0)
    res = tr.eval_results["results"][0]
    assert sum(sum(v.values()) for v in res.values()) == 8
    assert res == by_hand(tr, first, 0, search=spec, opponent_search=spec, opening_plies=2)
    tr.config.eval_opponent = "greedy"
    tr.evaluate(1)
    assert tr.eval_results["results"][1] == by_hand(tr, "greedy", 1, search=spec, opening_plies=2)
    # eval_search None: today's evaluation, on the same two networks
    tr.eval_search, tr.eval_opening_plies = None, None
    tr.config.eval_opponent = "previous"
    tr.evaluate(2)
    assert tr.eval_results["results"][2] == by_hand(tr, first, 2)
