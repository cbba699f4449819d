"""BatchedArena in the search modes without a GPU: the host model of such an arena (tests/arena_modes_model.py) pinned
to the oracle's arena where no mode is on, its apply and opening rules, the refusals of the Python surface -- all before any engine is
created -- and the surface itself."""
import inspect
import os
import re

import pytest

import arena_modes_model as AM
from alphazero_amd import _lib, arena as A
from alphazero_amd.arena import BatchedArena
from conftest import ROOT
from gumbel_full_model import GumbelFullModel
from leaf_batch_model import Model, Node, make_board
from tools import closed_form as cf

GAMES = {"othello6": ("othello", 0, 6, 6), "connect4": ("connect4", 1, 6, 7), "tictactoe": ("tictactoe", 2, 3, 3)}


def same_stats(a, b):
    return (a["draw"] == b["draw"] and a["player1"] == b["player1"] and a["player2"] == b["player2"]
            and dict(a["player1_starts"]) == dict(b["player1_starts"]) and dict(a["player2_starts"]) == dict(b["player2_starts"]))


# ---- the driver is the reference's
@pytest.mark.parametrize("start_player", [None, 1, 2])
@pytest.mark.parametrize("tie", ["lowest", "random"])
@pytest.mark.parametrize("tag", list(GAMES))
def test_without_a_mode_the_model_is_the_oracle_arena(tag, tie, start_player):
    """the model is trusted for the modes only after this: no mode on either side, move for move and stat for stat"""
    from oracle import oracle as O
    game, gid, H, W = GAMES[tag]
    otie = O.TIE_RANDOM if tie == "random" else O.TIE_LOWEST
    for n1, n2 in ((8, 12), (12, 8)):
        ref = O.arena_games((gid, H, W), ("fake", None), n1, ("fake", None), n2, 3, 8, start_player=start_player, tie_mode=otie)
        got = AM.arena_games(game, H, W, n1, n2, 3, 8, start_player=start_player, tie=tie)
        assert got[0] == ref[0], (tag, tie, start_player)
        assert got[1] == ref[1] and got[2] == ref[2] and same_stats(got[3], ref[3])


@pytest.mark.parametrize("kind", ["greedy", "random"])
def test_the_baseline_opponents_are_the_oracle_s(kind):
    from oracle import oracle as O
    ref = O.arena_games((0, 6, 6), ("fake", None), 8, kind, 8, 5, 4, tie_mode=O.TIE_LOWEST)
    got = AM.arena_games("othello", 6, 6, 8, 8, 5, 4, opponent=kind, tie="lowest")
    assert got[0] == ref[0] and same_stats(got[3], ref[3])


# ---- apply
def test_apply_keeps_the_subtree_of_a_move_inside_the_tree():
    m = Model(make_board("othello", 6, 6), tie="lowest", seed=1, game_id=7)
    m.search(24)
    child = max(m.root.children, key=lambda c: c.N)
    before = (child.N, child.Q, [(c.act, c.N, c.Q, c.P) for c in child.children])
    AM.apply(m, child.act)
    assert m.root is child and child.parent is None and (m.ply, m.sim_base) == (1, 0)
    assert (child.N, child.Q, [(c.act, c.N, c.Q, c.P) for c in child.children]) == before and child.N > 1


def test_apply_starts_a_fresh_root_for_a_move_outside_the_tree():
    b = make_board("othello", 6, 6)
    m = Model(b, tie="lowest", seed=1, game_id=7)  # never searched: the root is not expanded
    a = cf.move_to_action("othello", sorted(b.get_moves())[0], 6)
    AM.apply(m, a)
    r = m.root
    assert (r.N, r.Q, r.children, r.evaluated, r.expanded, m.ply) == (0, 0.0, [], False, False, 1)
    want = b.clone()
    want.play_move(cf.action_to_move("othello", a, 6))
    assert (r.board.grid == want.grid).all() and r.board.player == want.player
    # evaluated by the root-prior pass but never walked: the children are not materialised, the move is outside the tree
    m2 = Model(b, tie="lowest", seed=1, game_id=7)
    m2._evaluate(m2.root)
    AM.apply(m2, a)
    assert m2.root.children == [] and not m2.root.evaluated


def test_apply_clears_the_candidate_set():
    m = GumbelFullModel(make_board("othello", 6, 6), K=1, full=False, m=2, tie="lowest", seed=1, game_id=7)
    m.search(8)
    assert len(m.mask) == 2
    AM.apply(m, m.move())
    assert m.mask == [] and m.ply == 1


# ---- opening
def test_the_sampled_move_follows_u_across_the_cumulative_sums():
    counts = [1, 0, 3, 4]  # p = 0.125, 0, 0.375, 0.5; cum = 0.125, 0.125, 0.5, 1.0
    for u, want in ((0.0, 0), (0.1249, 0), (0.125, 2), (0.4999, 2), (0.5, 3), (0.999999, 3)):
        assert AM.sampled_index(counts, u) == want, u
    assert AM.sampled_index(counts, 1.0) == 3       # u beyond the running sum: the last child with p > 0
    assert AM.sampled_index([2, 5, 0], 1.5) == 1
    assert AM.sampled_index([7], 0.0) == 0          # a single child: no draw
    # on a hand-made root, through player_move: the draw is cf.move_sample_u(seed, game id, ply)
    m = Model(make_board("tictactoe", 3, 3), tie="lowest", seed=4, game_id=9, ply=2)
    m.root.expanded = True
    for act, n in ((0, 1), (4, 0), (7, 3), (8, 4)):
        c = Node(act, m.root, 0.25, False)
        c.N = n
        m.root.children.append(c)
    u = cf.move_sample_u(4, 9, 2)
    assert AM.player_move(m, 1.0) == [0, 4, 7, 8][AM.sampled_index(counts, u)]
    assert AM.player_move(m, 0.0) == 8


def test_opening_plies_0_is_none_for_a_visit_based_player():
    for tie in ("lowest", "random"):
        a = AM.arena_games("othello", 6, 6, 8, 12, 2, 4, tie=tie, opening_plies=None)
        b = AM.arena_games("othello", 6, 6, 8, 12, 2, 4, tie=tie, opening_plies=0)
        assert a[0] == b[0] and same_stats(a[3], b[3])
    c = AM.arena_games("othello", 6, 6, 8, 12, 2, 4, tie="lowest", opening_plies=4)
    assert c[0] != a[0] and len({tuple(mv[:4]) for mv in c[0]}) > 2  # a seeded opening: the rounds are different games


def test_a_gumbel_player_draws_during_the_opening_only(monkeypatch):
    from alphazero_amd import gumbel as G
    drawn, real = [], G.gumbel_g

    def recording(seed, gid, ply, action, scale=1.0):
        g = real(seed, gid, ply, action, scale)
        if float(scale) != 0.0:
            drawn.append((ply, float(scale)))
        return g
    monkeypatch.setattr(G, "gumbel_g", recording)
    spec = {"gumbel": {"m": 4, "gumbel_scale": 0.0}}  # the spec says 0: the opening draws at scale 1.0
    kw = dict(search=spec, opponent_search={"gumbel": {"m": 4, "gumbel_scale": 0.5}}, tie="lowest")
    tr2 = []
    g2 = AM.play_round("othello", 6, 6, 1, 6, False, 8, 8, opening_plies=2, trace=tr2, **kw)
    assert {p for p, _ in drawn} == {0, 1} and {sc for p, sc in drawn if p == 0} == {1.0} and {sc for p, sc in drawn if p == 1} == {0.5}
    assert [t[2] for t in tr2[:2]] == [1.0, 0.5] and all(t[2] == 0.0 for t in tr2[2:]) and len(tr2) == len(g2[0]) > 4
    # from ply 2 on every move is the scale-0 move: the best of logit + sigma among the candidates, no draw in it
    del drawn[:]
    tr0 = []
    g0 = AM.play_round("othello", 6, 6, 1, 6, False, 8, 8, opening_plies=0, trace=tr0, **kw)
    assert drawn == [] and all(t[2] == 0.0 for t in tr0)
    # None: the spec's own scale throughout
    del drawn[:]
    AM.play_round("othello", 6, 6, 1, 6, False, 8, 8, opening_plies=None, **kw)
    assert {sc for _, sc in drawn} == {0.5} and len({p for p, _ in drawn}) > 2
    assert AM.opening_scale({"m": 4, "gumbel_scale": 0.5}, 2, 1) == 0.5 and AM.opening_scale({"m": 4, "gumbel_scale": 0.5}, None, 9) == 0.5


# ---- refusals, all before any engine exists
@pytest.fixture
def no_engine(monkeypatch):
    from alphazero_amd import engine as E

    class Boom:
        def __init__(self, *a, **k):
            raise AssertionError("an engine was created")
    monkeypatch.setattr(E, "SelfPlayEngine", Boom)


@pytest.mark.parametrize("kw", [
    dict(search={"gumbell": 4}),
    dict(opponent="random", opponent_search={"leaf_batch": 4}),
    dict(opponent="greedy", opponent_search={}),
    dict(nn="mcts", search={"leaf_batch": 4}),
    dict(nn="mcts", search={"gumbel": 4}),
    dict(nn="mcts", search={"symmetry": "random"}),
    dict(opponent="mcts", opponent_search={"gumbel": 16}),
    dict(search={"gumbel_batch": 4}),
    dict(search={"gumbel_full": True}),
    dict(search={"gumbel": 4, "leaf_batch": 4}),
    dict(search={"gumbel": 17}),
    dict(search={"leaf_batch": 17}),
    dict(search={"symmetry": "sideways"}),
    dict(search={"gumbel": 4, "gumbel_batch": 4, "symmetry": "all"}),
    dict(search=[("gumbel", 4)]),
    dict(game="connect4", search={"symmetry": ("random", [0, 2])}),
    dict(opening_plies=-1),
    dict(opening_plies=2.0),
    dict(opening_plies=True),
    dict(opening_plies="4"),
])
def test_batched_arena_refuses_before_any_engine(no_engine, kw):
    args = dict(game="othello", nn="fake", opponent="fake", n_sim=8, board_size=6)
    args.update(kw)
    with pytest.raises(ValueError):
        BatchedArena(**args)


def test_external_networks_take_no_mode(no_engine):
    import torch
    from alphazero_amd.base import PolicyValueNetwork
    from alphazero_amd.evaluators import route

    class Other(PolicyValueNetwork):
        def __init__(self):
            torch.nn.Module.__init__(self)
    net = Other.__new__(Other)
    torch.nn.Module.__init__(net)
    if route(net) == "hip":
        pytest.skip("this build routes every network to the HIP network")
    for spec in ({"gumbel": 4}, {"leaf_batch": 2}, {"symmetry": "random"}):
        with pytest.raises(ValueError, match="external evaluator"):
            BatchedArena("othello", net, opponent="random", n_sim=8, board_size=6, search=spec)


def test_the_reused_messages_are_the_players():
    with pytest.raises(ValueError, match="needs eval_method 'neural'"):
        BatchedArena("othello", "mcts", n_sim=8, board_size=6, search={"gumbel": 4})
    with pytest.raises(ValueError, match="gumbel does not combine with leaf_batch=4"):
        BatchedArena("othello", "fake", n_sim=8, board_size=6, search={"gumbel": 4, "leaf_batch": 4})
    with pytest.raises(ValueError, match="needs the Gumbel root search"):
        BatchedArena("othello", "fake", n_sim=8, board_size=6, search={"gumbel_batch": 4})


def _trainer(**kw):
    from alphazero_amd.trainer import AlphaZeroTrainer
    return AlphaZeroTrainer(verbose=False, engine_slots=8, seed=1, materialize_memory=False, **kw)


def test_trainer_refuses_eval_search_on_the_host_arena_path(no_engine):
    from alphazero_amd.games.othello import OthelloConfig
    for kw in (dict(eval_search="selfplay", selfplay_gumbel=4), dict(eval_search={"leaf_batch": 4}), dict(eval_opening_plies=2)):
        tr = _trainer(**kw)
        tr.game = "othello"
        tr.config = OthelloConfig(board_size=6, simulations=None, compute_time=0.01, do_eval=True, eval_opponent="greedy", eval_episodes=2)
        with pytest.raises(ValueError, match="config.simulations"):
            tr.setup()
    for kw in (dict(eval_search="self-play"), dict(eval_search={"gumbel_batch": 4}), dict(eval_search={"nope": 1}), dict(eval_opening_plies=-2),
               dict(eval_search="selfplay", eval_opening_plies=1.5)):
        with pytest.raises(ValueError):
            _trainer(**kw)
    tr = _trainer(selfplay_symmetry="random", selfplay_gumbel=8, selfplay_gumbel_batch=4, selfplay_gumbel_full=True, eval_search="selfplay")
    assert tr._eval_search_spec() == {"symmetry": "random", "gumbel": 8, "gumbel_batch": 4, "gumbel_full": True}
    assert _trainer()._eval_search_spec() is None


# ---- surface
def test_the_export_and_the_keywords_are_there():
    header = open(os.path.join(ROOT, "include", "az_amd.h")).read()
    assert re.search(r"int az_engine_player_moves\(az_engine \*e, double temp, int32_t \*h_actions\);", header)
    assert "az_engine_player_moves" in _lib.SYMBOLS
    src = open(os.path.join(ROOT, "alphazero_amd", "_lib.py")).read()
    assert "L.az_engine_player_moves.argtypes = [vp, C.c_double, vp]" in src
    from alphazero_amd.engine import SelfPlayEngine
    assert inspect.signature(SelfPlayEngine.player_moves).parameters["temp"].default == 0.0
    names = list(inspect.signature(BatchedArena.__init__).parameters)
    assert names[-3:] == ["search", "opponent_search", "opening_plies"]
    assert all(inspect.signature(BatchedArena.__init__).parameters[n].default is None for n in names[-3:])
    from alphazero_amd.trainer import AlphaZeroTrainer
    names = list(inspect.signature(AlphaZeroTrainer.__init__).parameters)
    assert names[-2:] == ["eval_search", "eval_opening_plies"]
    assert all(inspect.signature(AlphaZeroTrainer.__init__).parameters[n].default is None for n in names[-2:])
    assert A.SEARCH_KEYS == ("symmetry", "leaf_batch", "gumbel", "gumbel_batch", "gumbel_full")
