"""CPU: the host-side mirror classes against what the Python reference's own classes do, and the committed golden fixtures against
what the reference produces.  The reference's side is recorded under tests/golden/ (live_boards_<tag>.npz, live_nets.npz,
live_reference.json) by tools/gen_live_fixtures.py where the reference is mounted; these tests need only the repository."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, golden
from tools.gen_live_fixtures import FIXTURE_PLAN, move_key, sha, tensor_sha


@pytest.fixture(scope="module")
def LIVE():
    """the reference's side of the comparisons (tools/gen_live_fixtures.py)"""
    with open(os.path.join(GOLD, "live_reference.json")) as f:
        return json.load(f)


def _board(tag):
    from alphazero_amd.games.connect4 import Connect4Board
    from alphazero_amd.games.othello import OthelloBoard
    from alphazero_amd.games.tictactoe import TicTacToeBoard
    if tag.startswith("othello"):
        return OthelloBoard(n=int(tag[-1]))
    if tag.startswith("connect4"):
        w, h = (7, 6) if tag == "connect4" else map(int, tag.split("_")[1].split("x"))
        return Connect4Board(width=w, height=h)
    return TicTacToeBoard()


@pytest.mark.parametrize("tag", ["othello8", "othello6", "othello4", "connect4", "connect4_5x6", "connect4_8x8", "connect4_4x4", "tictactoe"])
def test_boards_side_by_side(tag):
    """12 random playouts: every position of the mirror equals the reference's (grid, player, score, game over, winner), and so do the
    move lists -- in the same ORDER too: a seeded np.random picks the same get_random_move on both"""
    fx = golden(f"live_boards_{tag}.npz")
    mo, oo, d = fx["moves_off"], fx["other_off"], fx["moves"].shape[1]
    rng = np.random.RandomState(7)
    p = 0
    for game in range(12):
        mine = _board(tag)
        while True:
            assert mine.is_game_over() == bool(fx["over"][p])
            assert np.array_equal(np.asarray(mine.grid), fx["grids"][p]) and mine.player == fx["players"][p]
            assert np.array_equal(np.atleast_1d(np.asarray(mine.get_score(), dtype=np.float64)), fx["scores"][p])
            if fx["over"][p]:
                assert mine.get_winner() == fx["winners"][game]
                p += 1
                break
            b = mine.get_moves()
            assert np.array_equal(np.array([move_key(tag, m) for m in b], np.int32).reshape(-1, d), fx["moves"][mo[p]:mo[p + 1]])
            other = sorted(move_key(tag, m) for m in mine.get_moves(player=-mine.player))
            assert np.array_equal(np.array(other, np.int32).reshape(-1, d), fx["other"][oo[p]:oo[p + 1]])
            i = rng.randint(len(b))
            assert i == fx["picks"][p]
            mv = b[i]
            assert fx["legal"][p] and mine.is_legal_move(mv)
            mine.play_move(mv)
            p += 1
    assert p == len(fx["players"])


@pytest.mark.parametrize("tag", ["othello8", "connect4", "tictactoe"])
def test_networks_side_by_side(tag):
    from alphazero_amd.games.connect4 import Connect4Net
    from alphazero_amd.games.othello import OthelloNet
    from alphazero_amd.games.tictactoe import TicTacToeNet
    fx = golden("live_nets.npz")
    torch.manual_seed(4)
    mine = {"othello8": lambda: OthelloNet(n=8), "connect4": lambda: Connect4Net(7, 6), "tictactoe": lambda: TicTacToeNet()}[tag]()
    sm = mine.state_dict()
    assert list(sm.keys()) == list(fx[f"{tag}_keys"])
    assert [tensor_sha(t) for t in sm.values()] == list(fx[f"{tag}_sha"])  # same layer order -> same default initialisation under one seed
    mine.eval()
    x = torch.tensor(np.stack([np.asarray(_board(tag).grid, dtype=np.float32)] * 3))
    lp_m, v_m = mine(x)
    assert torch.allclose(torch.from_numpy(fx[f"{tag}_log_probs"]), lp_m, atol=1e-6)
    assert torch.allclose(torch.from_numpy(fx[f"{tag}_value"]), v_m, atol=1e-6)
    pr = fx[f"{tag}_evaluate_probs"]  # the mirror's evaluate() runs on the HIP engine: compared in the GPU tests through G2
    assert pr.shape[0] == mine.action_size and np.allclose(pr, np.exp(lp_m[0].detach().numpy()), atol=1e-6)


def _same_as_recorded(LIVE, name):
    old = np.load(os.path.join(GOLD, name), allow_pickle=False)
    want = LIVE["fixtures"][name]
    assert sorted(old.files) == sorted(want), name
    for k in old.files:
        assert sha(old[k]) == want[k], (name, k)


@pytest.mark.parametrize("tag,n_games,n_pos,sp", [("tictactoe", 512, 256, (4, 25)), ("othello6", 256, 512, (3, 25))])
def test_committed_fixtures_are_what_the_reference_produces(LIVE, tag, n_games, n_pos, sp):
    """tools/gen_golden.py re-run against the reference (same plan as its main()) reproduced tests/golden/ bit for bit when
    tools/gen_live_fixtures.py recorded it: the committed fixtures still hold exactly those arrays"""
    assert (tag, n_games, n_pos, sp) in FIXTURE_PLAN  # the plan the digests were recorded with
    for kind in ("rules", "net", "mct", "selfplay", "selfplay_frac", "sgd"):
        _same_as_recorded(LIVE, f"{kind}_{tag}.npz")


@pytest.mark.parametrize("tag", ["tictactoe", "connect4", "othello6", "othello8"])
def test_committed_arena_fixtures_are_what_the_reference_produces(LIVE, tag):
    """golden G7 (Arena.play_games of the reference), as regenerated when the digests were recorded"""
    _same_as_recorded(LIVE, f"arena_{tag}.npz")


def test_committed_sgd_fixture_of_the_baseline_network_is_what_the_reference_produces(LIVE):
    """golden G6 for OthelloNet 8x8: the reference's optimize_network on the committed G4 memory"""
    _same_as_recorded(LIVE, "sgd_othello8.npz")


def test_checkpoints_cross_load(LIVE, tmp_path):
    """checkpoint wire format (base.py:288-325, trainer.py:448-473): models/<name>/{config.json,<name>.pt} written by either
    side load into the other and give the same network"""
    from alphazero_amd.games.othello import OthelloConfig, OthelloNet
    rec = LIVE["checkpoint"]
    torch.manual_seed(2)
    mine = OthelloNet(config=OthelloConfig(board_size=6))
    d = os.path.join(tmp_path, "m1")
    mine.save_model("m1", model_path=d)
    json.dump(OthelloConfig(board_size=6).to_dict(), open(os.path.join(d, "config.json"), "w"))
    # the reference's from_pretrained reads config.json into its OthelloConfig and load_state_dict()s torch.load(<name>.pt), strictly:
    # the file must be what its own save_model writes -- the same files, a state dict with its keys in its order and its shapes
    assert sorted(os.listdir(d)) == sorted([f.replace("m2", "m1") for f in rec["files"]] + ["config.json"])
    obj = torch.load(os.path.join(d, "m1.pt"))
    assert type(obj).__name__ == rec["type"] and list(obj.keys()) == rec["keys"] and [list(t.shape) for t in obj.values()] == rec["shapes"]
    assert all(torch.equal(v, obj[k]) for k, v in mine.state_dict().items())
    assert sorted(json.load(open(os.path.join(d, "config.json")))) == sorted(rec["config"])
    # the other way round: what the reference's save_model writes under torch.manual_seed(3) -- torch.save of its state dict, whose
    # tensors are these (same sha256) -- with its config.json; the mirror reads it
    torch.manual_seed(3)
    sd = OthelloNet(config=OthelloConfig(board_size=6)).state_dict()
    assert list(sd.keys()) == rec["keys"] and [tensor_sha(t) for t in sd.values()] == rec["sha"]
    d2 = os.path.join(tmp_path, "m2")
    os.makedirs(d2)
    torch.save(sd, os.path.join(d2, "m2.pt"))
    json.dump(rec["config"], open(os.path.join(d2, "config.json"), "w"))
    mine2 = OthelloNet.from_pretrained("m2", models_path=str(tmp_path))
    assert all(torch.equal(v, mine2.state_dict()[k]) for k, v in sd.items())
    assert mine2.n == 6 and sorted(OthelloConfig(board_size=6).to_dict()) == sorted(rec["config"])


# ---------------------------------------------------------------------------------------------- the public surface
# What the mirror deliberately does not carry, by name -- everything else public in the in-scope modules must exist here with the
# reference's parameter names in the reference's order (extra trailing parameters need defaults):
SURFACE_EXCEPTIONS = {
    # rendering, the interactive player, HF hub and command lines: out of scope
    "players.HumanPlayer", "utils.get_hf_token", "utils.list_models_from_hf_hub", "utils.download_model_from_hf_hub",
    "utils.download_all_models_from_hf_hub", "utils.push_model_to_hf_hub", "utils.get_rgb_code", "timers.demo", "trainer.tests",
    # the host-side tree of the reference: here the tree lives in HBM and these four steps are the device kernels k_step / k_rollout_step
    # (csrc/az_engine.hip); MCT keeps search / get_action_probs / get_prior_probs / change_root / reset, which is what Players call
    "mcts.Node", "mcts.MCT.select_node", "mcts.MCT.rollout", "mcts.MCT.nn_evaluation", "mcts.MCT.back_propagate",
}


def test_public_surface_matches(LIVE):
    """every recorded public function / method of the reference (parameters as [name, literal default or None, kind]) against the mirror"""
    import importlib
    problems = []
    VAR = (inspect.Parameter.VAR_KEYWORD, inspect.Parameter.VAR_POSITIONAL)

    def compare(label, rparams, mf):
        rp, mp = {n: dflt for n, dflt, _ in rparams}, inspect.signature(mf).parameters
        rn, mn = [n for n, _, _ in rparams], list(mp)
        if mn[:len(rn)] != rn:
            problems.append(f"{label}: reference {rn}, mirror {mn}")
            return
        for extra in mn[len(rn):]:
            if mp[extra].default is inspect.Parameter.empty and mp[extra].kind not in VAR:
                problems.append(f"{label}: extra mirror parameter {extra} has no default")
        for name in rn:
            if (rp[name] is None) != (mp[name].default is inspect.Parameter.empty) and name != "self":
                problems.append(f"{label}: parameter {name} is {'required' if rp[name] is None else 'optional'} in the reference")
            elif rp[name] is not None and rp[name]["type"] != "other":
                rd, md = rp[name], mp[name].default
                if type(md).__name__ != rd["type"] or md != rd["value"]:  # literal defaults must be the reference's
                    problems.append(f"{label}: parameter {name} defaults to {rd['value']!r} in the reference, {md!r} here")

    for mod, entries in LIVE["surface"].items():
        mine = importlib.import_module("alphazero_amd." + mod)
        for name, obj in entries.items():
            label = f"{mod}.{name}"
            if label in SURFACE_EXCEPTIONS:
                continue
            if obj["what"] == "function":
                if not hasattr(mine, name):
                    problems.append(f"{label}: missing")
                else:
                    compare(label, obj["params"], getattr(mine, name))
                continue
            if not hasattr(mine, name):
                problems.append(f"{label}: missing")
                continue
            ours = getattr(mine, name)
            for meth, r in obj["methods"].items():
                ml = f"{label}.{meth}"
                if ml in SURFACE_EXCEPTIONS or meth in ("human_display", "pixel_display"):  # rendering: the base class refuses both
                    continue
                attr = inspect.getattr_static(ours, meth, None)
                if attr is None:
                    problems.append(f"{ml}: missing")
                    continue
                mkind = type(attr).__name__ if isinstance(attr, (staticmethod, classmethod)) else "function"
                mf = attr.__func__ if isinstance(attr, (staticmethod, classmethod)) else attr
                if not inspect.isfunction(mf):
                    problems.append(f"{ml}: not a function here")
                elif mkind != r["kind"]:
                    problems.append(f"{ml}: {r['kind']} in the reference, {mkind} here")
                else:
                    compare(ml, r["params"], mf)
    assert not problems, "\n".join(problems)


def test_abstract_hooks_raise_like_the_reference(LIVE):
    """base.py:370-397: a hook a concrete network does not define is a NotImplementedError, not an AttributeError"""
    from alphazero_amd.arena import Arena
    from alphazero_amd.games.connect4 import Connect4Net
    assert LIVE["hooks"]["Connect4Net.rotate_neural_output"] == "NotImplementedError"
    with pytest.raises(NotImplementedError):
        Connect4Net(7, 6).rotate_neural_output(np.zeros(7), 1)
    # a positional call binds as in the reference: play_game(False, False, False, True) asks for the results
    assert list(inspect.signature(Arena.play_game).parameters)[:5] == ["self", "player2_starts", "display", "save_frames", "return_results"]


def test_config_dataclasses_have_the_references_fields_and_defaults(LIVE):
    """base.py:60-92 and games/*.py: the JSON configs of the reference load unchanged only if every field exists here under the same
    name with the same default, in the same order (positional construction)"""
    import dataclasses
    from alphazero_amd import base as mbase
    from alphazero_amd.games import connect4 as mc4, othello as moth, tictactoe as mttt
    mine = {"base.Config": mbase.Config, "othello.OthelloConfig": moth.OthelloConfig, "connect4.Connect4Config": mc4.Connect4Config,
            "tictactoe.TicTacToeConfig": mttt.TicTacToeConfig}
    assert sorted(LIVE["configs"]) == sorted(mine)
    for label, ref in LIVE["configs"].items():
        rf = [tuple(x) for x in ref["fields"]]
        mf = [(f.name, repr(f.default)) for f in dataclasses.fields(mine[label])]
        assert rf == mf, (label, [x for x in rf if x not in mf], [x for x in mf if x not in rf])
        assert ref["to_dict"] == {k: repr(v) for k, v in dict(mine[label]().to_dict()).items()}, label


def test_registers_have_the_references_keys(LIVE):
    """games/registers.py: the same games, the same per-game entries (class names) and the same augmentation strategies"""
    import alphazero_amd.games.registers as mreg
    rreg = LIVE["registers"]
    for name in ("GAMES_SET", "CONFIGS_REGISTER", "BOARDS_REGISTER", "NETWORKS_REGISTER", "DATA_AUGMENT_STRATEGIES"):
        b = getattr(mreg, name)
        assert set(rreg[name]) == set(b), name
        if name.endswith("_REGISTER"):
            assert rreg[name + "_classes"] == {k: v.__name__ for k, v in b.items()}, name
    for game, strat in rreg["strategies"].items():
        mine = mreg.DATA_AUGMENT_STRATEGIES[game]
        flat = {k: [t.value for t in (v if isinstance(v, list) else [v])] for k, v in mine.items()}
        assert strat == flat, game
    assert rreg["move_formats"] == {k: v.value for k, v in mreg.MOVE_FORMATS_REGISTER.items()}
