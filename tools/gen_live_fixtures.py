#!/usr/bin/env python3
"""Records what the Python reference does where tests/test_live_reference.py compares the host-side mirror with it (TEST
INFRASTRUCTURE; runs only where the reference is mounted, like tools/gen_golden.py, whose load_reference() it uses).  The tests then
replay the mirror against these records and need no reference:

  live_boards_<tag>.npz  12 random playouts per board (np.random.RandomState(7) picks among get_moves() in the reference's order): every
                         position's grid, player, score, game-over flag, the ordered move list, the other player's move set, the pick, the
                         winners
  live_nets.npz          OthelloNet(n=8) / Connect4Net(7, 6) / TicTacToeNet() under torch.manual_seed(4): state_dict key order and a
                         sha256 of every tensor, the eval-mode forward of the start position (x3) and evaluate() of it
  live_reference.json    the public surface (parameter names, which have defaults, literal defaults), the config dataclasses' fields,
                         defaults and to_dict(), the registers, the abstract-hook behaviour, the checkpoint layout save_model writes, and
                         a sha256 of every array gen_golden.py regenerates for the committed fixtures (G1-G7 plan of the tests)

Usage: python tools/gen_live_fixtures.py
"""
import dataclasses
import hashlib
import importlib
import inspect
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from tools import gen_golden  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
BOARD_TAGS = ["othello8", "othello6", "othello4", "connect4", "connect4_5x6", "connect4_8x8", "connect4_4x4", "tictactoe"]
NET_TAGS = ["othello8", "connect4", "tictactoe"]
SURFACE_MODULES = ["base", "arena", "mcts", "players", "trainer", "schedulers", "timers", "utils", "games.othello", "games.connect4",
                   "games.tictactoe", "games.registers"]
# gen_golden's plans that test_live_reference re-ran against the reference: (tag, n_games, n_positions, self-play plan)
FIXTURE_PLAN = [("tictactoe", 512, 256, (4, 25)), ("othello6", 256, 512, (3, 25))]
ARENA_TAGS = ["tictactoe", "connect4", "othello6", "othello8"]


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def tensor_sha(t):
    return sha(t.detach().cpu().numpy())


def move_key(tag, m):
    return [int(m)] if tag.startswith("connect4") else [int(m[0]), int(m[1])]


def ref_board(R, tag):
    if tag.startswith("othello"):
        return R.oth.OthelloBoard(n=int(tag[-1]))
    if tag.startswith("connect4"):
        w, h = (7, 6) if tag == "connect4" else map(int, tag.split("_")[1].split("x"))
        return R.c4.Connect4Board(width=w, height=h)
    return R.ttt.TicTacToeBoard()


def gen_boards(R, tag):
    rng = np.random.RandomState(7)
    rec = {k: [] for k in ("grids", "players", "scores", "over", "picks", "legal")}
    moves, other, moves_off, other_off, winners = [], [], [0], [0], []
    for game in range(12):
        ref = ref_board(R, tag)
        while True:
            over = bool(ref.is_game_over())
            rec["grids"].append(np.asarray(ref.grid).copy())
            rec["players"].append(int(ref.player))
            rec["scores"].append(np.atleast_1d(np.asarray(ref.get_score(), dtype=np.float64)))
            rec["over"].append(over)
            if over:
                winners.append(int(ref.get_winner()))
                rec["picks"].append(-1)
                rec["legal"].append(False)
                moves_off.append(len(moves))
                other_off.append(len(other))
                break
            a = ref.get_moves()
            moves += [move_key(tag, m) for m in a]
            other += sorted(move_key(tag, m) for m in ref.get_moves(player=-ref.player))
            moves_off.append(len(moves))
            other_off.append(len(other))
            i = rng.randint(len(a))
            rec["picks"].append(i)
            rec["legal"].append(bool(ref.is_legal_move(a[i])))
            ref.play_move(a[i])
    d = 1 if tag.startswith("connect4") else 2
    np.savez_compressed(os.path.join(GOLD, f"live_boards_{tag}.npz"), grids=np.stack(rec["grids"]).astype(np.int8),
                        players=np.array(rec["players"], np.int8), scores=np.stack(rec["scores"]), over=np.array(rec["over"]),
                        picks=np.array(rec["picks"], np.int32), legal=np.array(rec["legal"]), winners=np.array(winners, np.int8),
                        moves=np.array(moves, np.int32).reshape(-1, d), moves_off=np.array(moves_off, np.int64),
                        other=np.array(other, np.int32).reshape(-1, d), other_off=np.array(other_off, np.int64))
    print(f"live_boards_{tag}: {len(rec['players'])} positions")


def gen_nets(R):
    out = {}
    for tag in NET_TAGS:
        torch.manual_seed(4)
        ref = {"othello8": lambda: R.oth.OthelloNet(n=8), "connect4": lambda: R.c4.Connect4Net(board_width=7, board_height=6),
               "tictactoe": lambda: R.ttt.TicTacToeNet()}[tag]()
        sd = ref.state_dict()
        ref.eval()
        rb = ref_board(R, tag)
        x = torch.tensor(np.stack([np.asarray(rb.grid, dtype=np.float32)] * 3))
        lp, v = ref(x)
        pr, _ = ref.evaluate(rb)
        out[f"{tag}_keys"] = np.array(list(sd.keys()))
        out[f"{tag}_sha"] = np.array([tensor_sha(t) for t in sd.values()])
        out[f"{tag}_log_probs"] = lp.detach().numpy()
        out[f"{tag}_value"] = v.detach().numpy()
        out[f"{tag}_evaluate_probs"] = np.asarray(pr, dtype=np.float64)
    np.savez_compressed(os.path.join(GOLD, "live_nets.npz"), **out)
    print("live_nets:", NET_TAGS)


def literal(d):
    """a default as the tests compare it: literal bool / int / float / str / None by type and value, anything else only as 'set'"""
    if d is inspect.Parameter.empty:
        return None
    if isinstance(d, (bool, int, float, str, type(None))):
        return {"type": type(d).__name__, "value": d}
    return {"type": "other"}


def params(f):
    return [[name, literal(p.default), p.kind.name] for name, p in inspect.signature(f).parameters.items()]


def functions(cls):
    out = {}
    for name, attr in vars(cls).items():
        if name.startswith("_") and name != "__init__":
            continue
        f = attr.__func__ if isinstance(attr, (staticmethod, classmethod)) else attr
        if inspect.isfunction(f):
            out[name] = {"kind": type(attr).__name__ if isinstance(attr, (staticmethod, classmethod)) else "function", "params": params(f)}
    return out


def gen_surface():
    surface = {}
    for mod in SURFACE_MODULES:
        ref = importlib.import_module("alphazero." + mod)
        entries = {}
        for name, obj in vars(ref).items():
            if getattr(obj, "__module__", None) != ref.__name__ or name.startswith("_") or name == "main":
                continue
            if inspect.isfunction(obj):
                entries[name] = {"what": "function", "params": params(obj)}
            elif inspect.isclass(obj):
                entries[name] = {"what": "class", "methods": functions(obj)}
        surface[mod] = entries
    return surface


def gen_configs(R):
    import alphazero.base as rbase
    out = {}
    for label, cls in (("base.Config", rbase.Config), ("othello.OthelloConfig", R.oth.OthelloConfig),
                       ("connect4.Connect4Config", R.c4.Connect4Config), ("tictactoe.TicTacToeConfig", R.ttt.TicTacToeConfig)):
        out[label] = {"fields": [[f.name, repr(f.default)] for f in dataclasses.fields(cls)],
                      "to_dict": {k: repr(v) for k, v in dict(cls().to_dict()).items()}}
    return out


def gen_registers(R):
    rreg = R.registers
    out = {}
    for name in ("GAMES_SET", "CONFIGS_REGISTER", "BOARDS_REGISTER", "NETWORKS_REGISTER", "DATA_AUGMENT_STRATEGIES"):
        a = getattr(rreg, name)
        out[name] = sorted(a)
        if name.endswith("_REGISTER"):
            out[name + "_classes"] = {k: v.__name__ for k, v in a.items()}
    out["strategies"] = {game: {k: [t.value for t in (v if isinstance(v, list) else [v])] for k, v in strat.items()}
                         for game, strat in rreg.DATA_AUGMENT_STRATEGIES.items()}
    out["move_formats"] = {k: v.value for k, v in rreg.MOVE_FORMATS_REGISTER.items()}
    return out


def gen_hooks(R):
    try:
        R.c4.Connect4Net(7, 6).rotate_neural_output(np.zeros(7), 1)
        raised = None
    except Exception as e:  # noqa: BLE001
        raised = type(e).__name__
    return {"Connect4Net.rotate_neural_output": raised}


def gen_checkpoint(R):
    """what OthelloNet(config=OthelloConfig(board_size=6)).save_model("m2", model_path=d) of the reference writes under torch.manual_seed(3)"""
    torch.manual_seed(3)
    ref = R.oth.OthelloNet(config=R.oth.OthelloConfig(board_size=6))
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "m2")
        ref.save_model("m2", model_path=d)
        files = sorted(os.listdir(d))
        obj = torch.load(os.path.join(d, "m2.pt"))
    return {"files": files, "type": type(obj).__name__, "keys": list(obj.keys()), "shapes": [list(t.shape) for t in obj.values()],
            "sha": [tensor_sha(t) for t in obj.values()], "config": R.oth.OthelloConfig(board_size=6).to_dict()}


def gen_fixture_digests(R):
    """sha256 of every array gen_golden.py writes when re-run against the reference with the tests' plans"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        gen_golden.GOLD = tmp
        for tag, n_games, n_pos, sp in FIXTURE_PLAN:
            positions = gen_golden.gen_rules(R, tag, n_games, seed=1000 + len(tag) + n_games, n_positions=n_pos)
            gen_golden.gen_net(R, tag, positions)
            gen_golden.gen_mct(R, tag, positions)
            gen_golden.gen_selfplay(R, tag, *sp)
            gen_golden.gen_selfplay(R, tag, *sp, seed=11, temp_steps=(2, 6), name="selfplay_frac")
            gen_golden.gen_sgd(R, tag)
        for tag in ARENA_TAGS:
            gen_golden.gen_arena(R, tag)
        for name in sorted(os.listdir(tmp)):
            f = np.load(os.path.join(tmp, name), allow_pickle=False)
            out[name] = {k: sha(f[k]) for k in sorted(f.files)}
    with tempfile.TemporaryDirectory() as tmp:  # G6 of OthelloNet 8x8 on the committed G4 memory
        import shutil
        shutil.copy(os.path.join(GOLD, "selfplay_othello8.npz"), tmp)
        gen_golden.GOLD = tmp
        gen_golden.gen_sgd(R, "othello8")
        f = np.load(os.path.join(tmp, "sgd_othello8.npz"), allow_pickle=False)
        out["sgd_othello8.npz"] = {k: sha(f[k]) for k in sorted(f.files)}
    gen_golden.GOLD = GOLD
    return out


def main():
    R = gen_golden.load_reference()
    for tag in BOARD_TAGS:
        gen_boards(R, tag)
    gen_nets(R)
    rec = {"surface": gen_surface(), "configs": gen_configs(R), "registers": gen_registers(R), "hooks": gen_hooks(R),
           "checkpoint": gen_checkpoint(R), "fixtures": gen_fixture_digests(R)}
    with open(os.path.join(GOLD, "live_reference.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("live_reference.json:", {k: len(v) for k, v in rec.items()})


if __name__ == "__main__":
    main()
