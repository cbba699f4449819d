"""Round-3 GPU tests: BASELINE config 5 (the trainer loop on Othello 8x8) against the oracle, the self-launching multi-rank bench in
rehearsal mode, and the single-game MCT's device storage (reset across boards, searches accumulating on one root)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import oracle as O
from alphazero_amd import base
from alphazero_amd.games.othello import OthelloBoard, OthelloConfig
from alphazero_amd.trainer import AlphaZeroTrainer

pytestmark = pytest.mark.gpu


def _np_sd(module):
    return {k: v.detach().cpu().numpy().copy() for k, v in module.state_dict().items() if not k.endswith("num_batches_tracked")}


def test_config5_train_loop_on_othello8_equals_oracle(tmp_path):
    """BASELINE config 5 (trainer.py:475-572) through AlphaZeroTrainer.train() on Othello 8x8, reduced episodes, 2 iterations,
    evaluation against the PREVIOUS network: iteration-1 samples == the oracle's self-play with the TRAINED weights, every evaluation
    game == the oracle's arena between the two networks of that iteration, files written."""
    base.DEFAULT_MODELS_PATH = str(tmp_path) + "/"
    cfg = OthelloConfig(board_size=8, simulations=12, episodes=12, epochs=1, batch_size=64, iterations=2, do_eval=True, eval_opponent="previous",
                        eval_episodes=4, device="cuda", save=True, save_checkpoints=True)
    path = os.path.join(tmp_path, "cfg.json")
    json.dump(cfg.to_dict(), open(path, "w"))
    tr = AlphaZeroTrainer(verbose=False, engine_slots=16, seed=11, materialize_memory=False)
    snaps, evals = [], []
    orig_update, orig_eval = tr.update_network, tr.evaluate

    def update_network(it):
        orig_update(it)
        snaps.append((_np_sd(tr.prev_nn), _np_sd(tr.nn)))  # (the network self-play used, the trained one)

    def evaluate(it):
        orig_eval(it)
        evals.append(dict(tr.eval_results["results"][it]))
    tr.update_network, tr.evaluate = update_network, evaluate
    samples = []
    orig_sp = tr.self_play

    def self_play(it):
        orig_sp(it)
        samples.append({k: v.cpu().numpy().copy() for k, v in tr.device_samples.items()})
    tr.self_play = self_play
    torch.manual_seed(3)
    tr.train(game="othello", experiment_name="o8", json_config_file=path)
    assert len(snaps) == 2 and len(samples) == 2
    tk = dict(temp_max_step=cfg.temp_max_step, temp_min_step=cfg.temp_min_step)
    for it in range(2):
        played_with = snaps[it][0]
        ref = O.selfplay(O.OTHELLO, 8, 8, 12, 12, ("conv", O.ConvNet(O.OTHELLO, 8, 8, played_with)), seed=11, first_game_id=12 * it, **tk)
        got = samples[it]
        assert np.array_equal(got["state"], ref["state"]) and np.array_equal(got["pi"], ref["pi"]) and np.array_equal(got["z"], ref["z"]), it
        assert np.array_equal(got["visits"], ref["visits"]) and np.array_equal(got["meta"][:, 0] + 12 * it, ref["meta"][:, 0])
        # evaluation: the trained network (player 1) against the one it replaced, BatchedArena seed = trainer seed + iteration
        new, old = snaps[it][1], snaps[it][0]
        _, _, _, ostats = O.arena_games((O.OTHELLO, 8, 8), ("conv", O.ConvNet(O.OTHELLO, 8, 8, new)), 12, ("conv", O.ConvNet(O.OTHELLO, 8, 8, old)), 12,
                                        seed=11 + it, n_rounds=4)
        want = {k: dict(v) if hasattr(v, "items") else v for k, v in ostats.items() if k not in ("player1", "player2", "draw")}
        assert evals[it] == want, (it, evals[it], want)
    assert not np.array_equal(snaps[0][0]["fc1.weight"], snaps[0][1]["fc1.weight"])  # training moved the weights
    assert np.array_equal(snaps[1][0]["fc1.weight"], snaps[0][1]["fc1.weight"])      # iteration 1 played with iteration 0's result
    d = os.path.join(tmp_path, "o8")
    for f in ("config.json", "loss.json", "eval.json", "o8.pt", "checkpoints/o8-chkpt-1.pt", "checkpoints/o8-chkpt-2.pt"):
        assert os.path.exists(os.path.join(d, f)), f
    loss = json.load(open(os.path.join(d, "loss.json")))
    # one loss value per SGD step: iteration 1's memory is the one still resident; iteration 0 trained on its own
    assert set(loss) == {"0", "1"} and len(loss["1"]["0"]["pi"]) == tr.device_memory["z"].shape[0] // 64 and len(loss["0"]["0"]["pi"]) > 0


def _rehearse(n, *extra, timeout=1500, torchrun=False):
    """`python bench.py --gpus n --full` started plainly (it launches its own ranks) or, torchrun=True, the way the driver starts it (`python -m
    torch.distributed.run --nnodes=1 --nproc-per-node n --master-addr 127.0.0.1 --master-port P bench.py --gpus n ...`), in rehearsal
    mode: gloo instead of RCCL, every rank on this box's one GPU, tiny sizes -> the parsed JSON line"""
    env = dict(os.environ, AZ_BENCH_BACKEND="gloo", AZ_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    launcher = [sys.executable]
    if torchrun:
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        launcher += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(port)]
    cmd = launcher + [os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "1", "--sims", "8", "--full", *extra]
    import tempfile
    with tempfile.TemporaryDirectory() as ddir:
        env["AZ_BENCH_DETAIL_DIR"] = ddir
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        # THE line of record: the last line of stdout, one JSON object of scalars, far below the driver's 8 KB
        assert lines and lines[-1].startswith("{") and len([ln for ln in lines if ln.startswith("{")]) == 1, p.stdout[-2000:]
        assert len(lines[-1]) < 8192
        line = json.loads(lines[-1], parse_constant=lambda c: (_ for _ in ()).throw(AssertionError(c)))
        for k in ("config", "roofline"):
            assert all(v is None or isinstance(v, (bool, int, float, str)) for v in line[k].values()), k
        assert all(not isinstance(v, (dict, list)) for k, v in line.items() if k not in ("config", "roofline", "cpu_baseline"))
        detail = json.load(open(os.path.join(ddir, line["detail"])))
    return line, detail


def test_bench_launches_its_own_ranks(tmp_path):
    """two self-launched ranks: the line must say n_gpus 2, carry per-rank times, the flat summaries inside `config` / `roofline` (what
    the driver's record keeps) and the saturated / config3 / config5 objects"""
    line, out = _rehearse(2, "--games", "64", "--saturated-games", "96", "--config3-total", "64", "--config5-episodes", "64")
    assert line["n_gpus"] == 2 and line["unit"] == "games/s" and line["value"] > 0 and out["n_gpus"] == 2
    assert len(out["per_rank_ms_per_step"]) == 2 and len(out["per_rank_gather_ms_per_step"]) == 2
    assert line["config"]["concurrent_games_per_gpu"] == 64 and line["config"]["end_to_end_frac"] > 0
    assert out["config3"]["n_gpus"] == 2 and out["config3"]["concurrent_games_per_gpu"] == 32 and out["config3"]["value"] > 0
    close = lambda a, b: abs(a - b) <= 1e-5 * abs(b)  # the line rounds to six significant digits
    assert close(line["config"]["config3_games_per_sec"], out["config3"]["value"])
    assert out["saturated"]["concurrent_games"] == 96 and close(line["config"]["saturated_games_per_sec"], out["saturated"]["value"]) and out["saturated"]["value"] > 0
    assert close(line["roofline"]["saturated_frac"], out["saturated"]["roofline"]["frac"]) and out["saturated"]["roofline"]["frac"] <= 1.0
    v = out["config5"]["variants"]
    assert set(v) == {"reference_batch_64", "reference_batch_64_10_epochs", "batch_512", "reference_batch_64_stock_pytorch"}
    assert all(len(x["iterations"]) == 2 for x in v.values())
    assert v["reference_batch_64"]["sgd_step"].startswith("hand-written") and v["reference_batch_64_stock_pytorch"]["sgd_step"] == "stock PyTorch"
    assert all(it["seconds"]["optimize_network"] > 0 and it["eval_results"] for x in v.values() for it in x["iterations"])
    assert v["reference_batch_64_10_epochs"]["iterations"][1]["sgd_steps"] == 10 * (v["reference_batch_64_10_epochs"]["iterations"][1]["samples_with_twins"] // 64)
    assert close(line["config"]["config5_10_epochs_sgd_share"], v["reference_batch_64_10_epochs"]["iterations"][1]["sgd_share"])
    assert line["roofline"]["frac"] <= 1.0 and "end_to_end_frac" in line["roofline"] and not out["errors"]


def test_bench_as_one_rank_under_torch_distributed_run():
    """the driver's launch line for N > 1, two ranks in rehearsal mode: headline + saturated + config5 (one variant) come out as under
    the self-launch"""
    line, out = _rehearse(2, "--games", "32", "--saturated-games", "48", "--config3-total", "64", "--config5-episodes", "64",
                          "--config5-variants", "reference_batch_64", "--config5-eval-episodes", "4", torchrun=True)
    assert line["n_gpus"] == 2 and len(out["per_rank_ms_per_step"]) == 2 and line["value"] > 0
    assert line["config"]["concurrent_games_per_gpu"] == 32 and out["saturated"]["concurrent_games"] == 48
    assert "config3" not in out  # 64 / 2 = the headline's 32 per GPU: config 3 IS the headline
    assert len(out["config5"]["variants"]["reference_batch_64"]["iterations"]) == 2


def test_bench_rehearsal_with_five_ranks_and_an_idle_rank():
    """VERDICT r3 item 3 (GPU half).  The N = 8 control flow -- sharded waves, the packed sample all-gather, config 3, the trainer loop
    with rank 0 training and the others waiting for the weights, the sharded arena -- rehearsed with FIVE ranks: a one-GPU box of this
    pool admits at most six processes on its card and this test process is one of them, so eight ranks cannot be started here (the
    world-8 arithmetic and collectives run on the CPU in tests/test_dist.py::test_world8_with_fewer_units_than_ranks).  config 5 runs
    with 4 evaluation games -> the fifth rank plays no arena round; its results must equal a single process's."""
    line, out = _rehearse(5, "--games", "32", "--saturated-games", "0", "--config3-total", "80", "--config5-episodes", "64",
                          "--config5-variants", "reference_batch_64", "--config5-eval-episodes", "4")
    assert line["n_gpus"] == 5 and len(out["per_rank_ms_per_step"]) == 5 and all(t > 0 for t in out["per_rank_ms_per_step"])
    assert line["config"]["concurrent_games_per_gpu"] == 32 and abs(line["plies_per_game"] - 60.5) < 3
    assert out["config3"]["concurrent_games_per_gpu"] == 16 and out["config3"]["n_gpus"] == 5
    multi = out["config5"]["variants"]["reference_batch_64"]["iterations"]
    import bench
    bench._imports()
    one = bench.run_config5(bench.Job(), 64, 8, eval_episodes=4, only=["reference_batch_64"])["variants"]["reference_batch_64"]["iterations"]
    for a, b in zip(multi, one):
        assert a["samples_with_twins"] == b["samples_with_twins"] and a["eval_results"] == json.loads(json.dumps(b["eval_results"]))
        assert a["last_losses"] == b["last_losses"]


def test_plain_bench_times_the_headline_only_and_dumps_the_same_outputs_twice(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` without --full: set-up, warm-up, K timed steps, the dump, the line --
    no profiled step, CPU baseline or other legs.  Two runs with the same arguments dump the same arrays: the last timed step's samples
    in (game id, move index) order"""
    steps, warmup, games = 2, 1, 64
    dumps = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
               "--games", str(games), "--sims", "8", "--dump-outputs", str(tmp_path / run)]
        env = dict(os.environ, AZ_BENCH_DETAIL_DIR=str(tmp_path / f"detail_{run}"))
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        line = json.loads([ln for ln in p.stdout.splitlines() if ln.strip()][-1])
        assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0 and line["unit"] == "games/s"
        assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["value"] > 0
        assert line["roofline"] is None and line["cpu_baseline"] is None
        detail = json.load(open(tmp_path / f"detail_{run}" / line["detail"]))
        assert not {"saturated", "config1", "config3", "config4", "config5", "latency", "tree_hbm"} & set(detail)
        assert set(detail["bench_seconds"]) == {"imports", "headline_build_warmup_timed", "until_line_of_record"}
        dumps.append({f[:-4]: np.load(tmp_path / run / f, allow_pickle=False) for f in os.listdir(tmp_path / run)})
    a, b = dumps
    assert sorted(a) == ["meta", "n_samples", "pi", "state", "visits", "z"] and sorted(b) == sorted(a)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    n = int(a["n_samples"][0])
    assert a["z"].shape[0] == n <= 128 * games and a["state"].shape == (n, 8, 8) and a["pi"].shape == (n, 65)
    g, mv = a["meta"][:, 0], a["meta"][:, 1]
    last = warmup + steps - 1  # the games of the last timed step
    assert g.min() == last * games and g.max() == (last + 1) * games - 1
    assert np.all(np.diff(g * 1000 + mv) > 0)
    assert np.all(np.isfinite(a["pi"])) and set(np.unique(a["z"])) <= {-1.0, 0.0, 1.0}


def test_bench_fails_when_a_rank_fails():
    """a rank that dies takes the job down with a non-zero exit code (no hang, no half a JSON line)"""
    env = dict(os.environ, AZ_BENCH_BACKEND="gloo", AZ_BENCH_ONE_DEVICE="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--games", "64", "--sims", "0"]  # n_sim = 0: refused
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_player_reset_between_games_on_different_boards():
    """reset() keeps the device storage; the reference's reset() yields a tree usable on ANY board -- an engine built for
    one board must not search another (wrong rules / a crash in set_roots)"""
    from alphazero_amd.games.connect4 import Connect4Board
    from alphazero_amd.games.tictactoe import TicTacToeBoard
    from alphazero_amd.players import MCTSPlayer
    np.random.seed(0)
    pl = MCTSPlayer(n_sim=30)
    for board in (OthelloBoard(n=8), OthelloBoard(n=6), Connect4Board(width=7, height=6), TicTacToeBoard(), OthelloBoard(n=8)):
        pl.reset()
        for _ in range(3):
            mv, probs, visits, _ = pl.get_move(board)
            assert board.is_legal_move(mv) and sum(visits.values()) >= 29  # the kept subtree's visits count too
            board.play_move(mv)
            pl.apply_move(mv)


def test_searches_accumulate_on_one_root():
    """200 searches of 100 simulations without a move: the reference's tree keeps growing (mcts.py:226-269); the device pools are
    grown on demand and keep the tree -- root N counts every simulation, children N sum up"""
    from alphazero_amd.mcts import MCT
    from alphazero_amd.games.othello import OthelloNet
    torch.manual_seed(0)
    mct = MCT(eval_method="neural", nn=OthelloNet(n=8).eval(), seed=5)
    b = OthelloBoard(n=8)
    cap0 = None
    for i in range(200):
        mct.search(b, n_sim=100)
        if cap0 is None:
            cap0 = mct._engine.cfg.node_capacity
    a, n, q, p, root_n = mct._engine.root_children(0)
    assert root_n == 200 * 100
    assert n.sum() in (root_n, root_n - 1)  # every simulation passes through one child of the root
    assert mct._engine.cfg.node_capacity > cap0  # the pools really had to grow
    # a wall-time bounded search on the same tree keeps working too
    mct.search(b, compute_time=0.05)
    assert mct._engine.root_children(0)[4] > root_n


def test_randomised_trainer_loops_equal_oracle():
    """tools/fuzz_trainer.py: random small trainer loops (game, board size, simulations, episodes, batch size, temperature schedule,
    engine slot count, augmentation on / off, evaluation opponent random / greedy / mcts / previous, seed), two iterations each: the
    samples of both iterations equal the oracle's self-play with that iteration's weights, every evaluation the oracle's arena"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_trainer
    assert fuzz_trainer.run(8, seed=77, verbose=False) == []
