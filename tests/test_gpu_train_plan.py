"""GPU: one OthelloNet 8x8 trainer walked through every default dense configuration of the training step's plan
(alphazero_amd/csrc/az_train_plan.h): batch 512 (<8,8,1,true>, fc2's forward in 64-row blocks), 272 (<4,16,1,true>),
80 (<8,8,1,false>), 16 (<4,16,1,false>) and 384 (<8,8,1,true> again).  OthelloNet 8x8 is the net whose dense kernels ask for more
dynamic LDS than the default limit, so every leg depends on the attributes the trainer sets from the plan once per plan change, and on
graphs captured anew.  Each leg against a fresh trainer of exactly that batch size: the same bits."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_train_step as C  # noqa: E402

pytestmark = pytest.mark.gpu


def test_one_trainer_through_every_default_dense_configuration():
    """one trainer of max_batch 512, begin() once, then two steps each at 512, 272, 80, 16 and 384, each leg one az_trainer_steps call
    with the same sample / permutation / loss pointers throughout.  Before each leg a fresh trainer of that batch size takes over the
    state (check_train_step.copy_state) and runs the same call: same losses, same state dict, bit for bit."""
    prob = C.StateProblem("othello8", 512)
    live = prob.trainer(512)
    live.load(prob.net)
    live.begin(*C.STATE_HYPER, C.state_dropout("othello8"), seed=3)
    for leg, B in enumerate((512, 272, 80, 16, 384)):
        fresh = prob.trainer(B)
        C.copy_state(live, fresh)
        a = C.state_run(live, prob, ((0, 2),), B=B, load=False, begin=False)
        b = C.state_run(fresh, prob, ((0, 2),), B=B, load=False, begin=False)
        fresh.close()
        assert C.all_finite(a) and int(a["sd.bn1.num_batches_tracked"]) == 2 * (leg + 1)
        C.same_bits(b, a, ("othello8", "leg", leg, "batch", B))
    live.close()
