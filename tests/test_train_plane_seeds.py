"""The data seeds tests/test_gpu_train_planes.py replaced (check_train_step.PLANE_FLIPS), judged without a GPU: what the hand-written
step showed on the MI355X at such a seed is what ONE ReLU unit on the other branch does to the float64 gradients -- the float64 run's
closest tie, in the layer recorded, to the four digits recorded -- and not an error of another size or shape."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_train_step as C  # noqa: E402


@pytest.mark.parametrize("tag,B,seed", sorted(C.PLANE_FLIPS))
def test_a_replaced_seed_is_one_flipped_unit(tag, B, seed):
    layer, seen = C.PLANE_FLIPS[tag, B, seed]
    (name, index, tie, rel), = C.relu_flip_effect(tag, B, seed, closest_only=True)
    print(f"{tag} {B} seed {seed}: {name}[{index}] at {tie:.3g} of its layer's largest input; forced the other way: err / max|g_ref| {rel:.3g} (MI355X: {seen})")
    assert name == layer and tie < 2e-6
    assert abs(rel - seen) <= 1e-3 * seen  # `seen` is recorded to four digits
    cases = {c[:2]: c[2] for c in C.PLANE_CASES}
    assert seed not in cases[tag, B] and len(cases[tag, B]) == len(set(cases[tag, B]))
