"""The float64 reference of the distillation tests (tests/distill_checks.py), pinned on
the CPU:
  * against the reference project's own outputs (tests/golden/G8_distill.npz) -- losses
    of the first batch and of 5 Adam steps at rtol 1e-6, first-step gradients to 1e-6 of
    each tensor's largest gradient.  The golden gradients are float32: their own rounding
    (measured here: up to 5.7e-7 of the largest gradient, up to 9e-4 of a near-zero
    element) is what an element-wise rtol would compare against, so the bound is taken
    relative to the largest gradient, the scale the float32 rounding is proportional to;
  * against deliberately wrong references at every shape the device tests use: each lies
    outside the device tests' criteria by at least 2x, so a device result within the
    criteria of the true reference fails against the wrong one."""
import numpy as np
import pytest

import distill_checks as C
from test_distill_host import build


@pytest.mark.parametrize("case", ["c5", "cli"])
@pytest.mark.parametrize("strategy", ["response", "feature", "attention"])
def test_float64_reference_matches_golden(golden, case, strategy):
    g = golden("G8_distill")
    tag = f"{case}_{strategy}"
    d64 = C.f64(build(case, strategy)[2])
    loss, _, grads = C.step_reference(d64, g["users"][0], g["items"][0], g["labels"][0])
    np.testing.assert_allclose(loss, float(g[f"{tag}::loss0"]), rtol=1e-6)
    for k, p in d64.student_model.named_parameters():
        key = f"{tag}::grad0::{k}"
        assert (k in grads) == (key in g.files), k
        if k not in grads:
            continue
        exp = g[key].astype(np.float64)
        scale = float(np.abs(exp).max())
        if scale < 1e-12:  # the attention term's identically-zero gradient: rounding noise on both sides
            assert float(np.abs(grads[k]).max()) < 1e-12, k
            continue
        np.testing.assert_allclose(grads[k], exp, rtol=0, atol=1e-6 * scale, err_msg=k)
    losses, _ = C.trajectory(d64, g["users"].reshape(-1), g["items"].reshape(-1), g["labels"].reshape(-1), 256, 5)
    np.testing.assert_allclose(losses, g[f"{tag}::losses"], rtol=1e-6)


def _outside(p, true, wrong):
    """Whether `wrong` (loss, logits, grads) lies at least 2x outside the criteria around `true`."""
    if abs(wrong[0] - true[0]) > 2 * C.LOSS_RTOL * abs(true[0]):
        return True
    return any(C.grad_excess(wrong[2][k], true[2][k], p.terms(k)) > 2 for k in true[2])


@pytest.mark.parametrize("case,strategy", [(c, s) for c in C.PATH_CASES for s in C.STRATEGIES]
                         + [(c, "feature") for c in C.FEATURE_CASES])
def test_one_step_criteria_reject_wrong_references(case, strategy):
    """One rank: the row sums left undivided by the batch size, and the teacher logit read
    one row off."""
    p = C.problem(case, strategy)
    for wrong in ("no_gb", "shift"):
        assert _outside(p, p.step(), p.step(wrong=wrong)), wrong


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("strategy", ["response", "feature"])
@pytest.mark.parametrize("case", list(C.SHARD_CASES))
def test_shard_criteria_reject_wrong_references(case, strategy, world):
    """Rank shards: a shard normalised by its own rows, and the teacher logit indexed
    inside the shard instead of the stream -- per rank, and in the ranks' sum."""
    p = C.problem(case, strategy)
    for rank in range(world):
        lo, hi = C.shard_bounds(p.B, world, rank)
        for wrong in ("no_gb", "shift"):
            assert _outside(p, p.step(lo, hi), p.step(lo, hi, wrong)), (rank, wrong)
    # the shards of the true reference sum to the one-rank step
    full = p.step()
    parts = [p.step(*C.shard_bounds(p.B, world, r)) for r in range(world)]
    np.testing.assert_allclose(sum(x[0] for x in parts), full[0], rtol=1e-12)
    for k, g in full[2].items():
        np.testing.assert_allclose(sum(x[2][k] for x in parts), g, rtol=1e-9, atol=1e-12 * np.abs(g).max(), err_msg=k)
    np.testing.assert_array_equal(np.concatenate([x[1] for x in parts]), full[1])
