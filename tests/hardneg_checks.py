"""Shared pieces of the dynamic-negative-sampling tests (tests/test_hardneg.py on the CPU,
tests/test_gpu_hardneg.py on the device).

The reference of every numeric check is ``oracle.ncf_oracle.OracleNCF`` on the CPU (models
from ``bpr_checks.models``: trained-size tables) -- never the code under test.

Near ties.  Two correct fp32 evaluations may order two candidates differently when their
scores differ by less than the logit tolerance, tol(x) = 1e-7 + 1e-5 |x| (the project's
logit gate).  A group is *decided* when the oracle's best score beats the best score of
every candidate with a different item id by at least 4 tol (tol at the best score).
  * decided groups: the chosen item must equal the oracle's choice exactly;
  * the rest: the chosen candidate's oracle score must be within 2 tol of the oracle
    maximum, and the returned score within tol of the oracle's score of that candidate;
  * at most 1% of a test's groups may be undecided (TIE_MAX_FRACTION), asserted.
Measured on the CPU with the fp32 oracle, uniform candidates: at most 0.4% of the groups of
any case of these tests are undecided (4 of 1,000), none in the cases of 17 groups or
fewer.
"""
import numpy as np
import torch

from bpr_checks import TIE_MAX_FRACTION

RTOL, ATOL = 1e-5, 1e-7  # the project's logit gate


def tol(x):
    return ATOL + RTOL * np.abs(x)


def draw(n, m, U, I, seed=3):
    """(users [n], candidates [n, m]) uniform over the ids."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, (n, m)).astype(np.int32)


def oracle_scores(ref, users, cand):
    """[n, m] float32 eval-mode logits of the oracle over the pairs (users[p], cand[p, j])."""
    users, cand = np.asarray(users), np.asarray(cand)
    n, m = cand.shape
    ref.eval()
    with torch.no_grad():
        z = ref(torch.as_tensor(np.repeat(users, m), dtype=torch.int64),
                torch.as_tensor(cand.reshape(-1), dtype=torch.int64))
    return z.numpy().reshape(n, m)


def oracle_choice(S, cand):
    """(slot [n], item [n], decided [n]) of the oracle scores S [n, m]: the first argmax,
    its item id, and whether it beats every candidate with another id by at least 4 tol."""
    cand = np.asarray(cand).astype(np.int64)
    n = len(S)
    slot = np.argmax(S, axis=1)  # the first maximum
    rows = np.arange(n)
    item = cand[rows, slot]
    best = S[rows, slot]
    other = np.where(cand != item[:, None], S, -np.inf).max(axis=1)
    return slot, item, best - other >= 4 * tol(best)


def check_selection(S, cand, items, slots=None, scores=None, what=""):
    """The near-tie rule above for one call's outputs against the oracle scores S [n, m].
    Returns the number of undecided groups (already asserted to be at most 1%)."""
    cand = np.asarray(cand).astype(np.int64)
    items = np.asarray(items).astype(np.int64).reshape(-1)
    n, m = cand.shape
    assert items.shape == (n,), (what, items.shape)
    slot_ref, item_ref, decided = oracle_choice(S, cand)
    undecided = int((~decided).sum())
    print(f"{what}: n={n} m={m} undecided={undecided}")
    assert undecided <= TIE_MAX_FRACTION * n, f"{what}: {undecided} of {n} groups undecided"
    bad = decided & (items != item_ref)
    assert not bad.any(), (what, "decided group", int(np.flatnonzero(bad)[0]), int(bad.sum()))
    rows = np.arange(n)
    member = cand == items[:, None]
    assert member.any(axis=1).all(), (what, "chosen item is not a candidate of its group")
    if slots is not None:
        slots = np.asarray(slots).astype(np.int64).reshape(-1)
        assert ((slots >= 0) & (slots < m)).all() and (cand[rows, slots] == items).all(), (what, "slot")
        chosen = S[rows, slots]
    else:
        chosen = np.where(member, S, -np.inf).max(axis=1)
    best = S[rows, slot_ref]
    u = ~decided
    assert (best[u] - chosen[u] <= 2 * tol(best[u])).all(), (what, "undecided group: a candidate far from the maximum")
    if scores is not None:
        scores = np.asarray(scores).reshape(-1)
        err = np.abs(scores - chosen)
        print(f"{what}: worst |score - oracle| / tol over all groups = {float((err / tol(chosen)).max()):.3f}")
        assert (err[u] <= tol(chosen[u])).all(), (what, "undecided group: score")
    return undecided


def state_to_oracle(state_dict, U, I, f, Lyr, mt):
    """An OracleNCF carrying the given parameters (tensors on any device)."""
    from oracle import ncf_oracle as O
    ref = O.OracleNCF(U, I, f, Lyr, 0.0, mt)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in state_dict.items()})
    return ref.eval()
