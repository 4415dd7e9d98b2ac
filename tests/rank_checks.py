"""Shared pieces of the candidate-ranking tests (tests/test_rank.py on the CPU,
tests/test_gpu_rank.py on the device).

The reference of every numeric check is ``oracle.ncf_oracle.OracleNCF`` on the CPU (through
``recommend_checks.oracle_scores`` / ``hardneg_checks.oracle_scores``) -- never the code
under test.  ``check_ranked`` is ``recommend_checks.check_topk`` restricted to a list: the
catalogue becomes the user's own candidate list, the item id key becomes the slot.  No
share of the cases may be skipped: every list of every call is checked in full.
"""
import numpy as np
import torch

from recommend_checks import ATOL, RTOL, tol

# list lengths every ragged case covers: empty, one, around one 16-lane tile, around four
# tiles (one per wave), many tiles; the long ones repeat ids (I = 80 < 200)
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 200, 1000]


def _np(x):
    return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)


def cycle_lengths(n_lists, lengths=LENGTHS, seed=3):
    """n_lists >= len(lengths) list lengths: `lengths` repeated, in a shuffled order."""
    assert n_lists >= len(lengths)
    lens = np.array([lengths[q % len(lengths)] for q in range(n_lists)], dtype=np.int64)
    return lens[np.random.default_rng(seed).permutation(n_lists)]


def ragged(lens, U, I, seed=3):
    """(users [n], ptr [n + 1], items [E]) for lists of the given lengths, users and ids
    uniform (so a list longer than the catalogue repeats ids)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    ptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    users = rng.integers(0, U, len(lens)).astype(np.int32)
    items = rng.integers(0, I, int(ptr[-1])).astype(np.int32)
    return users, ptr, items


def check_ranked(items, slots, scores, users, ptr, cand, S, k, what="", rtol=RTOL, atol=ATOL):
    """Every property of a rank() result against the oracle scores: S is either the
    [U, I] score matrix (indexed by user id and item id) or a flat [E] array of the
    oracle's score of every (list, slot) pair.  Shapes, the -1 / -1 / -inf fill beyond
    min(k, len), slots valid and distinct, items == list[slots], scores within tolerance,
    the stated order (score descending, then slot ascending), and that no candidate left
    out beats the k-th returned one by more than the two tolerances."""
    items, slots, scores = _np(items).astype(np.int64), _np(slots).astype(np.int64), _np(scores)
    users, ptr, cand = _np(users).reshape(-1), _np(ptr).astype(np.int64), _np(cand).astype(np.int64)
    S = np.asarray(S)
    n = len(users)
    assert len(ptr) == n + 1
    assert items.shape == slots.shape == scores.shape == (n, k), (what, items.shape, slots.shape, scores.shape)
    assert scores.dtype == np.float32
    for q in range(n):
        lst = cand[ptr[q]:ptr[q + 1]]
        want_all = S[users[q], lst] if S.ndim == 2 else S[ptr[q]:ptr[q + 1]]
        n_ret = min(k, len(lst))
        it, sl, sc = items[q], slots[q], scores[q]
        assert (it[n_ret:] == -1).all() and (sl[n_ret:] == -1).all(), (what, q, "fill")
        assert np.isneginf(sc[n_ret:]).all(), (what, q, "fill")
        it, sl, sc = it[:n_ret], sl[:n_ret], sc[:n_ret]
        if n_ret == 0:
            continue
        assert sl.min() >= 0 and sl.max() < len(lst), (what, q, "slot range")
        assert len(np.unique(sl)) == n_ret, (what, q, "duplicate slot")
        assert np.array_equal(it, lst[sl]), (what, q, "items != list[slots]")
        want = want_all[sl]
        err = np.abs(sc - want)
        assert (err <= tol(want, rtol, atol)).all(), (what, q, "score", float(err.max()), want[err.argmax()])
        ordered = (sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (sl[:-1] < sl[1:]))
        assert ordered.all(), (what, q, "order")
        rest = np.ones(len(lst), dtype=bool)
        rest[sl] = False
        if rest.any():
            left = want_all[rest]
            kth = want[-1]
            bound = kth + tol(kth, rtol, atol) + tol(left, rtol, atol)
            assert (left <= bound).all(), (what, q, "better candidate left out")
