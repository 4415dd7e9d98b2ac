"""Shared rules of the target-rank tests (tests/test_target_ranks.py on the CPU,
tests/test_gpu_target_ranks.py on the device).

``exact_ranks`` is the definition of a rank in NumPy over a given score matrix.
``check_ranks_band`` verifies a result against the CPU oracle's scores (never the code under
test) with the project's logit gate: every rank must lie between the count of the items that
beat the target by more than both tolerances and the count of those that could.  The oracle's
own rank always lies in that band, so no case is left out and no share of failures is tolerated.
"""
import numpy as np
import torch

from recommend_checks import seen_lists, tol


def _np(x):
    return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)


def _free(seen, U, I):
    """[U] -> bool [I]: the items a user's competitors are drawn from (not in seen)."""
    lists = seen_lists(seen, U)
    cache = {}

    def of(u):
        if u not in cache:
            f = np.ones(I, dtype=bool)
            f[lists[u]] = False
            cache[u] = f
        return cache[u]
    return of


def exact_ranks(Z, users, ptr, targets, seen):
    """int64 [E]: rank(u, t) = #{j != t, j not in seen(u): Z[u, j] > Z[u, t] or (== and j < t)} for
    every target, the float32 scores compared by value and ids breaking ties."""
    Z = np.asarray(Z, dtype=np.float32)
    users, ptr, targets = _np(users).reshape(-1), _np(ptr).astype(np.int64), _np(targets).astype(np.int64)
    U, I = Z.shape
    free = _free(seen, U, I)
    ids = np.arange(I)
    out = np.zeros(len(targets), dtype=np.int64)
    for q, u in enumerate(users):
        t = targets[ptr[q]:ptr[q + 1]]
        if len(t) == 0:
            continue
        z, zt = Z[u][None, :], Z[u, t][:, None]
        ahead = (z > zt) | ((z == zt) & (ids[None, :] < t[:, None]))  # t itself: equal score, equal id
        out[ptr[q]:ptr[q + 1]] = (ahead & free(u)[None, :]).sum(1)
    return out


def check_ranks_band(ranks, users, ptr, targets, S, seen, what=""):
    """lo <= rank <= hi for every target against the oracle scores S [U, I], with
    lo = #eligible j != t with S[u,j] - tol(S[u,j]) > S[u,t] + tol(S[u,t]) and
    hi = #eligible j != t with S[u,j] + tol(S[u,j]) >= S[u,t] - tol(S[u,t])."""
    ranks = _np(ranks).reshape(-1).astype(np.int64)
    users, ptr, targets = _np(users).reshape(-1), _np(ptr).astype(np.int64), _np(targets).astype(np.int64)
    S = np.asarray(S)
    U, I = S.shape
    assert len(ptr) == len(users) + 1 and len(ranks) == len(targets) == ptr[-1], (what, "shape")
    free = _free(seen, U, I)
    ids = np.arange(I)
    for q, u in enumerate(users):
        t = targets[ptr[q]:ptr[q + 1]]
        if len(t) == 0:
            continue
        s, st = S[u][None, :], S[u, t][:, None]
        other = free(u)[None, :] & (ids[None, :] != t[:, None])
        lo = (other & (s - tol(s) > st + tol(st))).sum(1)
        hi = (other & (s + tol(s) >= st - tol(st))).sum(1)
        r = ranks[ptr[q]:ptr[q + 1]]
        bad = (r < lo) | (r > hi)
        assert not bad.any(), (what, q, int(u), int(t[bad.argmax()]), int(r[bad.argmax()]), int(lo[bad.argmax()]),
                               int(hi[bad.argmax()]))


def check_scores(scores, users, ptr, targets, S, what=""):
    """The target's own logit within the gate of the oracle's."""
    scores = _np(scores).reshape(-1)
    users, ptr, targets = _np(users).reshape(-1), _np(ptr).astype(np.int64), _np(targets).astype(np.int64)
    owner = np.repeat(np.arange(len(users)), np.diff(ptr))
    want = np.asarray(S)[users[owner], targets]
    err = np.abs(scores - want)
    assert (err <= tol(want)).all(), (what, "score", float(err.max()))
