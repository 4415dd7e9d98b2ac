"""Shared checks of the nearest-neighbour tests (CPU and GPU): a float64 reference of the
similarity of every (query, row) pair, written from the definitions in include/ncf_hip.h,
its per-pair fp32 tolerance and the verification of a similar_items / similar_users /
ncf_neighbors result.

Tolerance of a pair: the forward-error bound of a length-d fp32 dot product in any
summation order, derived, not measured (u = 2^-24, R = sum_i |q_i c_i|):
  dot     1.01 (d + 2) u R + 1e-30
  cosine  1.01 (2 d + 10) u R / (|q| |c|), and exactly 0 where either norm is 0
The cosine count: d u for the dot, (d / 2 + 2) u for each inverse norm (sum of squares,
sqrt, reciprocal), 2 u for the two multiplies, 4 u of padding; 1.01 absorbs 1 / (1 - d u)."""
import numpy as np
import torch

U_FP32 = 2.0 ** -24


def table64(model, side, space):
    """float64 [N, d] vectors of one side's rows in `space`, from the fp32 tables."""
    gmf = (model.embed_item_GMF if side == "item" else model.embed_user_GMF).weight
    mlp = (model.embed_item_MLP if side == "item" else model.embed_user_MLP).weight
    parts = {"gmf": [gmf], "mlp": [mlp], "concat": [gmf, mlp]}[space]
    return np.concatenate([p.detach().cpu().numpy().astype(np.float64) for p in parts], axis=1)


def reference(table, queries, metric):
    """(S, T) float64 [Q, N]: reference score and tolerance of every (query, row) pair."""
    queries = np.asarray(queries, dtype=np.int64).reshape(-1)
    d = table.shape[1]
    Q = table[queries]
    S = Q @ table.T
    R = np.abs(Q) @ np.abs(table).T
    if metric == "dot":
        return S, 1.01 * (d + 2) * U_FP32 * R + 1e-30
    assert metric == "cosine"
    den = np.sqrt((Q * Q).sum(1))[:, None] * np.sqrt((table * table).sum(1))[None, :]
    zero = den == 0
    den = np.where(zero, 1.0, den)
    S = np.where(zero, 0.0, S / den)
    T = np.where(zero, 0.0, 1.01 * (2 * d + 10) * U_FP32 * R / den)
    return S, T


def check_neighbors(ids, scores, queries, S, T, k, exclude_self):
    """Every property of a result against the reference (S, T) of the same queries:
    shapes, fill, ids in range and unique, the query's own id absent when excluded, every
    score within its pair's tolerance, the (score descending, id ascending) order, and that
    no eligible row left out exceeds the k-th returned reference score by more than the
    two pairs' tolerances."""
    ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids).astype(np.int64)
    scores = np.asarray(scores.cpu() if isinstance(scores, torch.Tensor) else scores)
    queries = np.asarray(queries, dtype=np.int64).reshape(-1)
    Q, N = S.shape
    assert Q == len(queries)
    assert ids.shape == scores.shape == (Q, k)
    assert scores.dtype == np.float32
    assert not np.isnan(scores).any()
    n_ret = min(k, N - 1 if exclude_self else N)
    assert (ids[:, n_ret:] == -1).all() and np.isneginf(scores[:, n_ret:]).all(), "fill"
    if n_ret == 0:
        return
    it, sc = ids[:, :n_ret], scores[:, :n_ret].astype(np.float64)
    assert it.min() >= 0 and it.max() < N, "id range"
    srt = np.sort(it, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "duplicate id"
    if exclude_self:
        assert (it != queries[:, None]).all(), "query returned"
    rows = np.arange(Q)[:, None]
    want, wtol = S[rows, it], T[rows, it]
    err = np.abs(sc - want)
    bad = err > wtol
    assert not bad.any(), ("score", float(err[bad].max()), float(wtol[bad].min()), int(bad.sum()))
    ordered = (sc[:, :-1] > sc[:, 1:]) | ((sc[:, :-1] == sc[:, 1:]) & (it[:, :-1] < it[:, 1:]))
    assert ordered.all(), "order"
    rest = np.ones((Q, N), dtype=bool)
    rest[rows, it] = False
    if exclude_self:
        rest[np.arange(Q), queries] = False
    bound = (want[:, -1] + wtol[:, -1])[:, None] + T
    assert not (rest & (S > bound)).any(), "better row left out"
