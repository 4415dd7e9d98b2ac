"""HR@K / NDCG@K leave-one-out evaluation (reference src/training/metrics.py:4-25).

``metrics(model, test_loader, top_k)`` keeps the reference signature and return
value (per-batch lists).  For a HIP-resident model it scores every candidate of
every batch with one forward launch and ranks all batches with one
``ncf_hr_ndcg`` launch (one wave per batch); the loader is still iterated
exactly once, so the torch generator consumption (one base_seed draw) is the
reference's.  For a CPU model it runs the reference's per-batch loop.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L


def _hr_ndcg_topk(logits, items, sizes, top_k):
    """Loaders ncf_hr_ndcg does not take (batches above 1024 rows, or of unequal
    sizes): the reference's per-batch ranking (metrics.py:10-22) with torch.topk on
    the device logits -- HR = gt in the top k, NDCG = 1 / log2(first hit + 2)."""
    hr, nd = [], []
    pos = 0
    for s in sizes:
        if top_k > s:
            raise RuntimeError("selected index k out of range")  # torch.topk's error (metrics.py:13)
        pred, item = logits[pos:pos + s], items[pos:pos + s]
        _, idx = torch.topk(pred, top_k)
        hit = torch.take(item, idx) == item[0]
        first = torch.argmax(hit.to(torch.int32))
        any_hit = hit.any()
        hr.append(any_hit.to(torch.int32))
        nd.append(torch.where(any_hit, 1.0 / torch.log2(first.to(torch.float64) + 2.0),
                              torch.zeros((), dtype=torch.float64, device=logits.device)))
        pos += s
    return torch.stack(hr), torch.stack(nd)


def _hr_ndcg_device(logits, items_i32, batch, top_k):
    n = items_i32.numel()
    nb = (n + batch - 1) // batch
    last = n - (nb - 1) * batch
    if top_k > last or top_k > batch:
        raise RuntimeError("selected index k out of range")  # torch.topk's error (metrics.py:13)
    if batch > 1024:  # beyond ncf_hr_ndcg's LDS staging
        return _hr_ndcg_topk(logits, items_i32, [batch] * (nb - 1) + [last], top_k)
    hr = torch.empty(nb, dtype=torch.int32, device=logits.device)
    nd = torch.empty(nb, dtype=torch.float32, device=logits.device)
    L.check(L.hip().ncf_hr_ndcg(logits.data_ptr(), items_i32.data_ptr(), n, int(batch), int(top_k),
                                hr.data_ptr(), nd.data_ptr(), L.stream_ptr(logits.device)), "ncf_hr_ndcg")
    return hr, nd


def evaluate_rows_device(model, rows, items_i32, batch, top_k):
    """Per-batch HR (int32) and NDCG (float32) on the device for a packed candidate
    stream whose ids the caller has checked; nothing is synchronised."""
    from . import ops
    flat, lay = ops.ensure_flat(model)
    with torch.no_grad():
        logits = ops.forward_logits(flat, lay, rows, ws_owner=model)
    return _hr_ndcg_device(logits, items_i32, batch, top_k)


def evaluate_arrays(model, users, items, batch, top_k, sizes=None):
    """HR/NDCG lists for a flat candidate stream cut into `batch`-row batches (or into
    the given batch `sizes`, a loader's unequal batches)."""
    from . import ops
    flat, lay = ops.ensure_flat(model)
    dev = flat.device
    ops.check_ids(users, items, model.user_num, model.item_num)  # nn.Embedding raises (models.py:108-112)
    u = torch.as_tensor(np.asarray(users), dtype=torch.int32).to(dev)
    i = torch.as_tensor(np.asarray(items), dtype=torch.int32).to(dev)
    with torch.no_grad():
        logits = ops.forward_logits(flat, lay, ops.pack_rows(u, i), ws_owner=model)
    if sizes is not None:
        hr, nd = _hr_ndcg_topk(logits, i, sizes, top_k)
    else:
        hr, nd = _hr_ndcg_device(logits, i, batch, top_k)
    return hr.cpu().tolist(), nd.double().cpu().tolist()


def metrics(model, test_loader, top_k):
    dev_model = model.embed_user_GMF.weight.is_cuda
    if not dev_model:
        return _metrics_cpu(model, test_loader, top_k)
    us, its, sizes = [], [], []
    for user, item, _ in test_loader:
        us.append(torch.as_tensor(user).view(-1))
        its.append(torch.as_tensor(item).view(-1))
        sizes.append(its[-1].numel())
    if not sizes:
        return [], []
    bs = sizes[0]
    ragged = any(s != bs for s in sizes[:-1]) or sizes[-1] > bs  # e.g. a batch_sampler: per-batch ranking
    if top_k > min(sizes):
        raise RuntimeError("selected index k out of range")
    HR, NDCG = evaluate_arrays(model, torch.cat(us), torch.cat(its), bs, top_k, sizes if ragged else None)
    return HR, [float(x) for x in NDCG]


def _metrics_cpu(model, test_loader, top_k):
    HR, NDCG = [], []
    for user, item, _ in test_loader:
        with torch.no_grad():
            predictions = model(user, item)
            _, indices = torch.topk(predictions, top_k)
            recommends = torch.take(item, indices).cpu().numpy()
        gt_item = item[0].item()
        HR.append(int(gt_item in recommends))
        ndcg = 0.0
        if gt_item in recommends:
            index = np.where(recommends == gt_item)[0][0]
            ndcg = 1.0 / np.log2(index + 2)
        NDCG.append(ndcg)
    return HR, NDCG


def hr_ndcg_from_topk(items, gt_items):
    """Per-user HR (int) and NDCG (float) lists from ranked item ids [Q, k] and the held-out
    item of each row: metrics()'s formulas (hit if gt is in the top k, 1 / log2(pos + 2))."""
    items = np.asarray(items)
    gt = np.asarray(gt_items).reshape(-1, 1)
    hit = items == gt
    any_hit = hit.any(axis=1)
    pos = hit.argmax(axis=1)
    ndcg = np.where(any_hit, 1.0 / np.log2(pos + 2.0), 0.0)
    return [int(h) for h in any_hit], [float(x) for x in ndcg]


def full_rank_metrics(model, users, gt_items, top_k, exclude=None):
    """Full-ranking HR@K / NDCG@K: each user's held-out item ranked against the whole
    catalogue (``model.recommend``; ``exclude`` as there, usually the training
    positives) instead of the 99 sampled negatives of ``metrics()``.  Per-user lists."""
    users = np.asarray(users).reshape(-1)
    gt = np.asarray(gt_items).reshape(-1)
    if users.size != gt.size:
        raise ValueError("users and gt_items must have equal length")
    if users.size == 0:
        return [], []
    items, _ = model.recommend(torch.as_tensor(users.astype(np.int64)), top_k, exclude)
    return hr_ndcg_from_topk(items.cpu().numpy(), gt)


def _host(x):
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)


def rank_report(ranks, ptr, eligible, ks=(1, 5, 10, 20, 50, 100)):
    """Ranking metrics from exact full-catalogue ranks (``NCF.target_ranks``): pure NumPy.

    ``ranks``: the 0-based ranks of every held-out item, flat or shaped, in the order ``ptr``
    (int64 [n + 1]) cuts into the n users' lists; ``eligible`` [n]: the number of items each
    user's ranks are out of.  For a user with P >= 1 held-out items at sorted ranks
    r_0 < ... < r_{P-1} among E eligible items:
      hr@k = any r < k;  recall@k = #{r < k} / P;  precision@k = #{r < k} / k;
      ndcg@k = sum_{r < k} 1 / log2(r + 2)  over  sum_{j < min(P, k)} 1 / log2(j + 2);
      mrr = 1 / (r_0 + 1);  map (average precision) = mean_j (j + 1) / (r_j + 1);
      auc = 1 - sum_j (r_j - j) / (P (E - P)), NaN when E = P;  mean_rank = mean_j r_j.
    The formulas assume a user's held-out items are distinct and not among the items the
    ranks excluded (``exclude`` of ``target_ranks``): then a user's ranks are distinct.  Two
    equal ranks in one list mean a duplicate target: ValueError.

    Returns ``{"users": the users with P >= 1, "mean": {name: mean over those users},
    "per_user": {name: float64 [n]}}`` with names ``hr@k`` ... for every k of ``ks``, ``mrr``,
    ``map``, ``auc``, ``mean_rank``; a user without held-out items has NaN throughout and is
    left out of the means, as is a NaN auc."""
    r = _host(ranks).reshape(-1).astype(np.int64)
    ptr = _host(ptr).reshape(-1).astype(np.int64)
    n = ptr.size - 1
    E = _host(eligible).reshape(-1).astype(np.float64)
    if n < 0 or E.size != n or ptr[0] != 0 or ptr[-1] != r.size or (np.diff(ptr) < 0).any():
        raise ValueError("rank_report: ptr [n + 1] must ascend from 0 to len(ranks), eligible [n]")
    ks = [int(k) for k in ks]
    if any(k < 1 for k in ks):
        raise ValueError("rank_report: every k must be at least 1")
    P = np.diff(ptr)
    owner = np.repeat(np.arange(n), P)
    r = r[np.lexsort((r, owner))]  # ascending inside every user; owner is already ascending
    if ((r[1:] == r[:-1]) & (owner[1:] == owner[:-1])).any():
        raise ValueError("rank_report: a user has two equal ranks (duplicate targets)")
    j = np.arange(r.size) - ptr[owner]  # position among the user's sorted ranks
    has = P >= 1
    Pf = np.where(has, P, 1).astype(np.float64)
    nan = np.where(has, 0.0, np.nan)  # added to every per-user value: NaN for a user without targets

    def per_user(w):
        return np.bincount(owner, weights=w, minlength=n)

    gain = 1.0 / np.log2(r + 2.0)
    ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(max(int(P.max()) if n else 0, 1)) + 2.0))])
    out = {}
    for k in ks:
        hit = (r < k).astype(np.float64)
        hits = per_user(hit)
        out[f"hr@{k}"] = (hits > 0).astype(np.float64) + nan
        out[f"recall@{k}"] = hits / Pf + nan
        out[f"precision@{k}"] = hits / k + nan
        out[f"ndcg@{k}"] = per_user(hit * gain) / np.where(has, ideal[np.minimum(P, k)], 1.0) + nan
    first = np.full(n, np.nan)
    first[has] = r[ptr[:-1][has]]
    out["mrr"] = 1.0 / (first + 1.0)
    out["map"] = per_user((j + 1.0) / (r + 1.0)) / Pf + nan
    room = Pf * (E - P)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["auc"] = np.where(room > 0, 1.0 - per_user((r - j).astype(np.float64)) / room, np.nan) + nan
    out["mean_rank"] = per_user(r.astype(np.float64)) / Pf + nan
    mean = {}
    for name, v in out.items():
        ok = ~np.isnan(v)
        mean[name] = float(v[ok].mean()) if ok.any() else float("nan")
    return {"users": int(has.sum()), "mean": mean, "per_user": out}


def full_rank_report(model, users, targets, ks=(1, 5, 10, 20, 50, 100), exclude=None):
    """``rank_report`` of ``model.target_ranks(users, targets, exclude)``: every ranking metric
    at every K over the whole catalogue, for any number of held-out items per user
    (``targets`` as ``NCF.target_ranks`` takes them; ``exclude`` usually the training positives)."""
    r = model.target_ranks(users, targets, exclude)
    return rank_report(r.ranks, r.ptr, r.eligible, ks)
