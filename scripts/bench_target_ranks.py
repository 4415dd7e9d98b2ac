#!/usr/bin/env python3
"""What exact full-catalogue ranks cost: NCF(6041, 3707, 16, 3) NeuMF-end, 6,040 users, a
million random training positives excluded (the ml-1m shape and density).

Variants, in one process, alternating, each warmed up, device events around one whole call per
repeat:

  target_1     ncf_target_ranks, one held-out item per user (ops.target_ranks_into)
  target_64    the same users with 64 distinct held-out items each (the binary-search path)
  recommend_10, recommend_128
               the way to the same HR / NDCG without the kernel: ncf_recommend at k = 10 and at
               its limit k = 128 (ops.recommend_into), same users, same exclusions
  target_1_materialised
               target_1 forced to the materialised path (ncf_debug_set_target_path)

Reported per variant: median, min, max and interquartile range over the repeats; the ratios of
medians target_1 / recommend_10, target_1 / recommend_128 and target_64 / target_1; and the
check that target_1's ranks below 128 are the positions of those items in recommend_128's
lists.  One JSON document (--out).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from ncf_amd import ops  # noqa: E402
from ncf_amd.models import NCF  # noqa: E402
from serve_bench import alternate, emit, stats  # noqa: E402

U, I, Q, POSITIVES, LONG = 6041, 3707, 6040, 1_000_000, 64


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = NCF(U, I, 16, 3, 0.0, "NeuMF-end").to(dev)
    with torch.no_grad():  # spread tables: the ranks are not degenerate
        for emb in (model.embed_user_GMF, model.embed_item_GMF, model.embed_user_MLP, model.embed_item_MLP):
            emb.weight.normal_(0.0, 0.3)
    flat, lay = ops.ensure_flat(model)
    rng = np.random.default_rng(0)
    seen = ops.seen_csr(rng.integers(0, U, POSITIVES), rng.integers(0, I, POSITIVES), U, dev, I)
    users = torch.arange(Q, dtype=torch.int32, device=dev)
    order = np.argsort(rng.random((Q, I)), axis=1)[:, :LONG].astype(np.int32)  # distinct items per user
    tgt = {1: torch.as_tensor(order[:, :1].reshape(-1).copy(), device=dev),
           LONG: torch.as_tensor(order.reshape(-1).copy(), device=dev)}
    ptr = {m: torch.arange(Q + 1, dtype=torch.int64, device=dev) * m for m in tgt}
    ranks = {m: torch.empty(Q * m, dtype=torch.int32, device=dev) for m in tgt}
    scores = {m: torch.empty(Q * m, dtype=torch.float32, device=dev) for m in tgt}
    ws = {m: ops.target_ranks_workspace(lay, Q, Q * m, ops._Scratch(), dev) for m in tgt}
    mat_ranks = torch.empty(Q, dtype=torch.int32, device=dev)
    with ops._target_materialised():
        ws_mat = ops.target_ranks_workspace(lay, Q, Q, ops._Scratch(), dev)
    rec = {k: (torch.empty((Q, k), dtype=torch.int32, device=dev), torch.empty((Q, k), dtype=torch.float32, device=dev),
               ops.recommend_workspace(lay, Q, k, ops._Scratch(), dev)) for k in (10, 128)}

    def target(m):
        return lambda: ops.target_ranks_into(flat, lay, users, ptr[m], tgt[m], seen, ranks[m], scores[m], ws[m])

    def recommend(k):
        return lambda: ops.recommend_into(flat, lay, users, k, seen, rec[k][0], rec[k][1], rec[k][2])

    def materialised():
        with ops._target_materialised():
            ops.target_ranks_into(flat, lay, users, ptr[1], tgt[1], seen, mat_ranks, None, ws_mat)

    times = alternate({"target_1": target(1), "recommend_10": recommend(10), "recommend_128": recommend(128),
                       f"target_{LONG}": target(LONG), "target_1_materialised": materialised}, args.warmup,
                      args.repeats)
    res = {k: stats(v) for k, v in times.items()}
    med = {k: v["median_ms"] for k, v in res.items()}
    res["target_1_over_recommend_10"] = med["target_1"] / med["recommend_10"]
    res["target_1_over_recommend_128"] = med["target_1"] / med["recommend_128"]
    res[f"target_{LONG}_over_target_1"] = med[f"target_{LONG}"] / med["target_1"]
    # the same answer: a rank below 128 of an item outside the exclusions is its position in recommend's list
    r1, top = ranks[1].cpu().numpy(), rec[128][0].cpu().numpy()
    near = r1 < 128
    at = top[np.arange(Q), np.minimum(r1, 127)]
    t1 = tgt[1].cpu().numpy()
    own = seen.ptr.cpu().numpy()
    items = seen.items.cpu().numpy()
    excluded = np.array([t1[q] in items[own[q]:own[q + 1]] for q in range(Q)])
    check = near & ~excluded
    res["ranks_below_128"] = int(check.sum())
    res["ranks_below_128_agree_with_recommend"] = bool((at[check] == t1[check]).all())
    res["materialised_agrees"] = float((mat_ranks.cpu().numpy() == r1).mean())
    res["mean_rank_target_1"] = float(r1.mean())
    emit({"config": {"model": "NCF(6041, 3707, 16, 3) NeuMF-end", "users": Q, "item_num": I,
                     "excluded_pairs": int(seen.items.numel()), "repeats": args.repeats, "warmup": args.warmup,
                     "device": torch.cuda.get_device_name(dev)},
          "target_ranks": res}, args.out)


if __name__ == "__main__":
    main()
