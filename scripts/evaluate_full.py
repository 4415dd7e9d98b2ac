#!/usr/bin/env python3
"""Full-catalogue evaluation of a saved NCF checkpoint from exact ranks: HR / Recall /
Precision / NDCG at every requested K, MRR, MAP, AUC and the mean rank, for any number of
held-out items per user.

Loads a ``state_dict`` file as ``scripts/recommend.py`` does, ranks every held-out item of
every user against the whole catalogue (``NCF.target_ranks``: on a HIP device the fused
score-and-count kernel, else the CPU path) and prints one table and one JSON line
(``ncf_amd.metrics.rank_report``).  Held-out items: by default the first entry of each line of
the configured test file (``(user,item)\\tneg\\t...``: the leave-one-out protocol of
``metrics()``); with ``--heldout FILE`` the (user, item) pairs of a whitespace- or tab-separated
text file, any number per user (an 80/20 or time-window split).  ``--exclude_train`` leaves the
training positives of the configured data set out of every user's catalogue.

Usage: python scripts/evaluate_full.py --checkpoint results/models/NeuMF_end_3l_32f_best.pth \
           --model NeuMF-end --ks 1,5,10,20,50,100 --exclude_train [--heldout pairs.tsv]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from ncf_amd import ops  # noqa: E402
from ncf_amd.metrics import rank_report  # noqa: E402
from recommend import load_model  # noqa: E402


def test_file_heldout(path):
    """(users, items) int64: the ``(user,item)`` head of every line of a test-negative file."""
    us, its = [], []
    with open(path, "r") as fd:
        for line in fd:
            head = line.split("\t", 1)[0].strip()
            if not head:
                continue
            if not (head.startswith("(") and head.endswith(")")):
                raise ValueError(f"bad test-negative line head: {head!r}")
            u, i = head[1:-1].split(",")
            us.append(int(u))
            its.append(int(i))
    return np.asarray(us, dtype=np.int64), np.asarray(its, dtype=np.int64)


def group_by_user(users, items):
    """(distinct users ascending, CandidateLists of their held-out items in file order)."""
    order = np.argsort(users, kind="stable")
    uniq, counts = np.unique(users, return_counts=True)
    ptr = np.zeros(len(uniq) + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    return uniq, ops.CandidateLists(torch.from_numpy(ptr), torch.from_numpy(items[order]))


def table(rep, ks):
    lines = [f"users evaluated: {rep['users']}", f"{'k':>6} {'HR':>8} {'Recall':>8} {'Prec':>8} {'NDCG':>8}"]
    m = rep["mean"]
    for k in ks:
        lines.append(f"{k:>6} {m[f'hr@{k}']:8.4f} {m[f'recall@{k}']:8.4f} {m[f'precision@{k}']:8.4f} "
                     f"{m[f'ndcg@{k}']:8.4f}")
    lines.append(f"MRR {m['mrr']:.4f}  MAP {m['map']:.4f}  AUC {m['auc']:.4f}  mean rank {m['mean_rank']:.1f}")
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint", required=True, help="state_dict file")
    ap.add_argument("--model", default="NeuMF-end", choices=["GMF", "MLP", "NeuMF-end", "NeuMF-pre"])
    ap.add_argument("--ks", default="1,5,10,20,50,100", help="comma-separated cut-offs")
    ap.add_argument("--heldout", default=None, help="text file of held-out (user, item) pairs; default: the "
                                                     "first entry of each line of the configured test file")
    ap.add_argument("--exclude_train", action="store_true",
                    help="leave out the training positives of the configured data set")
    ap.add_argument("--device", default=None, help="default: cuda:0 if present, else cpu")
    args = ap.parse_args(argv)

    ks = [int(k) for k in args.ks.split(",")]
    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    model = load_model(args.checkpoint, args.model, device)
    if args.heldout:
        pairs = np.loadtxt(args.heldout, dtype=np.int64, ndmin=2)
        hu, hi = pairs[:, 0], pairs[:, 1]
    else:
        from ncf_amd.config import config
        hu, hi = test_file_heldout(config.test_negative)
    users, lists = group_by_user(hu, hi)
    exclude = None
    if args.exclude_train:
        from ncf_amd.config import config
        from ncf_amd.data import parse_train_rating
        tu, ti = parse_train_rating(config.train_rating)
        exclude = ops.seen_csr(tu, ti, model.user_num, device, model.item_num)
    r = model.target_ranks(torch.from_numpy(users), lists, exclude)
    rep = rank_report(r.ranks, r.ptr, r.eligible, ks)
    print(table(rep, ks))
    print(json.dumps({"checkpoint": args.checkpoint, "model": args.model, "device": str(device),
                      "users": rep["users"], "heldout": int(len(hu)), "item_num": model.item_num,
                      "exclude_train": bool(args.exclude_train), "metrics": rep["mean"]}))


if __name__ == "__main__":
    main()
