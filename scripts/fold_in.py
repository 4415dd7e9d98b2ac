#!/usr/bin/env python3
"""Fold new users into a saved NCF checkpoint and recommend for them.

Reads ``user<TAB>item`` lines (arbitrary user labels; item ids of the checkpoint's
catalogue), fits a GMF and an MLP vector per user to its list with the rest of the model
frozen (``NCF.fold_in``: the items as positives plus ``--num_ng`` sampled negatives each,
``--steps`` full-batch Adam steps), and writes to an ``.npz``: ``users`` (the labels, in
order of first appearance), ``gmf`` [Q, f], ``mlp`` [Q, dm], ``loss`` [Q, steps], and the
top-k of the whole catalogue with each user's given items left out as ``items`` (int64
[Q, k], -1 = no more eligible items) / ``scores`` (float32 [Q, k]).  Runs on a HIP device
if one is present (``ncf_fold_in``: one kernel runs every step of a user), else on the CPU.

Usage: python scripts/fold_in.py --checkpoint results/models/NeuMF_end_3l_32f_best.pth \
           --model NeuMF-end --interactions new_users.tsv --top_k 10 --out folded.npz
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.append(os.path.abspath(os.path.dirname(__file__)))

from ncf_amd import ops  # noqa: E402
from recommend import load_model  # noqa: E402


def read_interactions(path):
    """(labels in order of first appearance, list of int64 item arrays in file order)."""
    index, lists = {}, []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.split("\t")
            if len(parts) < 2:
                raise ValueError(f"{path}:{ln}: expected user<TAB>item")
            q = index.setdefault(parts[0], len(index))
            if q == len(lists):
                lists.append([])
            lists[q].append(int(parts[1]))
    return list(index), [np.asarray(x, dtype=np.int64) for x in lists]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint", required=True, help="state_dict file")
    ap.add_argument("--model", default="NeuMF-end", choices=["GMF", "MLP", "NeuMF-end", "NeuMF-pre"])
    ap.add_argument("--interactions", required=True, help="text file of user<TAB>item lines")
    ap.add_argument("--num_ng", type=int, default=4, help="sampled negatives per given item")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0, help="seed of the negative sampling")
    ap.add_argument("--top_k", type=int, default=10)
    ap.add_argument("--out", default="folded.npz")
    ap.add_argument("--device", default=None, help="default: cuda:0 if present, else cpu")
    args = ap.parse_args(argv)

    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    model = load_model(args.checkpoint, args.model, device)
    labels, lists = read_interactions(args.interactions)
    if not lists:
        raise SystemExit(f"{args.interactions}: no interactions")
    ex = ops.fold_examples(lists, model.item_num, args.num_ng, torch.Generator().manual_seed(args.seed))
    folded = model.fold_in(ex, steps=args.steps, lr=args.lr)
    served = model.with_users(folded)
    seen_u = np.concatenate([np.full(len(x), q, dtype=np.int64) for q, x in enumerate(lists)])
    items, scores = served.recommend(torch.arange(len(lists)), args.top_k, (seen_u, np.concatenate(lists)))
    loss = folded.loss.cpu().numpy()
    np.savez(args.out, users=np.asarray(labels), gmf=folded.gmf.cpu().numpy(), mlp=folded.mlp.cpu().numpy(),
             loss=loss, items=items.cpu().numpy(), scores=scores.cpu().numpy())
    print(f"folded {len(lists)} users ({ex.items.numel()} examples, {args.steps} steps) on {device}: "
          f"mean loss {loss[:, 0].mean():.4f} -> {loss[:, -1].mean():.4f}; top-{args.top_k} -> {args.out}")


if __name__ == "__main__":
    main()
