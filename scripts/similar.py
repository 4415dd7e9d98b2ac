#!/usr/bin/env python3
"""Nearest neighbours over the learned embeddings of a saved NCF checkpoint: "more like
this item" / "users like this one".

Loads a ``state_dict`` file as ``scripts/recommend.py`` does and writes ``queries``
(int64 [Q]), ``ids`` (int64 [Q, k], -1 = no more eligible rows) and ``scores``
(float32 [Q, k]) to an ``.npz``.  Runs ``NCF.similar_items`` / ``NCF.similar_users`` on a
HIP device if one is present (the fused score-and-select kernel), else on the CPU.

Usage: python scripts/similar.py --checkpoint results/models/NeuMF_end_3l_32f_best.pth \
           --model NeuMF-end --side item --ids all --top_k 10 --out similar.npz
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.append(os.path.abspath(os.path.dirname(__file__)))
sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from recommend import load_model, read_users  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint", required=True, help="state_dict file")
    ap.add_argument("--model", default="NeuMF-end", choices=["GMF", "MLP", "NeuMF-end", "NeuMF-pre"])
    ap.add_argument("--side", default="item", choices=["item", "user"])
    ap.add_argument("--ids", default="all", help="'all' or a text file of item / user ids")
    ap.add_argument("--top_k", type=int, default=10)
    ap.add_argument("--space", default=None, choices=["gmf", "mlp", "concat"],
                    help="default: the model type's own tables")
    ap.add_argument("--metric", default="cosine", choices=["cosine", "dot"])
    ap.add_argument("--keep_self", action="store_true", help="do not leave the queried id out of its own list")
    ap.add_argument("--out", default="similar.npz")
    ap.add_argument("--device", default=None, help="default: cuda:0 if present, else cpu")
    args = ap.parse_args(argv)

    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    model = load_model(args.checkpoint, args.model, device)
    n = model.item_num if args.side == "item" else model.user_num
    queries = read_users(args.ids, n)
    fn = model.similar_items if args.side == "item" else model.similar_users
    ids, scores = fn(torch.from_numpy(queries), args.top_k, args.space, args.metric, not args.keep_self)
    np.savez(args.out, queries=queries, ids=ids.cpu().numpy(), scores=scores.cpu().numpy())
    print(f"Wrote top-{args.top_k} {args.metric} neighbours among {n} {args.side}s for {len(queries)} queries "
          f"to {args.out} ({device})")


if __name__ == "__main__":
    main()
