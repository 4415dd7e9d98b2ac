#!/usr/bin/env python3
"""Top-K over caller-supplied candidate lists from a saved NCF checkpoint.

Loads a ``state_dict`` file as ``scripts/recommend.py`` does and reads the candidates from a
text file of ``user<TAB>item`` lines: one list per distinct user, users in the order of
their first line, a user's items in file order (duplicates are kept: every line is a
candidate).  Writes ``users`` (int64 [Q]), ``items`` (int64 [Q, k], -1 = the list is
shorter than k), ``slots`` (int64 [Q, k], the candidate's position in its user's list) and
``scores`` (float32 [Q, k]) to an ``.npz``.  Runs ``NCF.rank`` on a HIP device if one is
present (the fused score-and-select kernel), else on the CPU.

Usage: python scripts/rank.py --checkpoint results/models/NeuMF_end_3l_32f_best.pth \
           --model NeuMF-end --top_k 10 --candidates candidates.tsv --out ranked.npz
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.append(os.path.abspath(os.path.dirname(__file__)))
sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from recommend import load_model  # noqa: E402
from ncf_amd import ops  # noqa: E402


def read_candidates(path):
    """(users int64 [Q], ops.CandidateLists) of a ``user<TAB>item`` file."""
    pairs = np.loadtxt(path, dtype=np.int64, ndmin=2)
    if pairs.size == 0:
        pairs = pairs.reshape(0, 2)
    if pairs.shape[1] != 2:
        raise ValueError(f"{path}: expected two columns (user, item)")
    users, first, inverse = np.unique(pairs[:, 0], return_index=True, return_inverse=True)
    rank = np.empty(len(users), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(users))  # distinct users in file order
    q = rank[inverse.reshape(-1)]
    order = np.argsort(q, kind="stable")  # a user's lines stay in file order
    ptr = np.zeros(len(users) + 1, dtype=np.int64)
    np.cumsum(np.bincount(q, minlength=len(users)), out=ptr[1:])
    return users[np.argsort(first, kind="stable")], ops.CandidateLists(torch.from_numpy(ptr),
                                                                       torch.from_numpy(pairs[order, 1].copy()))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint", required=True, help="state_dict file")
    ap.add_argument("--model", default="NeuMF-end", choices=["GMF", "MLP", "NeuMF-end", "NeuMF-pre"])
    ap.add_argument("--top_k", type=int, default=10)
    ap.add_argument("--candidates", required=True, help="text file of user<TAB>item lines")
    ap.add_argument("--out", default="ranked.npz")
    ap.add_argument("--device", default=None, help="default: cuda:0 if present, else cpu")
    args = ap.parse_args(argv)

    device = torch.device(args.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    model = load_model(args.checkpoint, args.model, device)
    users, cands = read_candidates(args.candidates)
    cands = ops.CandidateLists(cands.ptr.to(device), cands.items.to(device))
    r = model.rank(torch.from_numpy(users), cands, args.top_k)
    np.savez(args.out, users=users, items=r.items.cpu().numpy(), slots=r.slots.cpu().numpy(),
             scores=r.scores.cpu().numpy())
    print(f"Wrote top-{args.top_k} of {cands.items.numel()} candidates in {len(users)} lists to {args.out} ({device})")


if __name__ == "__main__":
    main()
