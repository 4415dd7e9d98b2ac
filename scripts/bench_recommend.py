#!/usr/bin/env python3
"""Full-catalogue top-K: ncf_recommend against what the parent commit offers.

Shape and data: NCF(6041, 3707, 16, 3) NeuMF-end, every user, k = 10, the synthetic
ml-1m training positives excluded.  Two candidates on the same model, in one process,
alternating, device events around the work, every shape warmed up:

  fused     one ncf_recommend call (ops.recommend_into, preallocated outputs)
  baseline  user-chunked ops.pack_rows + ops.forward_logits + masked torch.topk (the
            index tensors of the mask and the (user, item) ids are built outside the
            timed window, in the baseline's favour)

Reported: median, min, max and interquartile range of the repeats, the ratio, the
algorithmic FLOPs and bytes per call computed from the shapes, and how far the two
results agree.  For the record, NCF(64, 4) through ncf_recommend's materialised path:
time and workspace bytes.  One JSON document (--out).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from ncf_amd import _lib as L  # noqa: E402
from ncf_amd import ops, synthetic  # noqa: E402
from ncf_amd.models import NCF  # noqa: E402
from serve_bench import alternate, emit, stats  # noqa: E402


def algorithmic_cost(U, I, f, nl, q, k, nnz):
    """FLOPs (2 per MAC) and compulsory bytes of one call, from the shapes alone."""
    dm = f << (nl - 1)
    tower_tail = sum((dm >> (j - 1)) * (dm >> j) for j in range(1, nl))  # layers 1..L-1, MACs per pair
    layer0 = 2 * dm * dm
    head = 2 * f + f  # predict dot over [gmf | tower], GMF product
    pairs = q * I
    fused = {
        "flops": 2 * (pairs * (tower_tail + head) + (I + q) * dm * dm) + 2 * pairs * dm,  # + add/ReLU of width dm
        # tables read once, projections written and read, seen lists, results
        "bytes": 4 * ((I + q) * (dm + f) + 2 * (I + q) * dm) + 4 * nnz + 8 * q * k,
    }
    baseline = {
        "flops": 2 * pairs * (layer0 + tower_tail + head),
        # per pair: packed row written and read, four embedding rows gathered, logit written and read by topk
        "bytes": pairs * (16 + 4 * (2 * dm + 2 * f) + 8) + 8 * nnz + 8 * q * k,
    }
    return fused, baseline


class Baseline:
    """User-chunked pack_rows + forward_logits + masked topk (the parent commit's route)."""

    def __init__(self, model, users, k, seen, chunk_users):
        self.flat, self.lay = ops.ensure_flat(model)
        self.model, self.k = model, k
        dev = self.flat.device
        I = model.item_num
        ptr = seen.ptr.cpu().numpy()
        sit = seen.items.cpu().numpy().astype(np.int64)
        self.chunks = []
        for b in range(0, len(users), chunk_users):
            uc = users[b:b + chunk_users]
            u = torch.as_tensor(np.repeat(uc, I), dtype=torch.int32, device=dev)
            i = torch.arange(I, dtype=torch.int32, device=dev).repeat(len(uc))
            flat_idx = np.concatenate([r * I + sit[ptr[x]:ptr[x + 1]] for r, x in enumerate(uc)])
            self.chunks.append((b, len(uc), u, i, torch.as_tensor(flat_idx, dtype=torch.int64, device=dev)))
        n = chunk_users * I
        self.rows = torch.empty(n, dtype=torch.int64, device=dev)
        self.logits = torch.empty(n, dtype=torch.float32, device=dev)
        self.items = torch.empty((len(users), k), dtype=torch.int64, device=dev)
        self.scores = torch.empty((len(users), k), dtype=torch.float32, device=dev)

    def __call__(self):
        I = self.model.item_num
        for b, c, u, i, idx in self.chunks:
            rows = ops.pack_rows(u, i, out=self.rows[:c * I])
            lg = ops.forward_logits(self.flat, self.lay, rows, out=self.logits[:c * I], ws_owner=self.model)
            lg.index_fill_(0, idx, float("-inf"))
            s, it = torch.topk(lg.view(c, I), self.k, dim=1)
            self.scores[b:b + c] = s
            self.items[b:b + c] = it


class Fused:
    def __init__(self, model, users, k, seen):
        self.flat, self.lay = ops.ensure_flat(model)
        dev = self.flat.device
        self.users = torch.as_tensor(users, dtype=torch.int32, device=dev)
        self.k, self.seen = k, seen
        self.items = torch.empty((len(users), k), dtype=torch.int32, device=dev)
        self.scores = torch.empty((len(users), k), dtype=torch.float32, device=dev)
        self.ws = ops.recommend_workspace(self.lay, len(users), k, model, dev)
        self.ws_bytes = int(L.hip().ncf_recommend_workspace_bytes(L.ctypes.byref(self.lay), len(users), k))

    def __call__(self):
        ops.recommend_into(self.flat, self.lay, self.users, self.k, self.seen, self.items, self.scores, self.ws)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--top_k", type=int, default=10)
    ap.add_argument("--chunk_users", type=int, default=512, help="users per chunk of the baseline")
    ap.add_argument("--record_repeats", type=int, default=20, help="repeats of the NCF(64,4) record (0: skip)")
    ap.add_argument("--out", default="profiles/recommend_c3.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_recommend.py needs a HIP device: there is no CPU timing")
    dev = torch.device("cuda", 0)
    U, I, f, nl, k = 6041, 3707, 16, 3, args.top_k
    ds = synthetic.make_dataset("ml-1m", seed=0)
    seen = ops.seen_csr(ds["train_users"], ds["train_items"], U, dev, I)
    nnz = int(seen.items.numel())
    users = np.arange(U)
    torch.manual_seed(0)
    model = NCF(U, I, f, nl, 0.0, "NeuMF-end").to(dev)
    fused = Fused(model, users, k, seen)
    base = Baseline(model, users, k, seen, args.chunk_users)
    times = alternate({"fused": fused, "baseline": base}, args.warmup, args.repeats)
    fi, bi = fused.items.cpu().numpy().astype(np.int64), base.items.cpu().numpy()
    fs, bs = fused.scores.cpu().numpy(), base.scores.cpu().numpy()
    same_rows = float((fi == bi).all(axis=1).mean())
    same_sets = float(np.mean([set(a) == set(b) for a, b in zip(fi, bi)]))
    common = fi == bi
    cost_f, cost_b = algorithmic_cost(U, I, f, nl, U, k, nnz)
    sf, sb = stats(times["fused"]), stats(times["baseline"])
    doc = {
        "device": torch.cuda.get_device_name(0),
        "shape": {"user_num": U, "item_num": I, "factor_num": f, "num_layers": nl, "model_type": "NeuMF-end",
                  "queried_users": U, "top_k": k, "excluded_pairs": nnz},
        "fused": dict(sf, workspace_bytes=fused.ws_bytes, algorithmic=cost_f,
                      gflops_at_median=cost_f["flops"] / sf["median_ms"] / 1e6),
        "baseline": dict(sb, chunk_users=args.chunk_users, algorithmic=cost_b,
                         gflops_at_median=cost_b["flops"] / sb["median_ms"] / 1e6),
        "baseline_over_fused": sb["median_ms"] / sf["median_ms"],
        "agreement": {"rows_identical": same_rows, "rows_same_item_set": same_sets,
                      "max_abs_score_diff_same_position": float(np.abs(fs - bs)[common].max())},
    }
    if args.record_repeats > 0:
        m2 = NCF(U, I, 64, 4, 0.0, "NeuMF-end").to(dev)
        rec = Fused(m2, users, k, seen)
        doc["record_ncf_64_4_materialised"] = dict(stats(alternate({"rec": rec}, 2, args.record_repeats)["rec"]),
                                                   workspace_bytes=rec.ws_bytes,
                                                   path=int(L.supported("NeuMF-end", 64, 4)))
    emit(doc, args.out)


if __name__ == "__main__":
    main()
