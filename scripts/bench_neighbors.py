#!/usr/bin/env python3
"""Similar items over the whole catalogue: ncf_neighbors against stock torch ops.

Shape and data: NCF(., I, 16, 3) NeuMF-end with N(0, 1) tables, item side, concat space
(d = 16 + 64), cosine, every item queried, k = 10, the query left out, at the ml-1m
(I = 3,707) and ml-20m (I = 26,744) catalogues.  Two candidates on the same model, in one
process, alternating, device events around the work, every shape warmed up:

  fused     one ncf_neighbors call (ops.neighbors_into, preallocated outputs)
  baseline  F.normalize of the concatenated tables, then per chunk of queries
            Q @ C^T, the self entry set to -inf, torch.topk

Reported per catalogue: median, min, max and interquartile range of the repeats, the
ratio, the fused call's workspace bytes, the baseline's peak allocation above the model,
and how far the two results agree.  One JSON document (--out).
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from ncf_amd import _lib as L  # noqa: E402
from ncf_amd import ops  # noqa: E402
from ncf_amd.models import NCF  # noqa: E402
from serve_bench import alternate, emit, stats  # noqa: E402


class Baseline:
    """normalize + query-chunked Q @ C^T + masked topk."""

    def __init__(self, model, k, chunk_queries):
        self.model, self.k, self.chunk = model, k, chunk_queries
        n = model.item_num
        dev = model.embed_item_GMF.weight.device
        self.ids = torch.empty((n, k), dtype=torch.int64, device=dev)
        self.scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        self.rows = torch.arange(chunk_queries, device=dev)
        self.cols = torch.arange(n, device=dev)

    @torch.no_grad()
    def __call__(self):
        m = self.model
        c = F.normalize(torch.cat((m.embed_item_GMF.weight, m.embed_item_MLP.weight), 1), dim=1)
        n = c.shape[0]
        for b in range(0, n, self.chunk):
            e = min(n, b + self.chunk)
            s = c[b:e] @ c.t()
            s[self.rows[:e - b], self.cols[b:e]] = float("-inf")
            val, idx = torch.topk(s, self.k, dim=1)
            self.scores[b:e] = val
            self.ids[b:e] = idx


class Fused:
    def __init__(self, model, k):
        self.flat, self.lay = ops.ensure_flat(model)
        dev = self.flat.device
        n = model.item_num
        self.q = torch.arange(n, dtype=torch.int32, device=dev)
        self.k = k
        self.ids = torch.empty((n, k), dtype=torch.int32, device=dev)
        self.scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        self.ws = ops.neighbors_workspace(self.lay, L.SIDE_ITEM, L.SPACE_CONCAT, n, k, model, dev)
        self.ws_bytes = int(L.hip().ncf_neighbors_workspace_bytes(L.ctypes.byref(self.lay), L.SIDE_ITEM,
                                                                  L.SPACE_CONCAT, n, k))

    def __call__(self):
        ops.neighbors_into(self.flat, self.lay, L.SIDE_ITEM, L.SPACE_CONCAT, L.SIM_COSINE, self.q, self.k, True,
                           self.ids, self.scores, self.ws)


def measure(I, f, nl, k, chunk_queries, warmup, repeats, dev):
    torch.manual_seed(0)
    model = NCF(64, I, f, nl, 0.0, "NeuMF-end")
    with torch.no_grad():
        model.embed_item_GMF.weight.normal_(0.0, 1.0)
        model.embed_item_MLP.weight.normal_(0.0, 1.0)
    model = model.to(dev)
    fused = Fused(model, k)
    base = Baseline(model, k, chunk_queries)
    variants = {"fused": fused, "baseline": base}
    alternate(variants, warmup, 0)
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base()
    torch.cuda.synchronize()
    peak = int(torch.cuda.max_memory_allocated(dev) - before)
    times = alternate(variants, 0, repeats)
    fi, bi = fused.ids.cpu().numpy().astype(np.int64), base.ids.cpu().numpy()
    fs, bs = fused.scores.cpu().numpy(), base.scores.cpu().numpy()
    common = fi == bi
    sf, sb = stats(times["fused"]), stats(times["baseline"])
    d = f + (f << (nl - 1))
    return {
        "shape": {"item_num": I, "factor_num": f, "num_layers": nl, "side": "item", "space": "concat", "d": d,
                  "metric": "cosine", "queries": I, "top_k": k, "exclude_self": True},
        "fused": dict(sf, workspace_bytes=fused.ws_bytes, gflops_at_median=2.0 * I * I * d / sf["median_ms"] / 1e6),
        "baseline": dict(sb, chunk_queries=chunk_queries, peak_alloc_bytes=peak, score_matrix_bytes=4 * I * I),
        "baseline_over_fused": sb["median_ms"] / sf["median_ms"],
        "agreement": {"rows_identical": float(common.all(axis=1).mean()),
                      "rows_same_id_set": float(np.mean([set(a) == set(b) for a, b in zip(fi, bi)])),
                      "max_abs_score_diff_same_position": float(np.abs(fs - bs)[common].max())},
    }


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--top_k", type=int, default=10)
    ap.add_argument("--chunk_queries", type=int, default=512, help="queries per chunk of the baseline")
    ap.add_argument("--items", type=int, nargs="+", default=[3707, 26744])
    ap.add_argument("--out", default="profiles/neighbors.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_neighbors.py needs a HIP device: there is no CPU timing")
    dev = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(0),
           "catalogues": [measure(I, 16, 3, args.top_k, args.chunk_queries, args.warmup, args.repeats, dev)
                          for I in args.items]}
    emit(doc, args.out)


if __name__ == "__main__":
    main()
