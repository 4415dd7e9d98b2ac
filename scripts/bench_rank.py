#!/usr/bin/env python3
"""What candidate ranking costs: NCF(6041, 3707, 16, 3) NeuMF-end, one candidate list for
each of the 6,041 users, top_k = 10.

Workloads:
  uniform  1,000 distinct random candidates per user
  skewed   list lengths log-uniform in [16, 3000], distinct random candidates

Three ways to rank, in one process, alternating, each warmed up, device events around one
whole call per repeat:

  fused         ncf_rank_candidates on its fused path (ops.rank_into)
  materialised  the same call forced to its materialised path (ncf_debug_set_rank_path:
                rows kernel, ncf_forward in chunks of 131,072 pairs, one wave per list)
  baseline      without the kernel, stock ops: ops.pack_rows + ops.forward_logits over all
                the pairs, the logits scattered into a [lists, longest] matrix padded with
                -inf, torch.topk (the repeated user column and the scatter index are built
                once, outside the timing)

Reported per variant: median, min, max and interquartile range over the repeats, the ratios
of medians fused / materialised and fused / baseline, and how often the variants' items agree
(fp32 near ties may differ between arithmetic orders; torch.topk does not order equal
scores by slot).  One JSON document (--out).
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

U, I, K = 6041, 3707, 10


def workload(name, rng):
    """(ptr int64 [U + 1], items int32) of distinct random candidates per user."""
    lens = np.full(U, 1000) if name == "uniform" else np.exp(rng.uniform(np.log(16), np.log(3000), U)).astype(np.int64)
    order = np.argsort(rng.random((U, I)), axis=1).astype(np.int32)  # a permutation of the catalogue per user
    ptr = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    return ptr, np.concatenate([order[u, :lens[u]] for u in range(U)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = NCF(U, I, 16, 3, 0.0, "NeuMF-end").to(dev)
    flat, lay = ops.ensure_flat(model)
    rng = np.random.default_rng(0)
    users = torch.arange(U, dtype=torch.int32, device=dev)
    out = {"config": {"model": "NCF(6041, 3707, 16, 3) NeuMF-end", "lists": U, "item_num": I, "top_k": K,
                      "repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev)},
           "rank": {}}

    for name in ("uniform", "skewed"):
        ptr_h, items_h = workload(name, rng)
        n_cand = int(ptr_h[-1])
        lens_h = np.diff(ptr_h)
        width = int(lens_h.max())
        ptr = torch.as_tensor(ptr_h, device=dev)
        cand = torch.as_tensor(items_h, device=dev)
        lens = torch.as_tensor(lens_h, device=dev)
        users_rep = users.repeat_interleave(lens).contiguous()
        # flat position e of list q, slot j -> q * width + j of the padded matrix
        pad_index = (torch.arange(n_cand, device=dev) - ptr[:-1].repeat_interleave(lens)
                     + torch.arange(U, device=dev).repeat_interleave(lens) * width)
        rows = torch.empty(n_cand, dtype=torch.int64, device=dev)
        logits = torch.empty(n_cand, dtype=torch.float32, device=dev)
        padded = torch.empty(U * width, dtype=torch.float32, device=dev)
        res_t = {k: (torch.empty((U, K), dtype=torch.int32, device=dev),
                     torch.empty((U, K), dtype=torch.int32, device=dev),
                     torch.empty((U, K), dtype=torch.float32, device=dev)) for k in ("fused", "materialised")}
        ws = {"fused": ops.rank_workspace(lay, U, n_cand, K, ops._Scratch(), dev)}
        with ops._rank_materialised():
            ws["materialised"] = ops.rank_workspace(lay, U, n_cand, K, ops._Scratch(), dev)
        base = {}

        def fused():
            ops.rank_into(flat, lay, users, ptr, cand, K, *res_t["fused"], ws["fused"])

        def materialised():
            with ops._rank_materialised():
                ops.rank_into(flat, lay, users, ptr, cand, K, *res_t["materialised"], ws["materialised"])

        def baseline():
            ops.pack_rows(users_rep, cand, out=rows)
            ops.forward_logits(flat, lay, rows, out=logits, ws_owner=model)
            padded.fill_(float("-inf"))
            padded[pad_index] = logits
            val, j = torch.topk(padded.view(U, width), K, dim=1)
            base["scores"] = val
            base["items"] = cand[(ptr[:-1].unsqueeze(1) + j).clamp_(max=n_cand - 1)]

        times = alternate({"fused": fused, "materialised": materialised, "baseline": baseline}, args.warmup,
                          args.repeats)
        res = {k: stats(v) for k, v in times.items()}
        med = {k: v["median_ms"] for k, v in res.items()}
        res["candidates"] = n_cand
        res["list_length"] = {"min": int(lens_h.min()), "median": float(np.median(lens_h)), "max": width}
        res["fused_pairs_per_us"] = n_cand / (1e3 * med["fused"])
        res["fused_over_materialised"] = med["fused"] / med["materialised"]
        res["fused_over_baseline"] = med["fused"] / med["baseline"]
        res["agree_fused_materialised"] = float((res_t["fused"][0] == res_t["materialised"][0]).float().mean().item())
        res["agree_fused_baseline"] = float((res_t["fused"][0] == base["items"]).float().mean().item())
        out["rank"][name] = res
        del cand, users_rep, pad_index, rows, logits, padded

    emit(out, args.out)


if __name__ == "__main__":
    main()
