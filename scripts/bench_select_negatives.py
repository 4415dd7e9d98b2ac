#!/usr/bin/env python3
"""What dynamic negative sampling costs per epoch: synthetic ml-1m positives,
NCF(6041, 3707, 16, 3) NeuMF-end, m in {4, 16} uniform candidates per positive.

Three ways to pick each positive's highest-scoring candidate, in one process, alternating,
each warmed up, device events around one whole-epoch selection per repeat:

  fused         ncf_select_negatives on its fused path (ops.select_negatives_into)
  materialised  the same call forced to its materialised path
                (ncf_debug_set_select_path: rows kernel, ncf_forward, select kernel, in
                chunks of 131,072 pairs)
  baseline      without the kernel: ops.pack_rows + ops.forward_logits over the P * m rows
                + torch.argmax and a gather (the repeated user column is built once,
                outside the timing)

Reported per variant: median, min, max and interquartile range over the repeats, and the
ratios of medians fused / materialised and fused / baseline.  For context, the time of one
hard-BPR epoch's optimizer steps at 32,768 triples per step (a TrainEngine(loss="bpr") over
the P chosen triples, graph-replayed), the selection time over that step time and its share of
selection + steps: the selection runs on the training stream at the epoch boundary and is
not overlapped.
One JSON document (--out).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from ncf_amd import ops, synthetic  # noqa: E402
from ncf_amd.engine import TrainEngine  # noqa: E402
from ncf_amd.models import NCF  # noqa: E402
from serve_bench import alternate, emit, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--triples", type=int, default=32768, help="triples per optimizer step of the epoch context")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ds = synthetic.make_dataset("ml-1m", seed=0)
    U, I = int(ds["user_num"]), int(ds["item_num"])
    pu = torch.as_tensor(np.asarray(ds["train_users"]), dtype=torch.int32, device=dev)
    pi = torch.as_tensor(np.asarray(ds["train_items"]), dtype=torch.int32, device=dev)
    P = pu.numel()
    torch.manual_seed(0)
    model = NCF(U, I, 16, 3, 0.0, "NeuMF-end").to(dev)
    flat, lay = ops.ensure_flat(model)
    rng = np.random.default_rng(0)
    out = {"config": {"model": "NCF(6041, 3707, 16, 3) NeuMF-end", "user_num": U, "item_num": I, "positives": P,
                      "repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev)},
           "select": {}}

    chosen = torch.empty(P, dtype=torch.int32, device=dev)
    for m in (4, 16):
        cand = torch.as_tensor(rng.integers(0, I, P * m).astype(np.int32), device=dev)  # timing only: uniform
        users_rep = pu.repeat_interleave(m).contiguous()
        rows = torch.empty(P * m, dtype=torch.int64, device=dev)
        logits = torch.empty(P * m, dtype=torch.float32, device=dev)
        picks = {k: torch.empty(P, dtype=torch.int32, device=dev) for k in ("fused", "materialised")}
        ws = {"fused": ops.select_negatives_workspace(lay, P, m, ops._Scratch(), dev)}
        with ops._select_materialised():
            ws["materialised"] = ops.select_negatives_workspace(lay, P, m, ops._Scratch(), dev)
        base = {}

        def fused():
            ops.select_negatives_into(flat, lay, pu, cand, m, picks["fused"], None, None, ws["fused"])

        def materialised():
            with ops._select_materialised():
                ops.select_negatives_into(flat, lay, pu, cand, m, picks["materialised"], None, None,
                                          ws["materialised"])

        def baseline():
            ops.pack_rows(users_rep, cand, out=rows)
            ops.forward_logits(flat, lay, rows, out=logits, ws_owner=model)
            j = torch.argmax(logits.view(P, m), dim=1)
            base["items"] = cand.view(P, m).gather(1, j.unsqueeze(1)).squeeze(1)

        times = alternate({"fused": fused, "materialised": materialised, "baseline": baseline}, args.warmup,
                          args.repeats)
        res = {k: stats(v) for k, v in times.items()}
        med = {k: v["median_ms"] for k, v in res.items()}
        res["fused_over_materialised"] = med["fused"] / med["materialised"]
        res["fused_over_baseline"] = med["fused"] / med["baseline"]
        # how often the three agree (fp32 near ties may differ between arithmetic orders)
        res["agree_fused_materialised"] = float((picks["fused"] == picks["materialised"]).float().mean().item())
        res["agree_fused_baseline"] = float((picks["fused"] == base["items"]).float().mean().item())
        out["select"][f"m{m}"] = res
        if m == 4:
            chosen.copy_(picks["fused"])
        del cand, users_rep, rows, logits

    # context: the optimizer steps of one hard-BPR epoch over the P chosen triples
    perm = torch.as_tensor(rng.permutation(P), device=dev)
    pairs = ops.build_pair_stream(pu, pi, chosen, 1, perm)
    eng = TrainEngine(model, lr=1e-3, loss="bpr")
    eng.set_epoch_stream(pairs, 2 * args.triples, checked=True)
    nb = eng.num_batches
    # one warm-up epoch (graph capture)
    ep = stats(alternate({"epoch": lambda: eng.run(nb, use_graph=True)}, 1, max(3, args.repeats // 2))["epoch"])
    ep["steps"] = int(nb)
    ep["triples_per_step"] = args.triples
    out["epoch_steps"] = ep
    for m in (4, 16):
        sel = out["select"][f"m{m}"]["fused"]["median_ms"]
        out["select"][f"m{m}"]["selection_over_epoch_steps"] = sel / ep["median_ms"]
        out["select"][f"m{m}"]["share_of_epoch"] = sel / (sel + ep["median_ms"])
    emit(out, args.out)


if __name__ == "__main__":
    main()
