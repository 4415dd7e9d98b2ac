#!/usr/bin/env python3
"""What the pairwise (BPR) mode costs at config C3: NCF(6041, 3707, 16, 3) NeuMF-end,
65,536 rows per step, synthetic ml-1m positives with 4 sampled negatives each.

Three streams on three engines with identical initial parameters, in one process,
alternating, each warmed up, device events around `--steps` graph-replayed optimizer
steps per repeat:

  bpr          loss="bpr" on the pair stream (ncf_build_pair_stream over a random
               permutation of the triples): 32,768 triples per step
  bce_pairs    loss="bce" on the very same rows (labels 1 / 0 ride in them), ungrouped
  bce_grouped  loss="bce" on the stream the epoch pipeline builds for BCE training
               (ncf_prepare_epoch: the DataLoader batches, each grouped by item)

bpr / bce_pairs is the cost of the mode itself (same rows, same order); bce_pairs /
bce_grouped is what the missing item grouping costs.  (The pair stream holds every
positive once per negative, so its row population is not the BCE stream's: the second
ratio compares the two training streams as the project builds them.)
Reported per stream: median, min, max and interquartile range of the per-step time over
the repeats; the two ratios of medians.  One JSON document (--out).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from ncf_amd import _lib as L  # noqa: E402
from ncf_amd import ops, synthetic  # noqa: E402
from ncf_amd.engine import TrainEngine  # noqa: E402
from ncf_amd.models import NCF  # noqa: E402


def stats(us):
    a = np.sort(np.asarray(us, dtype=np.float64))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_us": float(med), "min_us": float(a[0]), "max_us": float(a[-1]), "iqr_us": float(q3 - q1),
            "repeats": len(a)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=300, help="timed steps per repeat")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=65536, help="rows per step (two per triple)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ds = synthetic.make_dataset("ml-1m", seed=0)
    U, I = int(ds["user_num"]), int(ds["item_num"])
    pos = np.stack([ds["train_users"], ds["train_items"]], 1).astype(np.int64)
    P, ng = len(pos), 4
    rng = np.random.default_rng(0)
    neg = rng.integers(0, I, P * ng).astype(np.int32)  # timing only: unmasked uniform negatives
    pu = torch.as_tensor(pos[:, 0], dtype=torch.int32, device=dev)
    pi = torch.as_tensor(pos[:, 1], dtype=torch.int32, device=dev)
    negd = torch.as_tensor(neg, device=dev)
    S = P * ng
    pairs = ops.build_pair_stream(pu, pi, negd, ng, torch.as_tensor(rng.permutation(S), device=dev))
    ops.check_pair_rows(pairs, U, I)
    # the BCE epoch stream: features_fill in DataLoader order, batches grouped by item
    n = P + S
    rows = torch.empty(n, dtype=torch.int64, device=dev)
    L.check(L.hip().ncf_build_rows(pu.data_ptr(), pi.data_ptr(), P, negd.data_ptr(), ng, rows.data_ptr(),
                                   L.stream_ptr(dev)), "ncf_build_rows")
    grouped = ops.EpochPrep(dev, canonical=False)(rows, torch.as_tensor(rng.permutation(n), device=dev), args.rows, I)

    def engine(loss, stream):
        torch.manual_seed(0)
        eng = TrainEngine(NCF(U, I, 16, 3, 0.0, "NeuMF-end").to(dev), lr=1e-3, loss=loss)
        eng.set_epoch_stream(stream, args.rows, checked=True)
        eng.run(args.warmup, use_graph=True)
        return eng
    engines = {"bpr": engine("bpr", pairs), "bce_pairs": engine("bce", pairs), "bce_grouped": engine("bce", grouped)}
    torch.cuda.synchronize()
    times = {k: [] for k in engines}
    for _ in range(args.repeats):
        for name, eng in engines.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.run(args.steps, use_graph=True)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    res = {k: stats(v) for k, v in times.items()}
    med = {k: v["median_us"] for k, v in res.items()}
    out = {"config": {"model": "NCF(6041, 3707, 16, 3) NeuMF-end", "user_num": U, "item_num": I,
                      "rows_per_step": args.rows, "positives": P, "num_ng": ng, "steps": args.steps,
                      "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(dev),
                      "fact_mode": {k: bool(ops.fact_mode(e.lay)) for k, e in engines.items()},
                      "stream_rows": {"pairs": int(pairs.numel()), "grouped": int(grouped.numel())}},
           "per_step": res,
           "bpr_over_bce_pairs": med["bpr"] / med["bce_pairs"],
           "bce_pairs_over_bce_grouped": med["bce_pairs"] / med["bce_grouped"],
           "last_loss": {k: float(e.epoch_losses()[(int(e.ctl[0].item()) - 1) % e.num_batches])
                         for k, e in engines.items()}}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
