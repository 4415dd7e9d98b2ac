"""What the serving benchmarks (bench_recommend, bench_neighbors, bench_fold_in,
bench_select_negatives, bench_rank) share: device-event timing of one call, the alternating
loop over the variants of one process, the summary of a list of times and the JSON tail."""
import json
import os

import numpy as np
import torch


def stats(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_ms": float(med), "min_ms": float(a[0]), "max_ms": float(a[-1]), "iqr_ms": float(q3 - q1),
            "repeats": len(a)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(variants, warmup, repeats):
    """{name: [ms]}: every variant of {name: fn} called `warmup` times, then `repeats` rounds of
    one timed call of each in turn.  A variant with a reset() has it called before every call,
    outside the timed window (the device is synchronised after it)."""
    def prepared(fn):
        if hasattr(fn, "reset"):
            fn.reset()
            torch.cuda.synchronize()
        return fn

    for fn in variants.values():
        for _ in range(warmup):
            prepared(fn)()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(repeats):
        for name, fn in variants.items():
            times[name].append(timed(prepared(fn)))
    return times


def emit(doc, out_path):
    """Print the document as one JSON line; with out_path, write it there indented as well."""
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    print(json.dumps(doc))
