#!/usr/bin/env python3
"""Record G14_reference_scripts.json from a checkout of the reference project:

    python tests/golden/make_golden_refscripts.py <reference checkout>

Stored (names and recorded results only, no program text of the reference):
* import_surface: for each of the reference's scripts, the names it imports from
  ``src.*`` (``{script: {module: [names]}}``);
* train_neumf: the reference's own scripts/train_neumf.py run unchanged against this
  repository's ``src/`` on the tiny synthetic data set -- its arguments, the stdout
  lines that start with "Epoch " or "Best Result:" and the checkpoint it wrote;
* evaluate_models: the same for scripts/evaluate_models.py -- the progress lines it
  printed before it stopped, its exit status and the last line of its traceback;
* metrics_error: the message the reference's metrics() raises on a 2-row batch at
  top_k 10;
* nmf: the reference's NMFRecommender on the tiny data set (n_components 1 and 6,
  random_state 43, max_iter 200): predictions at four (user, item) pairs, the
  parameter count and NMFEvaluator's (HR@10, NDCG@10).
"""
import ast
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from reference_usage import tiny_nmf_inputs  # noqa: E402
from ncf_amd import synthetic  # noqa: E402


def import_surface(ref):
    out = {}
    sdir = os.path.join(ref, "scripts")
    for name in sorted(os.listdir(sdir)):
        if not name.endswith(".py"):
            continue
        mods = {}
        for node in ast.walk(ast.parse(open(os.path.join(sdir, name)).read())):
            if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] == "src":
                mods.setdefault(node.module, []).extend(a.name for a in node.names)
        out[name] = {m: sorted(set(v)) for m, v in sorted(mods.items())}
    return out


def run_script(ref, script, cwd, *args):
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ref, "scripts", script), *args], cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=900)


def load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import torch
    from ncf_amd.models import NCF
    ref = os.path.abspath(sys.argv[1])
    out = {"import_surface": import_surface(ref)}
    ds = synthetic.make_dataset("tiny", seed=3)
    with tempfile.TemporaryDirectory() as tmp:
        synthetic.write_reference_files(ds, os.path.join(tmp, "data", "processed"))
        args = ["--epochs", "2", "--num_layers", "2"]
        r = run_script(ref, "train_neumf.py", tmp, *args)
        assert r.returncode == 0, r.stderr[-3000:]
        out["train_neumf"] = {
            "args": args,
            "lines": [x for x in r.stdout.splitlines() if x.startswith(("Epoch ", "Best Result:"))],
            "checkpoints": sorted(os.listdir(os.path.join(tmp, "results", "models")))}
        torch.manual_seed(0)
        m = NCF(ds["user_num"], ds["item_num"], 32, 2, 0.0, "NeuMF-end")
        torch.save(m.state_dict(), os.path.join(tmp, "results", "models", "NeuMF-end_pretrain_best.pth"))
        r = run_script(ref, "evaluate_models.py", tmp)
        out["evaluate_models"] = {
            "checkpoint": "NeuMF-end_pretrain_best.pth",
            "progress": [x.strip() for x in r.stdout.splitlines() if x.strip()],
            "figures": sorted(os.listdir(os.path.join(tmp, "results", "figures"))),
            "returncode": r.returncode, "error": r.stderr.strip().splitlines()[-1]}
    met = load(ref, "src/training/metrics.py", "ref_metrics")
    torch.manual_seed(0)
    m = NCF(10, 20, 8, 2, 0.0, "NeuMF-end")
    try:
        met.metrics(m, [(torch.tensor([1, 1]), torch.tensor([3, 4]), torch.tensor([0, 0]))], 10)
        raise AssertionError("the reference's metrics() did not raise")
    except RuntimeError as e:
        out["metrics_error"] = str(e).splitlines()[0]
    nmf = load(ref, "src/ncf/nmf_model.py", "ref_nmf_model")
    mat, test, uu, ii = tiny_nmf_inputs(ds)
    out["nmf"] = {}
    for n in (1, 6):
        a = nmf.NMFRecommender(n_components=n, random_state=43, max_iter=200).fit(mat)
        hr, nd = nmf.NMFEvaluator(a, test, mat).evaluate()
        out["nmf"][str(n)] = {"users": uu.tolist(), "items": ii.tolist(),
                              "predict": [float(x) for x in a.predict(uu, ii)],
                              "parameters": int(a.get_n_parameters()), "hr": float(hr), "ndcg": float(nd)}
    path = os.path.join(ROOT, "tests", "golden", "G14_reference_scripts.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
