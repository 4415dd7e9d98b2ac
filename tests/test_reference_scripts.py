"""The reference scripts' use of this repo's ``src/`` import surface (CPU), checked
without the reference checkout against a record of its own scripts run unchanged on
this ``src/`` (tests/golden/G14_reference_scripts.json, written by
tests/golden/make_golden_refscripts.py -- names and results only).  The record itself
documents what those runs did; the tests assert what this repository's code does:
every recorded name resolves, and the calls behind it behave as the record says.

* scripts/train_neumf.py   (NCF, NCFData, load_all, config, metrics)
* scripts/evaluate_models.py  (src.ncf.nmf_model.run_nmf_experiment, which the
  reference itself lacks, then metrics at several K and test batch sizes up to the
  point where the reference's own metrics() raises)
* the NMF baseline classes against the reference's src/ncf/nmf_model.py."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from reference_usage import tiny_nmf_inputs  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "G14_reference_scripts.json")) as f:
        return json.load(f)


@pytest.fixture
def tiny_dir(tmp_path, monkeypatch):
    """The tiny data set as the reference's processed files, in the working directory."""
    from ncf_amd import synthetic
    ds = synthetic.make_dataset("tiny", seed=3)
    synthetic.write_reference_files(ds, str(tmp_path / "data" / "processed"))
    monkeypatch.chdir(tmp_path)
    return tmp_path, ds


def _surface(recorded, script):
    """The names `script` imports from src.*, resolved here: {name: object}."""
    mods = recorded["import_surface"][script]
    assert mods, script
    out = {}
    for mod, names in mods.items():
        m = importlib.import_module(mod)
        for n in names:
            assert hasattr(m, n), f"{script}: from {mod} import {n}"
            out[n] = getattr(m, n)
    return out


def test_reference_train_neumf_runs_on_our_src(tiny_dir, recorded):
    """Every name the reference's train_neumf.py imports from src.* resolves here and
    does on the CPU what that script needs of it: load_all reads the processed files,
    NCFData samples negatives and feeds a stock DataLoader, NCF trains a step on stock
    torch, metrics() returns one HR and NDCG per test user, and the checkpoint the
    recorded run wrote loads back."""
    import torch
    import torch.utils.data as data
    cwd, ds = tiny_dir
    api = _surface(recorded, "train_neumf.py")
    NCF, NCFData, load_all, config, metrics = (api[k] for k in ("NCF", "NCFData", "load_all", "config", "metrics"))
    train_data, test_data, user_num, item_num, train_mat = load_all()
    assert (user_num, item_num) == (ds["user_num"], ds["item_num"]) and len(train_data) == len(ds["train_users"])
    train_set = NCFData(train_data, item_num, train_mat, config.num_ng, True)
    train_set.ng_sample()
    assert len(train_set) == (1 + config.num_ng) * len(train_data)
    user, item, label = next(iter(data.DataLoader(train_set, batch_size=config.batch_size, shuffle=True)))
    torch.manual_seed(0)
    model = NCF(user_num, item_num, config.factor_num, 2, config.dropout, "NeuMF-end")
    opt = torch.optim.Adam(model.parameters(), lr=config.lr)
    loss = torch.nn.BCEWithLogitsLoss()(model(user, item), label.float())
    loss.backward()
    opt.step()
    assert 0.5 < loss.item() < 0.9
    test_set = NCFData(test_data, item_num, train_mat, 0, False)
    loader = data.DataLoader(test_set, batch_size=config.test_num_ng + 1, shuffle=False)
    model.eval()
    HR, NDCG = metrics(model, loader, config.top_k)
    assert len(HR) == len(NDCG) == len(ds["test_users"]) and 0 <= np.mean(NDCG) <= np.mean(HR) <= 1
    name = recorded["train_neumf"]["checkpoints"][0]
    assert name == f"NeuMF_end_2l_{config.factor_num}f_best.pth"
    config.model_dir.mkdir(parents=True, exist_ok=True)  # relative to the working directory, as in the reference
    torch.save(model.state_dict(), config.model_dir / name)
    assert (cwd / "results" / "models" / name).exists()
    NCF(user_num, item_num, config.factor_num, 2, config.dropout, "NeuMF-end").load_state_dict(
        torch.load(config.model_dir / name, map_location="cpu"))


def test_reference_evaluate_models_runs_on_our_src(tiny_dir, recorded):
    """On the reference itself the script dies at import (no run_nmf_experiment).
    With this src/ it loads the checkpoint, runs and plots the Top-K sweep, then
    stops exactly where the reference's own metrics() would: the negative-sampling
    sweep evaluates DataLoader batches of num_neg + 1 = 2 rows at top_k = 10, and
    torch.topk raises "selected index k out of range" (metrics.py:13,
    evaluate_models.py:39-45).  Same error, same point: parity, not a fix.  The
    record says where the reference's script stopped; the same calls stop there here."""
    import torch
    import torch.utils.data as data
    cwd, ds = tiny_dir
    api = _surface(recorded, "evaluate_models.py")
    assert callable(api["run_nmf_experiment"])
    NCF, NCFData, load_all, config, metrics = (api[k] for k in ("NCF", "NCFData", "load_all", "config", "metrics"))
    rec = recorded["evaluate_models"]
    torch.manual_seed(0)
    m = NCF(ds["user_num"], ds["item_num"], 32, 2, 0.0, "NeuMF-end")
    config.model_dir.mkdir(parents=True, exist_ok=True)  # relative to the working directory, as in the reference
    torch.save(m.state_dict(), config.model_dir / rec["checkpoint"])
    train_data, test_data, user_num, item_num, train_mat = load_all()
    model = NCF(user_num, item_num, config.factor_num, config.num_layers, config.dropout, "NeuMF-end")
    model.load_state_dict(torch.load(config.model_dir / rec["checkpoint"], map_location="cpu"))
    model.eval()
    test_set = NCFData(test_data, item_num, train_mat, 0, False)
    loader = data.DataLoader(test_set, batch_size=config.test_num_ng + 1, shuffle=False)
    hr = [np.mean(metrics(model, loader, k)[0]) for k in range(1, 11)]  # the Top-K sweep
    assert all(a <= b for a, b in zip(hr, hr[1:])) and 0 < hr[-1] <= 1
    # the record's last progress line is the sweep's first point: 1 negative, batches of 2
    assert rec["progress"][-1] == "Evaluating with 1 negative samples..."
    with pytest.raises(RuntimeError) as e:
        metrics(model, data.DataLoader(test_set, batch_size=2, shuffle=False), 10)
    assert rec["error"] == f"RuntimeError: {str(e.value).splitlines()[0]}"


def test_reference_metrics_raise_like_ours(recorded):
    """The reference's metrics() on a 2-row batch with top_k=10 raised the recorded
    error; ours raises the same one."""
    import torch
    from ncf_amd.metrics import metrics
    from ncf_amd.models import NCF
    torch.manual_seed(0)
    m = NCF(10, 20, 8, 2, 0.0, "NeuMF-end")
    loader = [(torch.tensor([1, 1]), torch.tensor([3, 4]), torch.tensor([0, 0]))]
    with pytest.raises(RuntimeError, match="k out of range") as e:
        metrics(m, loader, 10)
    assert str(e.value).splitlines()[0] == recorded["metrics_error"]


def test_nmf_baseline_matches_reference_classes(tiny_dir, recorded):
    """Our NMF classes against what the reference's classes gave when recorded, on the
    same matrix and settings.  The recorded predictions come from another run of
    scikit-learn's 200 multiplicative updates in float32, possibly on another CPU: rtol
    1e-4 (a few hundred roundings of 6e-8 each) plus 1e-7.  The parameter count is
    exact; HR@10 and NDCG@10 over the 60 test users are compared as recorded (one rank
    changing place would move HR by 1/60)."""
    from ncf_amd import nmf
    _, ds = tiny_dir
    U, I = ds["user_num"], ds["item_num"]
    mat, test, uu, ii = tiny_nmf_inputs(ds)
    for n in (1, 6):
        rec = recorded["nmf"][str(n)]
        assert rec["users"] == uu.tolist() and rec["items"] == ii.tolist()
        b = nmf.NMFRecommender(n_components=n, random_state=43, max_iter=200).fit(mat)
        np.testing.assert_allclose(b.predict(uu, ii), rec["predict"], rtol=1e-4, atol=1e-7)
        assert b.get_n_parameters() == rec["parameters"]
        assert nmf.NMFEvaluator(b, test, mat).evaluate() == pytest.approx((rec["hr"], rec["ndcg"]), rel=1e-6)
    res = nmf.run_nmf_experiment(mat, test, [1, 6], num_runs=2, max_iter=100)
    assert set(res) == {1, 6} and set(res[1]) >= {"hr_mean", "hr_std", "ndcg_mean", "ndcg_std", "parameters"}
    assert res[6]["parameters"] == (U + I) * 6
