"""CPU tests of the nearest-neighbour queries: NCF.similar_items / NCF.similar_users on a
CPU model against the float64 reference of tests/neighbors_checks.py, the argument
errors, scripts/similar.py, and the header's declarations against ncf_amd._lib."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import neighbors_checks as NC  # noqa: E402
from ncf_amd.models import NCF  # noqa: E402

U, I = 50, 80
SPACES = ["gmf", "mlp", "concat"]
METRICS = ["cosine", "dot"]


def _model(model_type="NeuMF-end", f=8, layers=3, seed=0):
    torch.manual_seed(seed)
    m = NCF(U, I, f, layers, 0.0, model_type)
    with torch.no_grad():
        for emb in (m.embed_user_GMF, m.embed_item_GMF, m.embed_user_MLP, m.embed_item_MLP):
            emb.weight.normal_(0.0, 1.0)
    return m.eval()


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("side", ["item", "user"])
def test_cpu_path_against_reference(model, side, space, metric):
    n = I if side == "item" else U
    queries = np.arange(n)
    table = NC.table64(model, side, space)
    S, T = NC.reference(table, queries, metric)
    fn = model.similar_items if side == "item" else model.similar_users
    for k, excl in ((1, True), (10, True), (10, False), (128, True)):
        ids, scores = fn(queries, k, space=space, metric=metric, exclude_self=excl)
        assert ids.dtype == torch.int64 and scores.dtype == torch.float32
        NC.check_neighbors(ids, scores, queries, S, T, k, excl)


@pytest.mark.parametrize("model_type,space", [("GMF", "gmf"), ("MLP", "mlp"), ("NeuMF-end", "concat"),
                                              ("NeuMF-pre", "concat")])
def test_default_space_per_model_type(model_type, space):
    m = _model(model_type, 8, 3, seed=1)
    q = [3, 0, 41]
    for fn in (m.similar_items, m.similar_users):
        got = fn(q, 5)
        want = fn(q, 5, space=space, metric="cosine", exclude_self=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    other = "mlp" if space == "gmf" else "gmf"
    assert not torch.equal(m.similar_items(q, 5)[1], m.similar_items(q, 5, space=other)[1])


def test_self_first_and_zero_row(model):
    m = _model(seed=2)
    with torch.no_grad():
        m.embed_item_GMF.weight[7].zero_()
        m.embed_item_MLP.weight[7].zero_()
    ids, scores = m.similar_items(np.arange(I), 4, exclude_self=False)
    keep = np.arange(I) != 7
    assert (ids[keep, 0].numpy() == np.arange(I)[keep]).all()
    assert np.abs(scores[keep, 0].numpy() - 1.0).max() <= 1.01 * (2 * 40 + 10) * NC.U_FP32
    assert not torch.isnan(scores).any()
    # the zero row scores 0 against everything: ties in ascending id order
    assert ids[7].tolist() == [0, 1, 2, 3] and (scores[7] == 0).all()
    ids, scores = m.similar_items([7], 4)
    assert ids[0].tolist() == [0, 1, 2, 3] and (scores[0] == 0).all()


def test_fill_beyond_the_table(model):
    ids, scores = model.similar_users([5], 128)
    assert (ids[0, :U - 1] >= 0).all() and (ids[0, U - 1:] == -1).all()
    assert torch.isneginf(scores[0, U - 1:]).all() and torch.isfinite(scores[0, :U - 1]).all()


def test_argument_errors(model):
    for bad in (dict(space="tower"), dict(metric="l2"), dict(space=1), dict(metric=None)):
        with pytest.raises(ValueError):
            model.similar_items([0], 3, **bad)
        with pytest.raises(ValueError):
            model.similar_users([0], 3, **bad)
    for k in (0, 129, 2.5, True):
        with pytest.raises(ValueError):
            model.similar_items([0], k)
    with pytest.raises(IndexError, match="index out of range in self"):
        model.similar_items([0, I], 3)
    with pytest.raises(IndexError, match="index out of range in self"):
        model.similar_users([-1], 3)
    with pytest.raises(IndexError, match="index out of range in self"):
        model.similar_users([U], 3)
    model.similar_items([U], 3)  # a valid item id (I > U)


def test_no_queries(model):
    for fn in (model.similar_items, model.similar_users):
        ids, scores = fn([], 6)
        assert ids.shape == scores.shape == (0, 6)
        assert ids.dtype == torch.int64 and scores.dtype == torch.float32


def test_similar_script_on_saved_checkpoint(tmp_path):
    m = _model("NeuMF-end", 8, 2, seed=3)
    ckpt = tmp_path / "model.pth"
    torch.save(m.state_dict(), ckpt)
    ids = tmp_path / "ids.txt"
    ids.write_text("4\n0\n17\n4\n")
    out = tmp_path / "sim.npz"
    env = dict(os.environ, PYTHONPATH=ROOT)
    script = os.path.join(ROOT, "scripts", "similar.py")
    done = subprocess.run([sys.executable, script, "--checkpoint", str(ckpt), "--model", "NeuMF-end", "--side", "user",
                           "--ids", str(ids), "--top_k", "7", "--space", "mlp", "--metric", "dot", "--keep_self",
                           "--out", str(out), "--device", "cpu"], check=True, cwd=tmp_path, env=env,
                          capture_output=True, text=True)
    assert len(done.stdout.strip().splitlines()) == 1 and "top-7" in done.stdout
    z = np.load(out)
    want_i, want_s = m.similar_users([4, 0, 17, 4], 7, space="mlp", metric="dot", exclude_self=False)
    assert z["queries"].tolist() == [4, 0, 17, 4]
    np.testing.assert_array_equal(z["ids"], want_i.numpy())
    np.testing.assert_array_equal(z["scores"], want_s.numpy())


def test_header_declares_what_lib_carries():
    import ncf_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "ncf_hip.h")).read()
    defines = dict(re.findall(r"#define (NCF_(?:SIDE|SPACE|SIM)_[A-Z]+) (\d+)", hdr))
    assert {k: int(v) for k, v in defines.items()} == {
        "NCF_SIDE_USER": L.SIDE_USER, "NCF_SIDE_ITEM": L.SIDE_ITEM, "NCF_SPACE_GMF": L.SPACE_GMF,
        "NCF_SPACE_MLP": L.SPACE_MLP, "NCF_SPACE_CONCAT": L.SPACE_CONCAT, "NCF_SIM_COSINE": L.SIM_COSINE,
        "NCF_SIM_DOT": L.SIM_DOT}
    assert (L.SIDE_USER, L.SIDE_ITEM, L.SPACE_GMF, L.SPACE_MLP, L.SPACE_CONCAT, L.SIM_COSINE, L.SIM_DOT) == \
        (0, 1, 0, 1, 2, 0, 1)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int64_t\s+ncf_neighbors_workspace_bytes\s*\(", code)
    assert re.search(r"\bint\s+ncf_neighbors\s*\(", code)
    assert int(re.search(r"#define NCF_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION
    for name, nargs in (("ncf_neighbors_workspace_bytes", 5), ("ncf_neighbors", 14)):
        assert len(L._HIP_PROTOS[name][1]) == nargs
        assert hasattr(L.hip(), name)
