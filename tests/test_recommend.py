"""CPU tests of full-catalogue top-K recommendation: NCF.recommend on a CPU model
against a brute-force ranking of the oracle's scores, ops.seen_csr,
metrics.full_rank_metrics against a hand computation and scripts/recommend.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from recommend_checks import check_topk, make_seen, oracle_scores  # noqa: E402

U, I = 50, 83
SHAPES = [("GMF", 8, 1), ("MLP", 8, 2), ("NeuMF-end", 16, 3)]


def _model(mt, f, nl, seed=0):
    from ncf_amd.models import NCF
    torch.manual_seed(seed)
    return NCF(U, I, f, nl, 0.0, mt)


@pytest.fixture(scope="module")
def seen():
    from ncf_amd import ops
    u, i = make_seen(U, I, np.random.default_rng(1))
    return ops.seen_csr(u, i, U, "cpu", I)


@pytest.mark.parametrize("mt,f,nl", SHAPES)
def test_cpu_recommend_matches_bruteforce(mt, f, nl, seen):
    m = _model(mt, f, nl)
    S = oracle_scores(m)
    rng = np.random.default_rng(2)
    every = np.arange(U)
    mixed = np.concatenate([rng.permutation(U)[:20], [5, 5, 7, 3, 0, 0]])  # shuffled, duplicates
    for users in (every, mixed):
        for k in (1, 10):
            for excl in (None, seen):
                items, scores = m.recommend(torch.as_tensor(users), k, excl)
                assert items.dtype == torch.int64 and scores.dtype == torch.float32
                check_topk(items, scores, users, S, k, excl)
    # user 5 has three eligible items: three results, then the -1 / -inf fill
    items, scores = m.recommend([5], 10, seen)
    assert (items[0, :3] >= 0).all() and (items[0, 3:] == -1).all() and torch.isneginf(scores[0, 3:]).all()
    assert sorted(items[0, :3].tolist()) == [1, I // 2, I - 1]
    # k above the catalogue size
    items, scores = m.recommend([0, 3], 100, None)
    check_topk(items, scores, [0, 3], S, 100, None)
    assert (items[:, I:] == -1).all() and (items[:, :I] >= 0).all()


@pytest.mark.parametrize("mt,f,nl", SHAPES)
def test_cpu_recommend_ties_lower_id_first(mt, f, nl):
    m = _model(mt, f, nl)
    with torch.no_grad():
        for emb in (m.embed_item_GMF, m.embed_item_MLP):
            emb.weight[60] = emb.weight[11]  # items 11 and 60 score the same for every user
    items, scores = m.recommend(torch.arange(U), I)
    items, scores = items.numpy(), scores.numpy()
    for q in range(U):
        a, b = np.where(items[q] == 11)[0][0], np.where(items[q] == 60)[0][0]
        assert scores[q, a] == scores[q, b] and b == a + 1


def test_recommend_eval_semantics_and_arguments():
    from ncf_amd.models import NCF
    torch.manual_seed(0)
    m = NCF(U, I, 8, 2, 0.5, "NeuMF-end")
    m.train()  # dropout on: recommend still scores in eval mode
    a = m.recommend([1, 2], 5)
    m.eval()
    b = m.recommend([1, 2], 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with torch.no_grad():
        want = m(torch.tensor([1] * 5), b[0][0])
    np.testing.assert_allclose(b[1][0].numpy(), want.numpy(), rtol=1e-5, atol=1e-7)
    for bad in (0, -1, 129, 2.5):
        with pytest.raises(ValueError):
            m.recommend([0], bad)
    with pytest.raises(IndexError):
        m.recommend([U], 3)
    items, scores = m.recommend([], 4)
    assert items.shape == scores.shape == (0, 4)


def test_seen_csr_from_arrays_and_dok():
    import scipy.sparse as sp
    from ncf_amd import ops
    u = np.array([2, 0, 2, 2, 0, 4, 2])
    i = np.array([7, 3, 1, 7, 3, 0, 5])
    s = ops.seen_csr(u, i, 5, "cpu")
    assert s.ptr.dtype == torch.int64 and s.items.dtype == torch.int32
    assert s.ptr.tolist() == [0, 1, 1, 4, 4, 5]
    assert s.items.tolist() == [3, 1, 5, 7, 0]
    mat = sp.dok_matrix((5, 9), dtype=np.float32)
    for a, b in zip(u, i):
        mat[a, b] = 1.0
    d = ops.seen_csr(mat)
    assert d.ptr.tolist() == s.ptr.tolist() and d.items.tolist() == s.items.tolist()
    with pytest.raises(IndexError):
        ops.seen_csr([0, 5], [1, 1], 5, "cpu")
    with pytest.raises(IndexError):
        ops.seen_csr([0, -1], [1, 1], 5, "cpu")
    with pytest.raises(IndexError):
        ops.seen_csr([0, 1], [1, 9], 5, "cpu", item_num=9)
    with pytest.raises(IndexError):
        ops.seen_csr([0, 1], [1, -2], 5, "cpu")
    empty = ops.seen_csr([], [], 3, "cpu")
    assert empty.ptr.tolist() == [0, 0, 0, 0] and empty.items.numel() == 0


def _hand_model():
    """GMF with score(user 0, i) = c[i] and score(user 1, i) = -c[i]."""
    from ncf_amd.models import NCF
    m = NCF(2, 5, 8, 1, 0.0, "GMF")
    c = torch.tensor([0.1, 0.5, 0.3, 0.2, 0.4])
    with torch.no_grad():
        m.embed_user_GMF.weight.zero_()
        m.embed_item_GMF.weight.zero_()
        m.embed_user_GMF.weight[0, 0] = 1.0
        m.embed_user_GMF.weight[1, 0] = -1.0
        m.embed_item_GMF.weight[:, 0] = c
        m.predict_layer.weight.fill_(1.0)
        m.predict_layer.bias.zero_()
    return m


def test_full_rank_metrics_hand_computation():
    from ncf_amd.metrics import full_rank_metrics
    from src.training.metrics import full_rank_metrics as reexport
    assert reexport is full_rank_metrics
    m = _hand_model()
    # user 0 ranks 1, 4, 2, 3, 0; user 1 ranks 0, 3, 2, 4, 1
    items, _ = m.recommend([0, 1], 5)
    assert items.tolist() == [[1, 4, 2, 3, 0], [0, 3, 2, 4, 1]]
    hr, nd = full_rank_metrics(m, [0, 1], [2, 1], 3)
    assert hr == [1, 0]
    assert nd == pytest.approx([1.0 / np.log2(4.0), 0.0])
    # item 1 excluded for user 0: its held-out item 2 moves up to position 1
    hr, nd = full_rank_metrics(m, [0, 1], [2, 3], 2, exclude=([0], [1]))
    assert hr == [1, 1]
    assert nd == pytest.approx([1.0 / np.log2(3.0), 1.0 / np.log2(3.0)])
    assert full_rank_metrics(m, [], [], 3) == ([], [])


def test_recommend_script_on_saved_checkpoint(tmp_path):
    m = _model("NeuMF-end", 8, 2, seed=3)
    ckpt = tmp_path / "model.pth"
    torch.save(m.state_dict(), ckpt)
    ids = tmp_path / "users.txt"
    ids.write_text("4\n0\n17\n4\n")
    out = tmp_path / "recs.npz"
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "recommend.py"), "--checkpoint", str(ckpt),
                    "--model", "NeuMF-end", "--top_k", "7", "--users", str(ids), "--out", str(out),
                    "--device", "cpu"], check=True, cwd=tmp_path, env=env, capture_output=True)
    z = np.load(out)
    items, scores = m.recommend([4, 0, 17, 4], 7)
    assert z["users"].tolist() == [4, 0, 17, 4]
    np.testing.assert_array_equal(z["items"], items.numpy())
    np.testing.assert_array_equal(z["scores"], scores.numpy())
