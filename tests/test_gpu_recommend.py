"""GPU tests of ncf_recommend (full-catalogue top-K) against the CPU oracle's logits over
every (user, item) pair: the fused score-and-select kernel on every kind of fused shape,
the materialised path, exclusion lists, determinism, ties, the agreement of the two
paths, Trainer.evaluate_full and graph capture.

Score tolerance: the project's logit gate (rtol 1e-5, atol 1e-7).  The ranking check is
tolerance based and leaves nothing out (tests/recommend_checks.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from recommend_checks import check_topk, make_seen, oracle_scores, seen_lists, tol  # noqa: E402

U, I = 300, 1007  # 1007: no multiple of 16 or of the 64-item chunk
DEV = "cuda:0"
FUSED = [("GMF", 8, 1), ("GMF", 64, 1), ("MLP", 8, 2), ("NeuMF-end", 8, 1), ("NeuMF-end", 16, 3),
         ("NeuMF-end", 8, 4), ("NeuMF-end", 32, 2), ("MLP", 64, 1), ("NeuMF-pre", 16, 3)]
MATERIALISED = [("NeuMF-end", 32, 3), ("MLP", 6, 2)]
SPECIAL = [3, 5, 7, 0]  # empty list, all but three items, ids around every multiple of 16, ordinary


def _model(mt, f, nl, seed=0):
    from ncf_amd.models import NCF
    torch.manual_seed(seed)
    return NCF(U, I, f, nl, 0.0, mt).to(DEV)


@pytest.fixture(scope="module")
def seen():
    from ncf_amd import ops
    u, i = make_seen(U, I, np.random.default_rng(1))
    return ops.seen_csr(u, i, U, DEV, I)


@pytest.fixture(scope="module")
def queries():
    rng = np.random.default_rng(2)
    mixed = np.concatenate([rng.permutation(U)[:30], [5, 5, 7, 3, 0, 0, 299]])  # Q = 37, shuffled, duplicates
    assert len(mixed) == 37
    return [np.arange(U), mixed] + [np.array([u]) for u in SPECIAL]


def _check_all(m, S, seen, queries):
    for users in queries:
        for k in (1, 10, 128):
            for excl in (None, seen):
                items, scores = m.recommend(torch.as_tensor(users), k, excl)
                assert items.dtype == torch.int64 and scores.dtype == torch.float32 and items.is_cuda
                check_topk(items, scores, users, S, k, excl)
    items, _ = m.recommend([5], 10, seen)  # three eligible items, then the fill
    assert sorted(items[0, :3].tolist()) == [1, I // 2, I - 1] and (items[0, 3:] == -1).all()


@pytest.mark.parametrize("mt,f,nl", FUSED + MATERIALISED)
def test_recommend_matches_oracle(mt, f, nl, seen, queries):
    import ncf_amd._lib as L
    assert L.supported(mt, f, nl) == (L.PATH_FUSED if (mt, f, nl) in FUSED else L.PATH_LAYERED)
    m = _model(mt, f, nl)
    _check_all(m, oracle_scores(m), seen, queries)


def _trained():
    """NeuMF-end(16, 3) after a few engine steps, so the scores spread."""
    from ncf_amd import ops
    from ncf_amd.engine import TrainEngine
    m = _model("NeuMF-end", 16, 3, seed=4)
    rng = np.random.default_rng(5)
    B = 2048
    u, i = rng.integers(0, U, B), rng.integers(0, I, B)
    y = ((u + i) % 3 == 0).astype(np.float32)
    eng = TrainEngine(m, lr=1e-2)
    eng.set_epoch_stream(ops.pack_rows(torch.as_tensor(u, dtype=torch.int32, device=DEV),
                                       torch.as_tensor(i, dtype=torch.int32, device=DEV),
                                       torch.as_tensor(y, dtype=torch.float32, device=DEV)), 256)
    eng.run(8, use_graph=False)
    torch.cuda.synchronize()
    return m


def test_recommend_trained_model(seen, queries):
    m = _trained()
    S = oracle_scores(m)
    assert S.std() > 1e-3  # the steps moved the scores apart
    _check_all(m, S, seen, queries)


@pytest.mark.parametrize("mt,f,nl", [("NeuMF-end", 16, 3), ("NeuMF-end", 32, 3)])
def test_recommend_is_deterministic(mt, f, nl, seen):
    m = _model(mt, f, nl)
    every = torch.arange(U)
    a = m.recommend(every, 10, seen)
    b = m.recommend(every, 10, seen)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # one query per user (other tiles, other splits of the item range): the same bits
    one = [m.recommend([u], 10, seen) for u in range(U)]
    assert torch.equal(torch.cat([x[0] for x in one]), a[0])
    assert torch.equal(torch.cat([x[1] for x in one]), a[1])


@pytest.mark.parametrize("mt,f,nl", [("GMF", 8, 1), ("NeuMF-end", 16, 3), ("NeuMF-end", 32, 3)])
def test_recommend_ties_lower_id_first(mt, f, nl):
    m = _model(mt, f, nl)
    best = int(m.recommend([17], 1)[0][0, 0])  # user 17's best item and a copy of it in another split
    copy = (best + 500) % I
    lo, hi = min(best, copy), max(best, copy)
    with torch.no_grad():
        for emb in (m.embed_item_GMF, m.embed_item_MLP):
            emb.weight[copy] = emb.weight[best]  # the two items score the same for every user
    for users in (torch.arange(U), torch.tensor([17])):
        items, scores = m.recommend(users, 128)
        items, scores = items.cpu().numpy(), scores.cpu().numpy()
        both = 0
        for q, u in enumerate(users.tolist()):
            a, b = np.where(items[q] == lo)[0], np.where(items[q] == hi)[0]
            # both or neither, unless the pair straddles the end of the list (then the lower id is in)
            if len(b):
                assert len(a) and b[0] == a[0] + 1 and scores[q, a[0]] == scores[q, b[0]], (q, u)
                both += 1
            elif len(a):
                assert a[0] == 127, (q, u)
        assert both > 0  # user 17 at least has the pair at the top


def test_two_paths_agree(seen):
    from ncf_amd import ops
    m = _model("NeuMF-end", 16, 3)
    S = oracle_scores(m)
    users = np.arange(U)
    k = 10
    fi, fs = m.recommend(torch.as_tensor(users), k, seen)
    with ops._recommend_materialised():
        mi, ms = m.recommend(torch.as_tensor(users), k, seen)
    check_topk(mi, ms, users, S, k, seen)
    fi, fs, mi, ms = fi.cpu().numpy(), fs.cpu().numpy(), mi.cpu().numpy(), ms.cpu().numpy()
    for q in range(U):
        fmap, mmap = dict(zip(fi[q], fs[q])), dict(zip(mi[q], ms[q]))
        fmap.pop(-1, None), mmap.pop(-1, None)
        for it in set(fmap) & set(mmap):
            assert abs(fmap[it] - mmap[it]) <= tol(S[q, it]), (q, it)
        kth = S[q, fi[q][fi[q] >= 0][-1]]
        for it in set(fmap) ^ set(mmap):  # only items tied with the k-th within the tolerances
            assert abs(S[q, it] - kth) <= 2 * tol(kth) + 2 * tol(S[q, it]), (q, it)


def _rank_bounds(S_u, excl, gt):
    """Positions the held-out item can take given the score tolerance: [lo, hi]."""
    elig = np.ones(len(S_u), dtype=bool)
    elig[excl] = False
    elig[gt] = False
    t = 2 * tol(S_u[gt])
    other = S_u[elig]
    return int((other > S_u[gt] + t).sum()), int((other >= S_u[gt] - t).sum())


def test_trainer_evaluate_full_matches_oracle():
    import torch.utils.data as data
    from ncf_amd import ops, synthetic
    from ncf_amd.data import NCFData
    from ncf_amd.models import NCF
    from ncf_amd.trainer import Trainer
    ds = synthetic.make_dataset("ml-100k", seed=0)
    Un, In = ds["user_num"], ds["item_num"]
    train = np.stack([ds["train_users"], ds["train_items"]], 1).astype(np.int64).tolist()
    tu = np.repeat(ds["test_users"], 100)
    ti = np.concatenate([ds["test_items"][:, None], ds["test_negatives"]], 1).reshape(-1)
    keep = ds["test_items"] < In  # a held-out item no training row mentions is outside the catalogue
    test = np.stack([tu, ti], 1).astype(np.int64).tolist()
    torch.manual_seed(0)
    model = NCF(Un, In, 8, 3, 0.0, "NeuMF-end").to(DEV)
    loader = data.DataLoader(NCFData(test, In, None, 0, False), batch_size=100, shuffle=False, num_workers=0)
    tr = Trainer(model, NCFData(train, In, None, 4, True), loader, batch_size=256, top_k=10)
    state = torch.get_rng_state()
    default = tr.evaluate_full()
    assert torch.equal(state, torch.get_rng_state())
    assert tr.evaluate_full(10) == default
    S = oracle_scores(model)
    lists = seen_lists(ops.seen_csr(ds["train_users"], ds["train_items"], Un, "cpu", In), Un)
    for k in (10, 100):
        hr, nd = tr.evaluate_full(k)
        assert len(hr) == len(nd) == len(ds["test_users"])
        decided = 0
        for q, (u, gt) in enumerate(zip(ds["test_users"].tolist(), ds["test_items"].tolist())):
            if not keep[q]:
                assert hr[q] == 0 and nd[q] == 0.0
                continue
            lo, hi = _rank_bounds(S[u], lists[u], gt)
            allowed = {(1, 1.0 / np.log2(p + 2.0)) if p < k else (0, 0.0) for p in range(lo, hi + 1)}
            assert any(hr[q] == h and abs(nd[q] - n) < 1e-12 for h, n in allowed), (q, u, lo, hi, hr[q], nd[q])
            decided += len(allowed) == 1
        assert decided > 0.9 * len(hr)  # the tolerance leaves almost every user's metric determined
    assert 0 < sum(hr) < len(hr)  # k = 100: hits and misses


def test_recommend_captured_in_a_graph(seen):
    from ncf_amd import ops
    m = _model("NeuMF-end", 16, 3)
    k = 10
    users = torch.arange(U, dtype=torch.int32, device=DEV)
    eager_i, eager_s = ops.recommend(m, users, k, seen)  # also the one-time kernel attribute call
    flat, lay = ops.ensure_flat(m)
    ws = ops.recommend_workspace(lay, U, k, m, torch.device(DEV))
    items = torch.zeros((U, k), dtype=torch.int32, device=DEV)
    scores = torch.zeros((U, k), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # one linear capture
        ops.recommend_into(flat, lay, users, k, seen, items, scores, ws)
    items.zero_()
    scores.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(items, eager_i) and torch.equal(scores, eager_s)


def test_documented_recommend_stub(seen):
    """the section-2 binding and the section-5 stub, executed as written."""
    import re
    from ncf_amd import ops
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec2 = text.split("## 2.", 1)[1].split("\n## 3.", 1)[0]
    sec5 = text.split("## 5.", 1)[1]
    blocks = re.findall(r"```python\n(.*?)```", sec2, re.S) + re.findall(r"```python\n(.*?)```", sec5, re.S)
    lib = os.path.join(ROOT, "ncf_amd", "libncf_hip.so")
    ns = {}
    for b in blocks:
        exec(compile(b.replace("/path/to/ncf_amd/libncf_hip.so", lib), "INTEGRATION.md", "exec"), ns)
    m = _model("NeuMF-end", 16, 3)
    flat, _ = ops.ensure_flat(m)
    users = torch.arange(U, dtype=torch.int32, device=DEV)
    items, scores = ns["recommend"](flat, ns["layout"](m), users, 10, seen.ptr, seen.items)
    want_i, want_s = ops.recommend(m, users, 10, seen)
    assert torch.equal(items, want_i) and torch.equal(scores, want_s)


def test_recommend_argument_errors():
    import ncf_amd._lib as L
    from ncf_amd import ops
    m = _model("GMF", 8, 1)
    for bad in (0, 129):
        with pytest.raises(ValueError):
            m.recommend([0], bad)
    with pytest.raises(IndexError):
        m.recommend([U], 5)
    flat, lay = ops.ensure_flat(m)
    lib = L.hip()
    assert lib.ncf_recommend_workspace_bytes(ctypes.byref(lay), 4, 129) == -1
    u = torch.zeros(4, dtype=torch.int32, device=DEV)
    out_i = torch.zeros((4, 128), dtype=torch.int32, device=DEV)
    out_s = torch.zeros((4, 128), dtype=torch.float32, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.float32, device=DEV)
    call = lambda n, k: lib.ncf_recommend(ctypes.byref(lay), flat.data_ptr(), u.data_ptr(), n, k, None, None,  # noqa: E731
                                          out_i.data_ptr(), out_s.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                          L.stream_ptr(torch.device(DEV)))
    assert call(4, 0) == L.NCF_E_ARG and call(4, 129) == L.NCF_E_ARG
    assert call(0, 5) == L.NCF_OK
    items, scores = m.recommend([], 5)
    assert items.shape == scores.shape == (0, 5)
