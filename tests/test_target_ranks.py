"""Target ranks on the CPU: NCF.target_ranks' stock-torch path against the definition
(tests/target_checks.py exact_ranks over the model's own eval-mode logits), its input forms and
errors, metrics.rank_report against a brute-force evaluation of every formula, and the
agreement with full_rank_metrics.  No GPU needed."""
import numpy as np
import pytest
import torch

import rank_checks as R
import recommend_checks as RC
import target_checks as T
from test_gpu_rank import FUSED_MODELS

U, I = 50, 80


def _model(mt, f, Lyr, seed=11):
    from ncf_amd.models import NCF
    torch.manual_seed(seed)
    return NCF(U, I, f, Lyr, 0.0, mt)


def _scores(model):
    """[U, I] eval-mode logits of the model itself, every pair in one call."""
    with torch.no_grad():
        z = model._logits_eval(torch.arange(U).repeat_interleave(I), torch.arange(I).repeat(U))
    return z.view(U, I).numpy()


def _seen():
    from ncf_amd import ops
    su, si = RC.make_seen(U, I, np.random.default_rng(2))
    return ops.seen_csr(su, si, U, "cpu", I)


def _lists(ptr, tgt):
    from ncf_amd import ops
    return ops.CandidateLists(torch.from_numpy(ptr), torch.from_numpy(tgt))


# --------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("mt,f,Lyr", FUSED_MODELS)
@pytest.mark.parametrize("exclude", [False, True])
def test_cpu_path_is_the_definition(mt, f, Lyr, exclude):
    model = _model(mt, f, Lyr)
    Z = _scores(model)
    seen = _seen() if exclude else None
    users, ptr, tgt = R.ragged(R.cycle_lengths(20), U, I)
    users[:3] = (3, 5, 7)  # nothing seen; all but three seen; the tile edges seen
    r = model.target_ranks(users, _lists(ptr, tgt), exclude=seen)
    assert r.ranks.dtype == torch.int64 and r.scores.dtype == torch.float32
    assert np.array_equal(r.ranks.numpy(), T.exact_ranks(Z, users, ptr, tgt, seen))
    owner = np.repeat(np.arange(20), np.diff(ptr))
    assert np.array_equal(r.scores.numpy().view(np.uint32), Z[users[owner], tgt].view(np.uint32))
    lens = np.array([len(x) for x in RC.seen_lists(seen, U)])
    assert np.array_equal(r.eligible.numpy(), I - lens[users]) and np.array_equal(r.ptr.numpy(), ptr)
    # small chunks give the same result: a list's rank does not depend on the chunking
    few = model._target_ranks_cpu(torch.as_tensor(users), _lists(ptr, tgt), seen, chunk_pairs=97 * I)
    assert torch.equal(few.ranks, r.ranks)


def test_seen_target_is_ranked_as_if_eligible():
    model = _model("NeuMF-end", 8, 3)
    Z = _scores(model)
    seen = _seen()
    mine = RC.seen_lists(seen, U)[5]  # all but three seen
    assert len(mine) == I - 3
    tgt = np.concatenate([mine[:10], np.setdiff1d(np.arange(I), mine)]).astype(np.int32)
    r = model.target_ranks([5], [tgt], exclude=seen)
    assert r.eligible.tolist() == [3]
    order = sorted(np.setdiff1d(np.arange(I), mine), key=lambda j: (-Z[5, j], j))
    for t, rank in zip(tgt.tolist(), r.ranks.tolist()):
        ahead = [j for j in order if j != t and (Z[5, j] > Z[5, t] or (Z[5, j] == Z[5, t] and j < t))]
        assert rank == len(ahead) <= 3
    assert sorted(r.ranks[10:].tolist()) == [0, 1, 2]  # the three eligible items hold the three positions


def test_duplicates_and_ties():
    model = _model("NeuMF-end", 8, 3)
    with torch.no_grad():  # items 9 and 30 are one item: equal scores for every user, the lower id first
        for emb in (model.embed_item_GMF, model.embed_item_MLP):
            emb.weight[30] = emb.weight[9]
    r = model.target_ranks([4, 4], [[9, 30, 9, 12, 30], [30]])
    a, b = r.ranks[:5].tolist(), r.scores[:5]
    assert a[0] == a[2] and a[1] == a[4]  # duplicates: equal ranks
    assert a[1] == a[0] + 1               # the tie: id 9 right in front of id 30
    assert b[0] == b[1] == b[2] == b[4]
    assert r.ranks[5] == a[1]             # the other targets of a list are ordinary competitors
    Z = _scores(model)
    assert np.array_equal(r.ranks.numpy(), T.exact_ranks(Z, [4, 4], [0, 5, 6], [9, 30, 9, 12, 30, 30], None))


def test_input_forms_agree():
    from ncf_amd import ops
    model = _model("MLP", 16, 2)
    seen = _seen()
    rng = np.random.default_rng(0)
    users = rng.integers(0, U, 12)
    tgt = rng.integers(0, I, (12, 3))
    wide = model.target_ranks(users, tgt, exclude=seen)
    assert wide.ranks.shape == wide.scores.shape == (12, 3)
    rag = model.target_ranks(users, [row for row in tgt], exclude=seen)
    cl = model.target_ranks(users, ops.candidate_lists(tgt), exclude=seen)
    assert rag.ranks.shape == (36,)
    for x in (rag, cl):
        assert torch.equal(x.ranks, wide.ranks.reshape(-1)) and torch.equal(x.scores, wide.scores.reshape(-1))
        assert torch.equal(x.ptr, wide.ptr) and torch.equal(x.eligible, wide.eligible)
    one = model.target_ranks(users, tgt[:, 0], exclude=seen)  # 1-D: one target per user
    col = model.target_ranks(users, tgt[:, :1], exclude=seen)
    assert one.ranks.shape == (12,) and torch.equal(one.ranks, col.ranks[:, 0])
    assert torch.equal(one.ptr, torch.arange(13))
    dok_like = (np.repeat(np.arange(U), 2), np.tile([0, 1], U))  # exclude as a (users, items) pair
    assert (model.target_ranks(users, tgt[:, 0], exclude=dok_like).eligible == I - 2).all()
    assert (model.target_ranks(users, tgt[:, 0]).eligible == I).all()


def test_errors():
    from ncf_amd import ops
    model = _model("GMF", 16, 1)
    users, ptr, tgt = R.ragged(R.cycle_lengths(12), U, I)
    bad = tgt.copy()
    bad[5] = I
    with pytest.raises(IndexError):
        model.target_ranks(users, _lists(ptr, bad))
    with pytest.raises(IndexError):
        model.target_ranks(np.full(12, U), _lists(ptr, tgt))
    with pytest.raises(IndexError):
        model.target_ranks(users, np.full(12, -1))
    with pytest.raises(ValueError):
        model.target_ranks(users[:11], _lists(ptr, tgt))       # users / ptr length mismatch
    with pytest.raises(ValueError):
        model.target_ranks(users, tgt[:11])                    # 1-D is one target per user
    with pytest.raises(ValueError):
        model.target_ranks(users, np.zeros((11, 2), dtype=np.int64))
    with pytest.raises(ValueError):
        model.target_ranks(users, np.zeros((12, 2, 2), dtype=np.int64))
    with pytest.raises(ValueError):
        model.target_ranks(users, _lists(ptr[::-1].copy(), tgt))  # non-monotone ptr
    with pytest.raises(ValueError):
        model.target_ranks(users, tgt[:12], exclude=ops.SeenCSR(torch.zeros(3, dtype=torch.int64),
                                                                torch.zeros(0, dtype=torch.int32)))
    none = model.target_ranks(users[:0], np.zeros((0, 4), dtype=np.int64))
    assert none.ranks.shape == (0, 4) and none.eligible.shape == (0,)
    empty = model.target_ranks(users[:4], [[], [], [], []])
    assert empty.ranks.shape == (0,) and empty.ptr.tolist() == [0] * 5


# --------------------------------------------------------------------------- against recommend's metrics
@pytest.mark.parametrize("k", [1, 10, 128])
def test_reproduces_full_rank_metrics(k):
    from ncf_amd.metrics import full_rank_metrics, rank_report
    from ncf_amd.models import NCF
    torch.manual_seed(3)
    model = NCF(60, 300, 8, 3, 0.0, "NeuMF-end")  # 300 items: ranks on both sides of 128
    rng = np.random.default_rng(1)
    users = np.arange(60)
    mask = rng.random((60, 300)) < 0.1
    gt = rng.integers(0, 300, 60)
    mask[users, gt] = False  # the held-out item is not a training positive
    seen = np.nonzero(mask)
    hr, nd = full_rank_metrics(model, users, gt, k, exclude=seen)
    r = model.target_ranks(users, gt, exclude=seen)
    ranks = r.ranks.numpy()
    assert hr == (ranks < k).astype(int).tolist()
    assert nd == np.where(ranks < k, 1.0 / np.log2(ranks + 2.0), 0.0).tolist()
    rep = rank_report(r.ranks, r.ptr, r.eligible, ks=(k,))
    assert np.array_equal(rep["per_user"][f"hr@{k}"], np.array(hr, dtype=np.float64))
    assert np.array_equal(rep["per_user"][f"ndcg@{k}"], np.array(nd))  # one target: the ideal DCG is 1
    assert (ranks >= 128).any() and (ranks < 10).any()


# --------------------------------------------------------------------------- rank_report
def _brute(Z, held, seen_mask, ks):
    """Every formula of rank_report evaluated user by user from the sorted list of eligible items."""
    out = {}
    n = len(held)
    for q in range(n):
        targets = held[q]
        free = ~seen_mask[q]
        free[targets] = True
        order = sorted(np.nonzero(free)[0], key=lambda j: (-Z[q, j], j))
        rel = np.array([j in set(targets) for j in order])
        P, E = len(targets), len(order)
        pos = np.nonzero(rel)[0]
        vals = {}
        for k in ks:
            top = rel[:k]
            vals[f"hr@{k}"] = float(top.any())
            vals[f"recall@{k}"] = top.sum() / P
            vals[f"precision@{k}"] = top.sum() / k
            dcg = sum(1.0 / np.log2(i + 2.0) for i in range(min(k, E)) if rel[i])
            vals[f"ndcg@{k}"] = dcg / sum(1.0 / np.log2(i + 2.0) for i in range(min(P, k)))
        vals["mrr"] = 1.0 / (pos[0] + 1.0)
        vals["map"] = np.mean([rel[:p + 1].sum() / (p + 1.0) for p in pos])
        neg = np.nonzero(~rel)[0]
        pairs = sum((p < neg).sum() for p in pos)  # (positive, negative) pairs in the right order
        vals["auc"] = pairs / (P * (E - P)) if E > P else np.nan
        vals["mean_rank"] = pos.mean()
        for name, v in vals.items():
            out.setdefault(name, []).append(v)
    return {k: np.array(v, dtype=np.float64) for k, v in out.items()}


def test_rank_report_is_brute_force():
    from ncf_amd.metrics import rank_report
    rng = np.random.default_rng(9)
    n, items = 40, 120
    ks = (1, 5, 10, 20, 50, 100)
    Z = rng.standard_normal((n, items)).astype(np.float32)
    Z[:, 7] = Z[:, 3]  # ties
    seen_mask = rng.random((n, items)) < 0.2
    held = [rng.choice(items, rng.integers(1, 8), replace=False) for _ in range(n)]
    held[4] = np.arange(items)[~seen_mask[4]][:7]
    seen_mask[5] = True  # every item but the held-out ones seen: E = P, no AUC
    for q in range(n):
        seen_mask[q, held[q]] = False
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(h) for h in held], out=ptr[1:])
    ranks = []
    for q in range(n):
        free = ~seen_mask[q]
        for t in held[q]:
            ahead = (Z[q] > Z[q, t]) | ((Z[q] == Z[q, t]) & (np.arange(items) < t))
            ahead[t] = False
            ranks.append(int((ahead & free).sum()))
    eligible = (~seen_mask).sum(1)
    rep = rank_report(np.array(ranks), ptr, eligible, ks)
    want = _brute(Z, held, seen_mask, ks)
    assert rep["users"] == n and set(rep["per_user"]) == set(want)
    for name, w in want.items():
        np.testing.assert_allclose(rep["per_user"][name], w, rtol=1e-12, atol=1e-12, err_msg=name)
        ok = ~np.isnan(w)
        assert rep["mean"][name] == pytest.approx(w[ok].mean(), rel=1e-12), name
    assert np.isnan(rep["per_user"]["auc"][5]) and not np.isnan(rep["mean"]["auc"])
    # users without held-out items are NaN and outside the means; torch tensors are taken
    ptr2 = np.concatenate([[0], ptr])  # an empty list in front
    rep2 = rank_report(torch.as_tensor(ranks), torch.as_tensor(ptr2), np.concatenate([[items], eligible]), ks)
    assert rep2["users"] == n and np.isnan(rep2["per_user"]["mrr"][0])
    assert rep2["mean"] == pytest.approx(rep["mean"], nan_ok=True)
    with pytest.raises(ValueError):
        rank_report([3, 3], [0, 2], [10])  # two equal ranks in one list: duplicate targets
    assert rank_report([3, 3], [0, 1, 2], [10, 10])["mean"]["mrr"] == 0.25
    with pytest.raises(ValueError):
        rank_report([1, 2], [0, 3], [10])
    with pytest.raises(ValueError):
        rank_report([1, 2], [0, 2], [10], ks=(0,))


def test_full_rank_report_chains_the_two():
    from ncf_amd.metrics import full_rank_report, rank_report
    model = _model("NeuMF-end", 8, 3)
    seen = _seen()
    users = np.array([3, 7, 11, 20])
    held = [[1, 2, 3], [40], [], [5, 79]]
    rep = full_rank_report(model, users, held, ks=(5, 10), exclude=seen)
    r = model.target_ranks(users, held, exclude=seen)
    want = rank_report(r.ranks, r.ptr, r.eligible, ks=(5, 10))
    assert rep["users"] == 3 and rep["mean"] == pytest.approx(want["mean"], nan_ok=True)
    assert set(rep["mean"]) == {"hr@5", "recall@5", "precision@5", "ndcg@5", "hr@10", "recall@10", "precision@10",
                                "ndcg@10", "mrr", "map", "auc", "mean_rank"}


# --------------------------------------------------------------------------- the synthetic dataset
def test_synthetic_heldout_ranks_are_full_rank_metrics():
    """What Trainer.evaluate_ranks and Trainer.evaluate_full compute (the Trainer itself needs a
    HIP device: tests/test_gpu_target_ranks.py), on a CPU model: every test user's held-out item
    against the whole catalogue with the training positives left out."""
    from ncf_amd import ops, synthetic
    from ncf_amd.metrics import full_rank_metrics
    from ncf_amd.models import NCF
    ds = synthetic.make_dataset("ml-100k", seed=0)
    Un, In = ds["user_num"], ds["item_num"]
    torch.manual_seed(0)
    model = NCF(Un, In, 8, 3, 0.0, "NeuMF-end")
    seen = ops.seen_csr(ds["train_users"], ds["train_items"], Un, "cpu", In)
    users, gt = ds["test_users"][:200], ds["test_items"][:200]
    r = model.target_ranks(users, gt, exclude=seen)
    ranks = r.ranks.numpy()
    assert ranks.shape == (200,) and (ranks < r.eligible.numpy()).all()
    for k in (10, 128):
        hr, nd = full_rank_metrics(model, users, gt, k, exclude=seen)
        assert hr == (ranks < k).astype(int).tolist()
        assert nd == np.where(ranks < k, 1.0 / np.log2(ranks + 2.0), 0.0).tolist()
    assert (ranks >= 128).any()  # positions recommend cannot report
