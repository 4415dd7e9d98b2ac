"""Shared checks of the top-K recommendation tests (CPU and GPU): the CPU oracle's
scores over every (user, item) pair and the tolerance-based verification of a result."""
import numpy as np
import torch

RTOL, ATOL = 1e-5, 1e-7  # the project's logit gate


def oracle_scores(model, chunk=1 << 18):
    """[user_num, item_num] float32 logits of oracle.OracleNCF carrying `model`'s weights."""
    from oracle import ncf_oracle as O
    U, I = model.user_num, model.item_num
    ref = O.OracleNCF(U, I, model.factor_num, model.num_layers, 0.0, model.model_type)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    ref.eval()
    out = torch.empty(U * I, dtype=torch.float32)
    items = torch.arange(I, dtype=torch.int64)
    step = max(1, chunk // I)
    with torch.no_grad():
        for u0 in range(0, U, step):
            us = torch.arange(u0, min(U, u0 + step), dtype=torch.int64)
            out[u0 * I:(u0 + len(us)) * I] = ref(us.repeat_interleave(I), items.repeat(len(us)))
    return out.view(U, I).numpy()


def seen_lists(seen, user_num):
    """SeenCSR -> list of per-user numpy id arrays (None -> empty lists)."""
    if seen is None:
        return [np.zeros(0, dtype=np.int64)] * user_num
    ptr = seen.ptr.cpu().numpy()
    it = seen.items.cpu().numpy().astype(np.int64)
    return [it[ptr[u]:ptr[u + 1]] for u in range(user_num)]


def tol(x, rtol=RTOL, atol=ATOL):
    return atol + rtol * np.abs(x)


def check_topk(items, scores, users, S, k, seen=None, rtol=RTOL, atol=ATOL):
    """Every property of a recommend() result against the oracle scores S [U, I]:
    shapes, fill, validity, no seen item, no duplicate, scores within tolerance, the
    stated order, and that no eligible item left out beats the k-th returned one by more
    than the two tolerances."""
    items = np.asarray(items.cpu() if isinstance(items, torch.Tensor) else items).astype(np.int64)
    scores = np.asarray(scores.cpu() if isinstance(scores, torch.Tensor) else scores)
    users = np.asarray(users).reshape(-1)
    U, I = S.shape
    assert items.shape == scores.shape == (len(users), k)
    lists = seen_lists(seen, U)
    for q, u in enumerate(users):
        excl = lists[u]
        n_ret = min(k, I - len(excl))
        it, sc = items[q], scores[q]
        assert (it[n_ret:] == -1).all() and np.isneginf(sc[n_ret:]).all(), (q, u, "fill")
        it, sc = it[:n_ret], sc[:n_ret]
        if n_ret == 0:
            continue
        assert it.min() >= 0 and it.max() < I, (q, u, "item range")
        assert len(np.unique(it)) == n_ret, (q, u, "duplicate item")
        assert not np.isin(it, excl).any(), (q, u, "seen item returned")
        want = S[u, it]
        err = np.abs(sc - want)
        assert (err <= tol(want, rtol, atol)).all(), (q, u, "score", float(err.max()), want[err.argmax()])
        ordered = (sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (it[:-1] < it[1:]))
        assert ordered.all(), (q, u, "order")
        rest = np.ones(I, dtype=bool)
        rest[it] = False
        rest[excl] = False
        if rest.any():
            left = S[u, rest]
            kth = want[-1]
            assert (left <= kth + tol(kth, rtol, atol) + tol(left, rtol, atol)).all(), (q, u, "better item left out")


def make_seen(user_num, item_num, rng, density=0.05):
    """(users, items) pairs: ~density random pairs; user 3 has none; user 5 has every item
    but three; user 7 has the ids on both sides of every multiple of 16 up to item_num."""
    mask = rng.random((user_num, item_num)) < density
    mask[3] = False
    mask[5] = True
    mask[5, [1, item_num // 2, item_num - 1]] = False
    mask[7] = False
    edges = np.arange(16, item_num, 16)
    mask[7, edges] = True
    mask[7, edges - 1] = True
    mask[7, 0] = True
    mask[7, item_num - 1] = True
    u, i = np.nonzero(mask)
    perm = rng.permutation(len(u))  # unsorted, with some pairs twice: seen_csr sorts and de-duplicates
    u, i = u[perm], i[perm]
    return np.concatenate([u, u[:50]]), np.concatenate([i, i[:50]])
