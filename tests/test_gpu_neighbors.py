"""GPU tests of ncf_neighbors (similar items / users over the embedding tables) against the
float64 reference and the derived per-pair tolerance of tests/neighbors_checks.py: every
space, metric and side, the vector widths (d % 4 != 0, d < 16, d = 576), the edges of the
table and of the query tile, exact ties, a zero row, independence of the launch geometry
bit for bit, the C ABI's refusals, graph capture and the agreement with the CPU path.

The tables are N(0, 1), not the 0.01 initialisation, so norms and ties are not degenerate."""
import copy
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import neighbors_checks as NC  # noqa: E402

DEV = "cuda:0"
U, I = 300, 1007  # 1007: no multiple of 16 or of the 64-row chunk
SPACES = ["gmf", "mlp", "concat"]
METRICS = ["cosine", "dot"]


def _cpu_model(mt, f, nl, users, items, seed=0):
    from ncf_amd.models import NCF
    torch.manual_seed(seed)
    m = NCF(users, items, f, nl, 0.0, mt)
    with torch.no_grad():
        for emb in (m.embed_user_GMF, m.embed_item_GMF, m.embed_user_MLP, m.embed_item_MLP):
            emb.weight.normal_(0.0, 1.0)
    return m.eval()


@functools.lru_cache(maxsize=None)
def _models(mt, f, nl, users, items, seed=0):
    """(CPU model, its copy on the device), built once per shape."""
    mc = _cpu_model(mt, f, nl, users, items, seed)
    return mc, copy.deepcopy(mc).to(DEV)


@functools.lru_cache(maxsize=None)
def _reference(mt, f, nl, users, items, side, space, metric):
    """(S, T) of every row of the side's table queried against every row, computed once."""
    mc, _ = _models(mt, f, nl, users, items)
    table = NC.table64(mc, side, space)
    S, T = NC.reference(table, np.arange(table.shape[0]), metric)
    S.setflags(write=False)
    T.setflags(write=False)
    return S, T


def _fn(m, side):
    return m.similar_items if side == "item" else m.similar_users


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("side", ["item", "user"])
def test_every_space_metric_and_side(side, space, metric):
    shape = ("NeuMF-end", 16, 3, U, I)
    _, m = _models(*shape)
    S, T = _reference(*shape, side, space, metric)
    queries = np.arange(S.shape[0])
    for k in (1, 10, 128):
        ids, scores = _fn(m, side)(torch.as_tensor(queries), k, space=space, metric=metric)
        assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and ids.is_cuda and scores.is_cuda
        NC.check_neighbors(ids, scores, queries, S, T, k, True)
    ids, scores = _fn(m, side)(torch.as_tensor(queries), 10, space=space, metric=metric, exclude_self=False)
    NC.check_neighbors(ids, scores, queries, S, T, 10, False)


@pytest.mark.parametrize("mt,f,nl", [("GMF", 5, 1), ("MLP", 6, 2), ("NeuMF-end", 64, 4)])
def test_vector_widths(mt, f, nl):
    """GMF(5, 1): d = 5 and 10 (d % 4 != 0, d < 16, scalar loads); MLP(6, 2): d = 6, 12, 18;
    NeuMF-end(64, 4): d = 64, 512, 576 (the widest query tile in LDS, 37,120 bytes)."""
    shape = (mt, f, nl, 70, 203)
    _, m = _models(*shape)
    queries = np.arange(203)
    for space in SPACES:
        for metric in METRICS:
            S, T = _reference(*shape, "item", space, metric)
            assert NC.table64(m, "item", space).shape[1] == {"gmf": f, "mlp": f << (nl - 1),
                                                            "concat": f + (f << (nl - 1))}[space]
            for k in (10, 128):
                ids, scores = m.similar_items(queries, k, space=space, metric=metric)
                NC.check_neighbors(ids, scores, queries, S, T, k, True)


def test_default_space_is_the_model_types_own():
    for mt, space in (("GMF", "gmf"), ("MLP", "mlp"), ("NeuMF-end", "concat")):
        _, m = _models(mt, 8, 2, 40, 90)
        got = m.similar_items(np.arange(90), 5)
        want = m.similar_items(np.arange(90), 5, space=space, metric="cosine", exclude_self=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_edges_of_table_and_tile():
    # N = 37: less than one chunk; k = 128 with the query left out: 36 results, then the fill
    shape = ("NeuMF-end", 8, 2, 37, 1)
    _, m = _models(*shape)
    for metric in METRICS:
        S, T = _reference(*shape, "user", "concat", metric)
        q = np.arange(37)
        ids, scores = m.similar_users(q, 128, metric=metric)
        assert (ids[:, :36] >= 0).all() and (ids[:, 36:] == -1).all() and torch.isneginf(scores[:, 36:]).all()
        NC.check_neighbors(ids, scores, q, S, T, 128, True)
        # Q = 1, Q = 17 (a tile and one query), the same id twice
        for q in (np.array([36]), np.arange(17) * 2, np.array([4, 9, 4, 4, 0])):
            for excl in (True, False):
                ids, scores = m.similar_users(q, 10, metric=metric, exclude_self=excl)
                NC.check_neighbors(ids, scores, q, S[q], T[q], 10, excl)
        ids, scores = m.similar_users([4, 9, 4, 4, 0], 10, metric=metric)
        assert torch.equal(ids[0], ids[2]) and torch.equal(ids[0], ids[3])
        assert torch.equal(scores[0], scores[2]) and torch.equal(scores[0], scores[3])
    # N = 1: nothing is eligible
    ids, scores = m.similar_items([0], 5)
    assert (ids == -1).all() and torch.isneginf(scores).all()
    ids, scores = m.similar_items([0, 0], 3, exclude_self=False)
    assert ids.tolist() == [[0, -1, -1]] * 2 and torch.isneginf(scores[:, 1:]).all()
    # the query itself comes first under cosine, at a score within its tolerance of 1
    S, T = _reference(*shape, "user", "concat", "cosine")
    ids, scores = m.similar_users(np.arange(37), 3, exclude_self=False)
    assert ids[:, 0].tolist() == list(range(37))
    assert (np.abs(scores[:, 0].cpu().numpy().astype(np.float64) - 1.0) <= np.diag(T)).all()


def test_exact_ties_come_in_ascending_id_order():
    mc = _cpu_model("NeuMF-end", 8, 3, 100, 20, seed=5)
    group = [5, 40, 41, 77]
    with torch.no_grad():
        for w in (mc.embed_user_GMF.weight, mc.embed_user_MLP.weight):
            w[group[1:]] = w[group[0]].clone()
    m = mc.to(DEV)
    q = np.arange(100)
    for space in SPACES:
        for metric in METRICS:
            ids, scores = m.similar_users(q, 99, space=space, metric=metric)  # every other row
            ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
            for r in range(100):
                pos = np.nonzero(np.isin(ids[r], group))[0]
                members = [g for g in group if g != r]
                assert ids[r, pos].tolist() == members, (space, metric, r)  # contiguous below: ascending ids
                assert (pos == pos[0] + np.arange(len(members))).all(), (space, metric, r)
                assert (scores[r, pos] == scores[r, pos[0]]).all(), (space, metric, r)
        ids, scores = m.similar_users(group, 3, space=space)  # cosine: the copies score highest
        for r, g in enumerate(group):
            assert ids[r].tolist() == [x for x in group if x != g]
            assert (scores[r] == scores[r, 0]).all()


def test_zero_row_scores_zero_and_never_nan():
    mc = _cpu_model("NeuMF-end", 8, 2, 30, 150, seed=6)
    with torch.no_grad():
        mc.embed_item_GMF.weight[9].zero_()
        mc.embed_item_MLP.weight[9].zero_()
    table = NC.table64(mc, "item", "concat")
    m = mc.to(DEV)
    q = np.arange(150)
    S, T = NC.reference(table, q, "cosine")
    assert (S[9] == 0).all() and (T[9] == 0).all() and (S[:, 9] == 0).all()
    for excl in (True, False):
        ids, scores = m.similar_items(q, 128, exclude_self=excl)
        assert not torch.isnan(scores).any()
        NC.check_neighbors(ids, scores, q, S, T, 128, excl)  # tolerance 0 for the zero row's pairs
        assert (scores[ids == 9] == 0).all() and (ids == 9).any()
    ids, scores = m.similar_items([9], 10)
    assert ids[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10] and (scores == 0).all()
    ids, scores = m.similar_items([9], 10, exclude_self=False)
    assert ids[0].tolist() == list(range(10)) and (scores == 0).all()


@pytest.mark.parametrize("metric", METRICS)
def test_result_does_not_depend_on_the_launch_geometry(metric):
    """Bit for bit.  nb_geometry (ncf_neighbors.hip) always gives a workgroup 16 queries and
    splits the ceil(N / 64) chunks over about 1024 / ceil(Q / 16) workgroups.  At N = 203
    (4 chunks): Q = 1 and Q = 203 (13 tiles) run 4 splits of one chunk each and the merge
    of 4 partial lists; Q = 16,400 (1,025 tiles) runs unsplit, one workgroup walking all
    4 chunks.  At N = 1007 (16 chunks) Q = 1007 (63 tiles) runs 16 splits."""
    from ncf_amd import ops
    _, m = _models("NeuMF-end", 16, 3, 70, 203)
    all_i, all_s = ops.neighbors(m, "item", np.arange(203), 10, "concat", metric)
    for r in range(203):
        one_i, one_s = ops.neighbors(m, "item", [r], 10, "concat", metric)
        assert torch.equal(one_i[0], all_i[r]) and torch.equal(one_s[0], all_s[r]), r
    many = np.arange(16400) % 203
    big_i, big_s = ops.neighbors(m, "item", many, 10, "concat", metric)
    assert torch.equal(big_i, all_i[many]) and torch.equal(big_s, all_s[many])
    _, m = _models("NeuMF-end", 16, 3, U, I)
    all_i, all_s = ops.neighbors(m, "item", np.arange(I), 128, "concat", metric)
    some = np.array([0, 15, 16, 63, 64, 500, 1006])
    for r in some:
        one_i, one_s = ops.neighbors(m, "item", [r], 128, "concat", metric)
        assert torch.equal(one_i[0], all_i[r]) and torch.equal(one_s[0], all_s[r]), r
    many = np.arange(16400) % I
    big_i, big_s = ops.neighbors(m, "item", many, 128, "concat", metric)
    assert torch.equal(big_i, all_i[many]) and torch.equal(big_s, all_s[many])


def test_c_abi_refusals():
    import ncf_amd._lib as L
    from ncf_amd import ops
    _, m = _models("NeuMF-end", 16, 3, U, I)
    flat, lay = ops.ensure_flat(m)
    lib = L.hip()
    n, k = 4, 10
    q = torch.zeros(n, dtype=torch.int32, device=DEV)
    out_i = torch.full((n, 128), 7, dtype=torch.int32, device=DEV)
    out_s = torch.full((n, 128), 7.0, dtype=torch.float32, device=DEV)
    need = lib.ncf_neighbors_workspace_bytes(ctypes.byref(lay), L.SIDE_ITEM, L.SPACE_CONCAT, n, k)
    assert need > 0
    ws = torch.zeros(1 << 20, dtype=torch.float32, device=DEV)
    assert need <= ws.numel() * 4
    st = L.stream_ptr(torch.device(DEV))

    def call(side=L.SIDE_ITEM, space=L.SPACE_CONCAT, metric=L.SIM_COSINE, nq=n, top_k=k, ws_bytes=ws.numel() * 4,
             params=flat.data_ptr(), queries=q.data_ptr(), ids=out_i.data_ptr(), scores=out_s.data_ptr(),
             wsp=ws.data_ptr()):
        return lib.ncf_neighbors(ctypes.byref(lay), params, side, space, metric, queries, nq, top_k, 1, ids, scores,
                                 wsp, ws_bytes, st)

    for bad in (dict(side=2), dict(side=-1), dict(space=3), dict(space=-1), dict(metric=2), dict(metric=-1),
                dict(top_k=0), dict(top_k=129), dict(nq=-1), dict(ws_bytes=need - 1), dict(ws_bytes=0),
                dict(params=None), dict(queries=None), dict(ids=None), dict(scores=None), dict(wsp=None)):
        assert call(**bad) == L.NCF_E_ARG, bad
    wsb = lambda side, space, nq, top_k: lib.ncf_neighbors_workspace_bytes(  # noqa: E731
        ctypes.byref(lay), side, space, nq, top_k)
    assert wsb(2, 0, n, k) == -1 and wsb(0, 3, n, k) == -1 and wsb(0, 0, n, 0) == -1 and wsb(0, 0, n, 129) == -1
    assert wsb(0, 0, -1, k) == -1 and wsb(0, 0, 0, k) == 0
    assert lib.ncf_neighbors_workspace_bytes(None, 0, 0, n, k) == -1
    assert call(nq=0) == L.NCF_OK
    torch.cuda.synchronize()
    assert (out_i == 7).all() and (out_s == 7.0).all()  # nothing was launched
    assert call(ws_bytes=need) == L.NCF_OK
    torch.cuda.synchronize()
    want_i, want_s = ops.neighbors(m, "item", q, k)
    assert torch.equal(out_i.view(-1)[:n * k].view(n, k), want_i)
    assert torch.equal(out_s.view(-1)[:n * k].view(n, k), want_s)
    with pytest.raises(ValueError):
        m.similar_items([0], 3, space="tower")
    with pytest.raises(ValueError):
        m.similar_items([0], 3, metric="l2")
    with pytest.raises(ValueError):
        ops.neighbors(m, "movie", [0], 3)
    with pytest.raises(ValueError):
        m.similar_items([0], 129)
    with pytest.raises(IndexError, match="index out of range in self"):
        m.similar_items([I], 3)
    with pytest.raises(IndexError, match="index out of range in self"):
        m.similar_users([U], 3)
    ids, scores = m.similar_items([], 4)
    assert ids.shape == scores.shape == (0, 4) and ids.dtype == torch.int64 and ids.is_cuda


def test_neighbors_captured_in_a_graph():
    import ncf_amd._lib as L
    from ncf_amd import ops
    _, m = _models("NeuMF-end", 16, 3, U, I)
    k = 10
    q = torch.arange(I, dtype=torch.int32, device=DEV)
    eager_i, eager_s = ops.neighbors(m, "item", q, k, "concat", "cosine")
    flat, lay = ops.ensure_flat(m)
    ws = ops.neighbors_workspace(lay, L.SIDE_ITEM, L.SPACE_CONCAT, I, k, m, torch.device(DEV))
    ids = torch.zeros((I, k), dtype=torch.int32, device=DEV)
    scores = torch.zeros((I, k), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # one linear capture
        ops.neighbors_into(flat, lay, L.SIDE_ITEM, L.SPACE_CONCAT, L.SIM_COSINE, q, k, True, ids, scores, ws)
    for _ in range(2):
        ids.zero_()
        scores.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(ids, eager_i) and torch.equal(scores, eager_s)


@pytest.mark.parametrize("metric", METRICS)
def test_cpu_and_hip_backends_agree(metric):
    """The id sets are equal wherever the reference's k-th and (k + 1)-th scores differ by
    more than the two pairs' tolerances; both backends pass the checker."""
    shape = ("NeuMF-end", 16, 3, U, I)
    mc, mg = _models(*shape)
    S, T = _reference(*shape, "item", "concat", metric)
    q = np.arange(I)
    k = 10
    ci, cs = mc.similar_items(q, k, metric=metric)
    gi, gs = mg.similar_items(q, k, metric=metric)
    NC.check_neighbors(ci, cs, q, S, T, k, True)
    NC.check_neighbors(gi, gs, q, S, T, k, True)
    Sx = S.copy()
    Sx[q, q] = -np.inf
    order = np.argsort(-Sx, axis=1, kind="stable")[:, :k + 1]
    rows = q[:, None]
    top, tol = Sx[rows, order], T[rows, order]
    clear = top[:, k - 1] - top[:, k] > tol[:, k - 1] + tol[:, k]
    assert clear.mean() > 0.9
    ci, gi = np.sort(ci.numpy(), axis=1), np.sort(gi.cpu().numpy(), axis=1)
    assert (ci[clear] == gi[clear]).all()
    assert (ci[clear] == np.sort(order[clear, :k], axis=1)).all()
