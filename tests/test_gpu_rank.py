"""Candidate ranking on the device: ncf_rank_candidates (fused and materialised paths) and
NCF.rank, against the CPU oracle with the rules of tests/rank_checks.py, and bit for bit
against ncf_recommend and ncf_select_negatives.

Shapes.  Fused path (ncf_supported == 1, dm <= 64): a 16-lane tile holds 16 candidates of
one list, a workgroup's four waves take tiles w, w + 4, ..., and below 1,024 lists every
list's tiles are split over ceil(1024 / n_lists) workgroups.  List lengths 0, 1, 15, 16,
17 (around one tile), 63, 64, 65 (around one tile per wave), 200 and 1,000 (several tiles
per wave, ids repeated: I = 80).  n_lists = 1 is 64 splits, 17 < 50 users projects the
call's rows with 61 splits, 1,000 >= 50 projects the user table with 2 splits, 1,100 has
one split (the kernel writes the outputs itself); 4,097 lists are more than the 4,096
workgroups of the grid, so workgroups walk more than one list.  Materialised path: a
layered shape and a fused shape forced there, with 144,100 flat candidates: more than one
131,072-pair chunk, the boundary inside a list.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bpr_checks as C
import hardneg_checks as H
import rank_checks as R
import recommend_checks as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ML1M = (6041, 3707)
U, I = 50, 80
FUSED_MODELS = [("NeuMF-end", 8, 3), ("NeuMF-end", 16, 3), ("NeuMF-pre", 8, 3), ("MLP", 16, 2), ("GMF", 16, 1)]
SENT = -7


# --------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def _small(mt, f, Lyr):
    """(oracle scores [U, I] of the model, the model on the device), computed once."""
    ref, m = C.models(mt, f, Lyr, U, I, 11)
    S = H.oracle_scores(ref, np.arange(U), np.tile(np.arange(I), (U, 1)))
    return S, m.to(DEV)


def _pack(lists):
    """(ptr, items) of a sequence of id arrays."""
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    flat = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return ptr, flat.astype(np.int32)


def _split(ptr, items):
    return [items[ptr[q]:ptr[q + 1]] for q in range(len(ptr) - 1)]


def _rank(m, users, ptr, cand, k, n_lists=None, ws_short=0, want_slots=True, null=()):
    """One raw ncf_rank_candidates call: (rc, items, slots, scores, need); the outputs are
    flat NumPy arrays with 8 sentinel entries behind the n_lists * k the call may write."""
    import ncf_amd._lib as L
    from ncf_amd import ops
    flat, lay = ops.ensure_flat(m)
    u = torch.as_tensor(np.ascontiguousarray(users, dtype=np.int32), device=DEV)
    p = torch.as_tensor(np.ascontiguousarray(ptr, dtype=np.int64), device=DEV)
    c = torch.as_tensor(np.ascontiguousarray(cand, dtype=np.int32), device=DEV)
    n = len(users) if n_lists is None else n_lists
    size = max(len(users), 1) * max(k, 1) + 8
    items = torch.full((size,), SENT, dtype=torch.int32, device=DEV)
    slots = torch.full((size,), SENT, dtype=torch.int32, device=DEV)
    scores = torch.full((size,), float("nan"), dtype=torch.float32, device=DEV)
    need = int(L.hip().ncf_rank_candidates_workspace_bytes(ctypes.byref(lay), n, c.numel(), k))
    ws = torch.empty(max(need, 4096) // 4 + 64, dtype=torch.float32, device=DEV)
    args = {"params": flat.data_ptr(), "users": u.data_ptr(), "ptr": p.data_ptr(), "cand": c.data_ptr(),
            "items": items.data_ptr(), "scores": scores.data_ptr(), "ws": ws.data_ptr()}
    for name in null:
        args[name] = None
    rc = L.hip().ncf_rank_candidates(ctypes.byref(lay), args["params"], args["users"], args["ptr"], args["cand"], n,
                                     c.numel(), k, args["items"], slots.data_ptr() if want_slots else None,
                                     args["scores"], args["ws"],
                                     need - ws_short if ws_short else ws.numel() * 4, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, items.cpu().numpy(), slots.cpu().numpy(), scores.cpu().numpy(), need


def _ok(m, users, ptr, cand, k):
    """A call that must succeed and write nothing past n_lists * k: ([n, k] items, slots, scores)."""
    rc, items, slots, scores, _ = _rank(m, users, ptr, cand, k)
    e = len(users) * k
    assert rc == 0
    assert (items[e:] == SENT).all() and (slots[e:] == SENT).all() and np.isnan(scores[e:]).all()  # nothing past n * k
    shape = (len(users), k)
    return items[:e].reshape(shape), slots[:e].reshape(shape), scores[:e].reshape(shape)


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


# --------------------------------------------------------------------------- 1. fused path against the oracle
@pytest.mark.parametrize("mt,f,Lyr", FUSED_MODELS)
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("n", [1, 17, 1000])
def test_fused_vs_oracle(mt, f, Lyr, k, n):
    import ncf_amd._lib as L
    assert L.supported(mt, f, Lyr) == 1
    S, model = _small(mt, f, Lyr)
    # one ragged call over every length; a single list cannot be ragged: one call per length
    calls = [[ln] for ln in R.LENGTHS] if n == 1 else [R.cycle_lengths(n)]
    for lens in calls:
        users, ptr, items = R.ragged(lens, U, I)
        got = _ok(model, users, ptr, items, k)
        R.check_ranked(*got, users, ptr, items, S, k, f"fused {mt}({f},{Lyr}) n={n} k={k} lens={list(lens)[:3]}")


# --------------------------------------------------------------------------- 2. the bits of ncf_recommend
@pytest.mark.parametrize("mt,f,Lyr,path", [("NeuMF-end", 8, 3, 1), ("NeuMF-end", 32, 3, 2)])
@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("exclude", [False, True])
def test_whole_catalogue_is_recommend(mt, f, Lyr, path, k, exclude):
    import ncf_amd._lib as L
    from ncf_amd import ops
    assert L.supported(mt, f, Lyr) == path
    _, model = _small(mt, f, Lyr)
    users = np.arange(U)
    seen = None
    lists = [np.arange(I)] * U
    if exclude:
        su, si = RC.make_seen(U, I, np.random.default_rng(2))
        seen = ops.seen_csr(su, si, U, DEV, I)
        lists = [np.setdiff1d(np.arange(I), x) for x in RC.seen_lists(seen, U)]
    want_i, want_s = model.recommend(torch.from_numpy(users), k=k, exclude=seen)
    ptr, cand = _pack(lists)
    items, slots, scores = _ok(model, users, ptr, cand, k)
    assert np.array_equal(items, want_i.cpu().numpy())
    assert np.array_equal(scores.view(np.uint32), want_s.cpu().numpy().view(np.uint32))
    for q in (0, 5, 7, 49):  # the slot is the position in the user's own list
        ok = slots[q] >= 0
        assert np.array_equal(lists[q][slots[q][ok]], items[q][ok]) and (items[q][~ok] == -1).all()


# --------------------------------------------------------------------------- 3. the bits of ncf_select_negatives
@pytest.mark.parametrize("m", [1, 5, 16, 40])
@pytest.mark.parametrize("n", [17, 1000])
def test_top1_is_hardest_negative(m, n):
    from ncf_amd import ops
    _, model = _small("NeuMF-end", 16, 3)
    users, cand = H.draw(n, m, U, I)
    if m >= 5:
        cand[1, :] = cand[1, 0]  # one id throughout: slot 0
    sel = ops.select_negatives(model, users, cand)
    ptr = np.arange(n + 1, dtype=np.int64) * m
    items, slots, scores = _ok(model, users, ptr, cand.reshape(-1), 1)
    assert np.array_equal(items[:, 0], sel.items.cpu().numpy())
    assert np.array_equal(slots[:, 0], sel.slots.cpu().numpy())
    assert np.array_equal(scores[:, 0].view(np.uint32), sel.scores.cpu().numpy().view(np.uint32))


# --------------------------------------------------------------------------- 4. independence, bit for bit
@pytest.mark.parametrize("k", [10, 128])
def test_independence(k):
    _, model = _small("NeuMF-end", 16, 3)
    users, ptr, items = R.ragged(R.cycle_lengths(300), U, I, seed=7)
    lists = _split(ptr, items)
    rng = np.random.default_rng(1)
    probe_u, probe = 13, rng.integers(0, I, 333).astype(np.int32)
    alone = _ok(model, [probe_u], *_pack([probe]), k)                       # 64 splits
    for pos in (0, 150, 299):                                              # 4 splits
        us, ls = users.copy(), list(lists)
        us[pos], ls[pos] = probe_u, probe
        got = _ok(model, us, *_pack(ls), k)
        assert _same([x[pos:pos + 1] for x in got], alone), pos
    twice = _ok(model, [probe_u, 3, probe_u], *_pack([probe, lists[0], probe]), k)
    assert _same([x[0:1] for x in twice], alone) and _same([x[2:3] for x in twice], alone)
    base = _ok(model, users, ptr, items, k)
    rev = _ok(model, users[::-1], *_pack(lists[::-1]), k)
    assert _same([x[::-1] for x in rev], base)
    # the split over grid.y: 17 lists alone (61 splits) and as the head of 1,100 lists (one split)
    big_u = np.concatenate([users, users, users, users[:200]])
    big = _ok(model, big_u, *_pack((lists * 4)[:1100]), k)
    head = _ok(model, users[:17], *_pack(lists[:17]), k)
    assert _same([x[:17] for x in big], head)
    assert _same([x[:300] for x in big], base) and _same([x[300:600] for x in big], base)


@pytest.mark.parametrize("length", [80, 200])
def test_permuted_candidates(length):
    _, model = _small("NeuMF-end", 16, 3)
    rng = np.random.default_rng(4)
    lst = (rng.permutation(I) if length <= I else rng.integers(0, I, length)).astype(np.int32)
    perm = rng.permutation(length)
    k = 10
    a = _ok(model, [21], *_pack([lst]), k)
    b = _ok(model, [21], *_pack([lst[perm]]), k)
    key = lambda r: sorted(zip(r[0][0].tolist(), r[2][0].view(np.uint32).tolist()))  # noqa: E731
    assert key(a) == key(b)
    assert np.array_equal(lst[perm[b[1][0]]], b[0][0])  # the slots map back through the permutation
    assert np.array_equal(lst[a[1][0]], a[0][0])


# --------------------------------------------------------------------------- 5. duplicates
def test_duplicates():
    _, model = _small("NeuMF-end", 8, 3)
    items, slots, scores = _ok(model, [4], *_pack([np.full(40, 9)]), 10)
    assert slots[0].tolist() == list(range(10)) and (items == 9).all()
    assert len(set(scores[0].view(np.uint32).tolist())) == 1
    lst = np.array([5, 9] * 20)  # 40 candidates, three tiles: the copies alternate
    items, slots, scores = _ok(model, [4], *_pack([lst]), 40)
    assert sorted(slots[0].tolist()) == list(range(40))
    first = items[0, 0]
    assert (items[0, :20] == first).all() and (items[0, 20:] == (14 - first)).all()
    assert (np.diff(slots[0, :20]) > 0).all() and (np.diff(slots[0, 20:]) > 0).all()


# --------------------------------------------------------------------------- 6. workgroups walk more than one list
def test_fused_ml1m_workgroups_walk_lists():
    import ncf_amd._lib as L
    assert L.supported("NeuMF-end", 16, 3) == 1
    ref, model = C.models("NeuMF-end", 16, 3, *ML1M, 11)
    users, cand = H.draw(4097, 24, *ML1M)
    ptr = np.arange(4098, dtype=np.int64) * 24
    items, slots, scores = _ok(model.to(DEV), users, ptr, cand.reshape(-1), 10)
    sample = np.unique(np.concatenate([[0, 1, 4095, 4096], np.random.default_rng(0).integers(0, 4097, 300)]))
    S = H.oracle_scores(ref, users[sample], cand[sample]).reshape(-1)
    R.check_ranked(items[sample], slots[sample], scores[sample], users[sample], np.arange(len(sample) + 1) * 24,
                   cand[sample].reshape(-1), S, 10, "fused ml-1m 4097 x 24")


# --------------------------------------------------------------------------- 7. materialised path
@pytest.mark.parametrize("k", [10, 128])
def test_materialised_layered_shape(k):
    import ncf_amd._lib as L
    assert L.supported("NeuMF-end", 32, 3) == 2
    S, model = _small("NeuMF-end", 32, 3)
    users, ptr, items = R.ragged(R.cycle_lengths(1000), U, I)
    assert ptr[-1] > (1 << 17) and (1 << 17) not in ptr  # two chunks, the boundary inside a list
    R.check_ranked(*_ok(model, users, ptr, items, k), users, ptr, items, S, k, f"materialised NeuMF-end(32,3) k={k}")


def test_materialised_forced_agrees_with_fused():
    from ncf_amd import ops
    S, model = _small("NeuMF-end", 8, 3)
    users, ptr, items = R.ragged(R.cycle_lengths(1000), U, I)
    fused = _ok(model, users, ptr, items, 10)
    with ops._rank_materialised():  # restores the path in its finally
        mat = _ok(model, users, ptr, items, 10)
        few = _ok(model, users[:3], ptr[:4], items[:ptr[3]], 10)
    again = _ok(model, users, ptr, items, 10)
    R.check_ranked(*mat, users, ptr, items, S, 10, "materialised (forced) NeuMF-end(8,3)")
    R.check_ranked(*few, users[:3], ptr[:4], items[:ptr[3]], S, 10, "materialised (forced), 3 lists")
    assert _same(fused, again)  # the fused path is back
    np.testing.assert_allclose(mat[2], fused[2], rtol=2e-5, atol=2e-7)  # both within the gate of the oracle


# --------------------------------------------------------------------------- 8. arguments
@pytest.mark.parametrize("forced", [False, True])
def test_arguments(forced):
    import contextlib
    import ncf_amd._lib as L
    from ncf_amd import ops
    S, model = _small("NeuMF-end", 8, 3)
    users, ptr, items = R.ragged(R.cycle_lengths(20), U, I)
    with (ops._rank_materialised() if forced else contextlib.nullcontext()):
        assert _rank(model, users, ptr, items, 0)[0] == L.NCF_E_ARG
        assert _rank(model, users, ptr, items, 129)[0] == L.NCF_E_ARG
        rc, _, _, _, need = _rank(model, users, ptr, items, 10, ws_short=1)
        assert rc == L.NCF_E_ARG and need > 0
        for name in ("params", "users", "ptr", "cand", "items", "scores", "ws"):
            rc, it, sl, sc, _ = _rank(model, users, ptr, items, 10, null=(name,))
            assert rc == L.NCF_E_ARG and (it == SENT).all() and (sl == SENT).all() and np.isnan(sc).all(), name
        assert _rank(model, users, ptr, items, 10, n_lists=-1)[0] == L.NCF_E_ARG
        rc, it, sl, sc, _ = _rank(model, users, ptr, items, 10, n_lists=0)
        assert rc == L.NCF_OK and (it == SENT).all() and (sl == SENT).all() and np.isnan(sc).all()
        # slots_out left out; a prefix of the lists: nothing written past n_lists * k
        rc, it, sl, sc, _ = _rank(model, users[:7], ptr[:8], items[:ptr[7]], 10, want_slots=False)
        assert rc == L.NCF_OK and (sl == SENT).all()
        assert (it[70:] == SENT).all() and np.isnan(sc[70:]).all() and not np.isnan(sc[:70]).any()
        full = _ok(model, users, ptr, items, 10)
        assert np.array_equal(it[:70].reshape(7, 10), full[0][:7])
        assert np.array_equal(sc[:70].reshape(7, 10).view(np.uint32), full[2][:7].view(np.uint32))
        # only empty lists, and no candidates at all
        none = _ok(model, users[:4], np.zeros(5, dtype=np.int64), np.zeros(0, dtype=np.int32), 3)
        assert (none[0] == -1).all() and (none[1] == -1).all() and np.isneginf(none[2]).all()
    assert L.hip().ncf_debug_set_rank_path(5) == L.NCF_E_ARG
    lay = ops.ensure_flat(model)[1]
    wsb = L.hip().ncf_rank_candidates_workspace_bytes
    assert wsb(ctypes.byref(lay), 10, 100, 0) == -1 and wsb(ctypes.byref(lay), 10, 100, 129) == -1
    assert wsb(ctypes.byref(lay), -1, 100, 4) == -1 and wsb(ctypes.byref(lay), 10, -1, 4) == -1
    assert wsb(None, 10, 100, 4) == -1 and wsb(ctypes.byref(lay), 0, 0, 4) == 0


def test_model_surface_on_device():
    from ncf_amd import ops
    S, model = _small("NeuMF-end", 8, 3)
    users, ptr, items = R.ragged(R.cycle_lengths(30), U, I)
    cl = ops.CandidateLists(torch.from_numpy(ptr), torch.from_numpy(items))
    r = model.rank(torch.as_tensor(users), cl, k=10)
    assert isinstance(r, ops.Ranked) and r.items.is_cuda and r.items.shape == (30, 10)
    assert r.items.dtype == torch.int64 and r.slots.dtype == torch.int64 and r.scores.dtype == torch.float32
    R.check_ranked(r.items, r.slots, r.scores, users, ptr, items, S, 10, "NCF.rank")
    shared = np.arange(0, I, 3)
    a = model.rank(users, shared, k=5)                                     # 1-D shared list
    b = model.rank(users, torch.as_tensor(np.tile(shared, (30, 1)), device=DEV), k=5)  # 2-D, on the device
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    R.check_ranked(a.items, a.slots, a.scores, users, np.arange(31) * len(shared), np.tile(shared, 30), S, 5, "shared")
    bad = items.copy()
    bad[5] = I
    with pytest.raises(IndexError):
        model.rank(users, ops.CandidateLists(torch.from_numpy(ptr), torch.from_numpy(bad)))
    with pytest.raises(IndexError):
        model.rank(np.full(30, U), cl)
    with pytest.raises(ValueError):
        model.rank(users[:29], cl)
    with pytest.raises(ValueError):
        model.rank(users, cl, k=129)
    assert model.rank(users[:0], np.zeros((0, 4), dtype=np.int64), k=3).items.shape == (0, 3)


# --------------------------------------------------------------------------- 9. graph capture
@pytest.mark.parametrize("n,forced", [(17, False), (1100, False), (17, True)])
def test_graph_capture(n, forced):
    """Captured and replayed, the call gives the eager result bit for bit (61 splits with the
    merge pass, one split, and the materialised path); one linear capture, no parallel branches."""
    import contextlib
    from ncf_amd import ops
    _, model = _small("NeuMF-end", 8, 3)
    flat, lay = ops.ensure_flat(model)
    users, ptr, items = R.ragged(R.cycle_lengths(n), U, I)
    u = torch.as_tensor(users, device=DEV)
    p = torch.as_tensor(ptr, device=DEV)
    c = torch.as_tensor(items, device=DEV)
    k = 10

    def fresh():
        return (torch.full((n, k), SENT, dtype=torch.int32, device=DEV),
                torch.full((n, k), SENT, dtype=torch.int32, device=DEV),
                torch.full((n, k), float("nan"), dtype=torch.float32, device=DEV))
    with (ops._rank_materialised() if forced else contextlib.nullcontext()):
        ws = ops.rank_workspace(lay, n, c.numel(), k, ops._Scratch(), DEV)
        eager = fresh()
        for _ in range(2):
            ops.rank_into(flat, lay, u, p, c, k, *eager, ws)
        torch.cuda.synchronize()
        cap = fresh()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):  # one linear capture
            ops.rank_into(flat, lay, u, p, c, k, *cap, ws)
        for dst, src in zip(cap, fresh()):
            dst.copy_(src)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
    for a, b in zip(cap, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert (cap[1][:, 0] >= -1).all() and not torch.isnan(cap[2]).any()
