"""Target ranks on the device: ncf_target_ranks (fused and materialised paths),
NCF.target_ranks and Trainer.evaluate_ranks -- against the CPU oracle with the band of
tests/target_checks.py, and exactly (bit for bit) against ncf_recommend and ncf_rank_candidates.

Shapes.  U = 50, I = 80 is two 64-item chunks, the second of one 16-item tile.  Fused path
(dm <= 64): a list is cut into units of at most tb targets, tb the power of two in [16, 128]
that covers the mean list length; a workgroup sweeps the catalogue for 4 units (fewer than 256
units) or 16.  List lengths 0, 1, 15, 16, 17, 63, 64, 65, 200 and 1,000: empty lists, units of
at most 4 targets (counted by ballot), longer units (binary search and LDS histogram), lists of
several units, repeated ids (I = 80).  n_lists = 1 is one list split over the two chunks, 17 < 50
users projects the call's rows, 1,000 >= 50 projects the user table with 16-unit tiles.
Materialised path: a layered shape with 1,700 lists (more than one 131,072-pair chunk of 1,638
lists) and a fused shape forced there.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import bpr_checks as C
import rank_checks as R
import recommend_checks as RC
import target_checks as T
from test_gpu_rank import FUSED_MODELS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ML1M = (6041, 3707)
U, I = 50, 80
SENT = -7


# --------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def _small(mt, f, Lyr):
    """(oracle scores [U, I] of the model, the model on the device), computed once."""
    _, m = C.models(mt, f, Lyr, U, I, 11)
    return RC.oracle_scores(m), m.to(DEV)


@functools.lru_cache(maxsize=None)
def _seen():
    from ncf_amd import ops
    su, si = RC.make_seen(U, I, np.random.default_rng(2))
    return ops.seen_csr(su, si, U, DEV, I)


def _pack(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    flat = np.concatenate([np.asarray(x, dtype=np.int32) for x in lists]) if len(lists) else np.zeros(0, np.int32)
    return ptr, flat.astype(np.int32)


def _split(ptr, items):
    return [items[ptr[q]:ptr[q + 1]] for q in range(len(ptr) - 1)]


def _call(m, users, ptr, tgt, seen=None, n_lists=None, ws_short=0, want_scores=True, null=(), out=None):
    """One raw ncf_target_ranks call: (rc, ranks, scores, need); the outputs are flat NumPy arrays
    with 8 sentinel entries behind the n_tgt the call may write.  `out`: (ranks, scores) device
    tensors to write into instead of fresh ones."""
    import ncf_amd._lib as L
    from ncf_amd import ops
    flat, lay = ops.ensure_flat(m)
    u = torch.as_tensor(np.ascontiguousarray(users, dtype=np.int32), device=DEV)
    p = torch.as_tensor(np.ascontiguousarray(ptr, dtype=np.int64), device=DEV)
    t = torch.as_tensor(np.ascontiguousarray(tgt, dtype=np.int32), device=DEV)
    n = len(users) if n_lists is None else n_lists
    if out is None:
        out = (torch.full((t.numel() + 8,), SENT, dtype=torch.int32, device=DEV),
               torch.full((t.numel() + 8,), float("nan"), dtype=torch.float32, device=DEV))
    ranks, scores = out
    need = int(L.hip().ncf_target_ranks_workspace_bytes(ctypes.byref(lay), n, t.numel()))
    ws = torch.empty(max(need, 4096) // 4 + 64, dtype=torch.float32, device=DEV)
    args = {"params": flat.data_ptr(), "users": u.data_ptr(), "ptr": p.data_ptr(), "targets": t.data_ptr(),
            "ranks": ranks.data_ptr(), "ws": ws.data_ptr()}
    for name in null:
        args[name] = None
    rc = L.hip().ncf_target_ranks(ctypes.byref(lay), args["params"], args["users"], args["ptr"], args["targets"], n,
                                  t.numel(), None if seen is None else seen.ptr.data_ptr(),
                                  None if seen is None or "seen_items" in null else seen.items.data_ptr(),
                                  args["ranks"], scores.data_ptr() if want_scores else None, args["ws"],
                                  need - ws_short if ws_short else ws.numel() * 4, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, ranks.cpu().numpy(), scores.cpu().numpy(), need


def _ok(m, users, ptr, tgt, seen=None):
    """A call that must succeed and write nothing past n_tgt: (ranks [E], scores [E])."""
    rc, ranks, scores, _ = _call(m, users, ptr, tgt, seen)
    e = len(tgt)
    assert rc == 0
    assert (ranks[e:] == SENT).all() and np.isnan(scores[e:]).all()  # nothing past n_tgt
    assert (ranks[:e] >= 0).all() and not np.isnan(scores[:e]).any()
    return ranks[:e], scores[:e]


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _device_scores(model, users):
    """[len(users), I] device scores of the users' whole rows: NCF.rank over the full item list
    with k = I <= 128 -- the pair score of ncf_recommend and ncf_target_ranks, bit for bit."""
    n_items = model.item_num
    assert n_items <= 128
    r = model.rank(torch.as_tensor(np.asarray(users)), np.arange(n_items), k=n_items)
    Z = np.empty((len(users), n_items), dtype=np.float32)
    np.put_along_axis(Z, r.items.cpu().numpy(), r.scores.cpu().numpy(), axis=1)
    return Z


# --------------------------------------------------------------------------- 1. fused path against the oracle band
@pytest.mark.parametrize("mt,f,Lyr", FUSED_MODELS)
@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("n", [1, 17, 1000])
def test_fused_vs_oracle_band(mt, f, Lyr, exclude, n):
    import ncf_amd._lib as L
    assert L.supported(mt, f, Lyr) == 1
    S, model = _small(mt, f, Lyr)
    seen = _seen() if exclude else None
    # one ragged call over every length; a single list cannot be ragged: one call per length
    calls = [[ln] for ln in R.LENGTHS] if n == 1 else [R.cycle_lengths(n)]
    for lens in calls:
        users, ptr, tgt = R.ragged(lens, U, I)
        if exclude and n > 1:
            users[:3] = (3, 5, 7)  # nothing seen; all but three seen; the tile edges seen
        ranks, scores = _ok(model, users, ptr, tgt, seen)
        what = f"fused {mt}({f},{Lyr}) n={n} exclude={exclude} lens={list(lens)[:3]}"
        T.check_ranks_band(ranks, users, ptr, tgt, S, seen, what)
        T.check_scores(scores, users, ptr, tgt, S, what)


# --------------------------------------------------------------------------- 2. exact: the order of ncf_recommend
@pytest.mark.parametrize("mt,f,Lyr", FUSED_MODELS)
@pytest.mark.parametrize("exclude", [False, True])
def test_rank_is_position_in_recommend(mt, f, Lyr, exclude):
    """I = 80 <= 128: recommend(u, 80, seen) is the whole eligible order in device scores."""
    _, model = _small(mt, f, Lyr)
    seen = _seen() if exclude else None
    users = np.arange(U)
    items, sc = model.recommend(torch.from_numpy(users), k=I, exclude=seen)
    items, sc = items.cpu().numpy(), sc.cpu().numpy()
    tgt = np.tile(np.arange(I, dtype=np.int32), U)  # every item of every user: 80 targets per list
    ptr = np.arange(U + 1, dtype=np.int64) * I
    ranks, scores = _ok(model, users, ptr, tgt, seen)
    ranks, scores = ranks.reshape(U, I), scores.reshape(U, I)
    Z = _device_scores(model, users)
    assert np.array_equal(scores.view(np.uint32), Z.view(np.uint32))  # the bits of ncf_rank_candidates
    want = T.exact_ranks(Z, users, ptr, tgt, seen).reshape(U, I)
    lists = RC.seen_lists(seen, U)
    for u in users:
        elig = np.setdiff1d(np.arange(I), lists[u])
        assert np.array_equal(items[u][ranks[u, elig]], elig), u         # items[rank] == t
        assert np.array_equal(sc[u][ranks[u, elig]].view(np.uint32), scores[u, elig].view(np.uint32)), u
        assert np.array_equal(ranks[u, lists[u]], want[u, lists[u]]), u   # seen targets: ranked as if eligible
    assert np.array_equal(ranks, want)


# --------------------------------------------------------------------------- 3. ml-1m shape
def test_fused_ml1m_exact():
    import ncf_amd._lib as L
    from ncf_amd import ops
    assert L.supported("NeuMF-end", 16, 3) == 1
    Un, In = ML1M
    _, model = C.models("NeuMF-end", 16, 3, Un, In, 11)
    model = model.to(DEV)
    rng = np.random.default_rng(5)
    n = 4097
    users = rng.integers(0, Un, n).astype(np.int32)
    tgt = rng.integers(0, In, n).astype(np.int32)
    ptr = np.arange(n + 1, dtype=np.int64)
    seen = ops.seen_csr(rng.integers(0, Un, 300_000), rng.integers(0, In, 300_000), Un, DEV, In)
    ranks, scores = _ok(model, users, ptr, tgt, seen)
    sample = np.unique(np.concatenate([[0, 1, 4095, 4096], rng.integers(0, n, 296)]))
    su = users[sample]
    # every device score of the sampled users: NCF.rank over 128-item slices with k = 128
    cuts = list(range(0, In, 128)) + [In]
    slices = [np.arange(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    sp, sflat = _pack(slices * len(su))
    r = model.rank(np.repeat(su, len(slices)), ops.CandidateLists(torch.from_numpy(sp), torch.from_numpy(sflat)), k=128)
    ri, rs = r.items.cpu().numpy().reshape(len(su), -1), r.scores.cpu().numpy().reshape(len(su), -1)
    Z = np.zeros((Un, In), dtype=np.float32)
    for q, u in enumerate(su):
        ok = ri[q] >= 0
        assert ok.sum() == In
        Z[u, ri[q][ok]] = rs[q][ok]
    want = T.exact_ranks(Z, su, np.arange(len(su) + 1), tgt[sample], seen)
    assert np.array_equal(ranks[sample], want)
    assert np.array_equal(scores[sample].view(np.uint32), Z[su, tgt[sample]].view(np.uint32))
    top_i, top_s = model.recommend(torch.as_tensor(su.astype(np.int64)), k=128, exclude=seen)
    top_i = top_i.cpu().numpy()
    lists = RC.seen_lists(seen, Un)
    near = 0
    for q, e in enumerate(sample):
        if ranks[e] < 128 and tgt[e] not in lists[su[q]]:
            assert top_i[q, ranks[e]] == tgt[e], (q, e)
            near += 1
    assert near > 0 and (ranks[sample] >= 128).any()  # both sides of recommend's limit


# --------------------------------------------------------------------------- 4. independence, bit for bit
@pytest.mark.parametrize("exclude", [False, True])
def test_independence(exclude):
    _, model = _small("NeuMF-end", 16, 3)
    seen = _seen() if exclude else None
    users, ptr, tgt = R.ragged(R.cycle_lengths(300), U, I, seed=7)
    lists = _split(ptr, tgt)
    rng = np.random.default_rng(1)
    probe_u, probe = 13, rng.integers(0, I, 333).astype(np.int32)
    alone = _ok(model, [probe_u], *_pack([probe]), seen)
    for pos in (0, 150, 299):
        us, ls = users.copy(), list(lists)
        us[pos], ls[pos] = probe_u, probe
        p2, t2 = _pack(ls)
        got = _ok(model, us, p2, t2, seen)
        assert _same([x[p2[pos]:p2[pos + 1]] for x in got], alone), pos
    p3, t3 = _pack([probe, lists[0], probe])
    twice = _ok(model, [probe_u, 3, probe_u], p3, t3, seen)
    assert _same([x[:333] for x in twice], alone) and _same([x[p3[2]:] for x in twice], alone)
    base = _ok(model, users, ptr, tgt, seen)
    rp, rt = _pack(lists[::-1])
    rev = _ok(model, users[::-1], rp, rt, seen)
    for q in (0, 1, 150, 298, 299):
        a = [x[rp[299 - q]:rp[300 - q]] for x in rev]
        assert _same(a, [x[ptr[q]:ptr[q + 1]] for x in base]), q
    assert sorted(rev[0].tolist()) == sorted(base[0].tolist())
    # the split of the catalogue: 17 lists alone (4-unit tiles, one chunk per split) and as the
    # head of 1,100 lists (16-unit tiles, one split)
    big_u = np.concatenate([users, users, users, users[:200]])
    bp, bt = _pack((lists * 4)[:1100])
    big = _ok(model, big_u, bp, bt, seen)
    head = _ok(model, users[:17], *_pack(lists[:17]), seen)
    assert _same([x[:bp[17]] for x in big], head)
    assert _same([x[:bp[300]] for x in big], base) and _same([x[bp[300]:bp[600]] for x in big], base)


@pytest.mark.parametrize("length", [3, 80, 200])
def test_permuted_targets(length):
    _, model = _small("NeuMF-end", 16, 3)
    rng = np.random.default_rng(4)
    lst = (rng.permutation(I)[:length] if length <= I else rng.integers(0, I, length)).astype(np.int32)
    perm = rng.permutation(length)
    a = _ok(model, [21], *_pack([lst]), _seen())
    b = _ok(model, [21], *_pack([lst[perm]]), _seen())
    assert _same([x[perm] for x in a], b)
    if length > I:  # duplicates get equal ranks
        for t in np.unique(lst):
            assert len(set(a[0][lst == t].tolist())) == 1


# --------------------------------------------------------------------------- 5. materialised path
MAT_LENGTHS = [0, 1, 2, 5, 17, 65]


def test_materialised_layered_shape():
    import ncf_amd._lib as L
    from ncf_amd import ops
    assert L.supported("NeuMF-end", 32, 3) == 2
    S, model = _small("NeuMF-end", 32, 3)
    n = 1700
    assert n * I > (1 << 17)  # more than one chunk of 1,638 lists
    users, ptr, tgt = R.ragged(R.cycle_lengths(n, MAT_LENGTHS), U, I)
    users[:3] = (3, 5, 7)
    seen = _seen()
    ranks, scores = _ok(model, users, ptr, tgt, seen)
    T.check_ranks_band(ranks, users, ptr, tgt, S, seen, "materialised NeuMF-end(32,3)")
    T.check_scores(scores, users, ptr, tgt, S, "materialised NeuMF-end(32,3)")
    flat, lay = ops.ensure_flat(model)
    uu = torch.arange(U, dtype=torch.int32, device=DEV).repeat_interleave(I)
    ii = torch.arange(I, dtype=torch.int32, device=DEV).repeat(U)
    Z = ops.forward_logits(flat, lay, ops.pack_rows(uu, ii)).cpu().numpy().reshape(U, I)
    assert np.array_equal(ranks, T.exact_ranks(Z, users, ptr, tgt, seen))


def test_materialised_forced():
    from ncf_amd import ops
    S, model = _small("NeuMF-end", 8, 3)
    seen = _seen()
    users, ptr, tgt = R.ragged(R.cycle_lengths(1000), U, I)
    users[:3] = (3, 5, 7)
    fused = _ok(model, users, ptr, tgt, seen)
    with ops._target_materialised():  # restores the path in its finally
        mat = _ok(model, users, ptr, tgt, seen)
        few = _ok(model, users[:3], ptr[:4], tgt[:ptr[3]], None)
    again = _ok(model, users, ptr, tgt, seen)
    T.check_ranks_band(mat[0], users, ptr, tgt, S, seen, "materialised (forced) NeuMF-end(8,3)")
    T.check_scores(mat[1], users, ptr, tgt, S, "materialised (forced)")
    T.check_ranks_band(few[0], users[:3], ptr[:4], tgt[:ptr[3]], S, None, "materialised (forced), 3 lists")
    flat, lay = ops.ensure_flat(model)
    uu = torch.arange(U, dtype=torch.int32, device=DEV).repeat_interleave(I)
    ii = torch.arange(I, dtype=torch.int32, device=DEV).repeat(U)
    Z = ops.forward_logits(flat, lay, ops.pack_rows(uu, ii)).cpu().numpy().reshape(U, I)
    assert np.array_equal(mat[0], T.exact_ranks(Z, users, ptr, tgt, seen))
    assert _same(fused, again)  # the fused path is back


# --------------------------------------------------------------------------- 6. arguments
@pytest.mark.parametrize("forced", [False, True])
def test_arguments(forced):
    import ncf_amd._lib as L
    from ncf_amd import ops
    S, model = _small("NeuMF-end", 8, 3)
    seen = _seen()
    users, ptr, tgt = R.ragged(R.cycle_lengths(20), U, I)
    e = len(tgt)
    with (ops._target_materialised() if forced else contextlib.nullcontext()):
        rc, _, _, need = _call(model, users, ptr, tgt, seen, ws_short=1)
        assert rc == L.NCF_E_ARG and need > 0
        for name in ("params", "users", "ptr", "targets", "ranks", "ws"):
            rc, rk, sc, _ = _call(model, users, ptr, tgt, seen, null=(name,))
            assert rc == L.NCF_E_ARG and (rk == SENT).all() and np.isnan(sc).all(), name
        assert _call(model, users, ptr, tgt, seen, n_lists=-1)[0] == L.NCF_E_ARG
        rc, rk, sc, _ = _call(model, users, ptr, tgt, seen, n_lists=0)
        assert rc == L.NCF_OK and (rk == SENT).all() and np.isnan(sc).all()
        rc, rk, sc, _ = _call(model, users, ptr, tgt, seen, null=("seen_items",))  # seen_ptr without seen_items
        assert rc == L.NCF_E_ARG and (rk == SENT).all() and np.isnan(sc).all()
        full = _ok(model, users, ptr, tgt, seen)
        T.check_ranks_band(full[0], users, ptr, tgt, S, seen, f"arguments forced={forced}")
        # scores_out left out; a prefix of the lists: nothing written past its targets
        e7 = int(ptr[7])
        rc, rk, sc, _ = _call(model, users[:7], ptr[:8], tgt[:e7], seen, want_scores=False)
        assert rc == L.NCF_OK and np.isnan(sc).all()
        assert np.array_equal(rk[:e7], full[0][:e7]) and (rk[e7:] == SENT).all()
        # seen NULL
        free = _ok(model, users, ptr, tgt, None)
        T.check_ranks_band(free[0], users, ptr, tgt, S, None, f"no seen, forced={forced}")
        assert np.array_equal(free[1].view(np.uint32), full[1].view(np.uint32))
        # twice into the same outputs, and after another call's result: nothing stale adds up
        out = (torch.full((e + 8,), 1000, dtype=torch.int32, device=DEV),
               torch.full((e + 8,), 3.0, dtype=torch.float32, device=DEV))
        for _ in range(2):
            rc, rk, sc, _ = _call(model, users, ptr, tgt, seen, out=out)
            assert rc == L.NCF_OK and _same((rk[:e], sc[:e]), full) and (rk[e:] == 1000).all() and (sc[e:] == 3.0).all()
        # only empty lists, and no targets at all
        rc, rk, sc, _ = _call(model, users[:4], np.zeros(5, dtype=np.int64), np.zeros(0, dtype=np.int32), seen)
        assert rc == L.NCF_OK and (rk == SENT).all() and np.isnan(sc).all()
    assert L.hip().ncf_debug_set_target_path(5) == L.NCF_E_ARG
    lay = ops.ensure_flat(model)[1]
    wsb = L.hip().ncf_target_ranks_workspace_bytes
    assert wsb(ctypes.byref(lay), -1, 100) == -1 and wsb(ctypes.byref(lay), 10, -1) == -1
    assert wsb(None, 10, 100) == -1 and wsb(ctypes.byref(lay), 0, 0) == 0 and wsb(ctypes.byref(lay), 10, 100) > 0


# --------------------------------------------------------------------------- 7. graph capture
@pytest.mark.parametrize("n,forced", [(17, False), (1100, False), (17, True)])
def test_graph_capture(n, forced):
    """Captured and replayed twice, the call gives the eager result bit for bit (several splits,
    one split, the materialised path): the pre-pass zeroes the counts on every replay.  One
    linear capture, no parallel branches."""
    from ncf_amd import ops
    _, model = _small("NeuMF-end", 8, 3)
    flat, lay = ops.ensure_flat(model)
    seen = _seen()
    users, ptr, tgt = R.ragged(R.cycle_lengths(n), U, I)
    u = torch.as_tensor(users, device=DEV)
    p = torch.as_tensor(ptr, device=DEV)
    t = torch.as_tensor(tgt, device=DEV)
    e = t.numel()

    def fresh():
        return (torch.full((e,), SENT, dtype=torch.int32, device=DEV),
                torch.full((e,), float("nan"), dtype=torch.float32, device=DEV))
    with (ops._target_materialised() if forced else contextlib.nullcontext()):
        ws = ops.target_ranks_workspace(lay, n, e, ops._Scratch(), DEV)
        eager = fresh()
        for _ in range(2):
            ops.target_ranks_into(flat, lay, u, p, t, seen, *eager, ws)
        torch.cuda.synchronize()
        cap = fresh()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):  # one linear capture
            ops.target_ranks_into(flat, lay, u, p, t, seen, *cap, ws)
        for dst, src in zip(cap, fresh()):
            dst.copy_(src)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
    for a, b in zip(cap, eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert (cap[0] >= 0).all() and not torch.isnan(cap[1]).any()
    assert np.array_equal(cap[0].cpu().numpy(), _ok(model, users, ptr, tgt, seen)[0])


# --------------------------------------------------------------------------- 8. model surface
def test_model_surface_on_device():
    from ncf_amd import ops
    S, model = _small("NeuMF-end", 8, 3)
    su, si = RC.make_seen(U, I, np.random.default_rng(2))
    seen = _seen()
    users, ptr, tgt = R.ragged(R.cycle_lengths(30), U, I)
    cl = ops.CandidateLists(torch.from_numpy(ptr), torch.from_numpy(tgt))
    r = model.target_ranks(torch.as_tensor(users), cl, exclude=(su, si))
    assert isinstance(r, ops.TargetRanks) and all(x.is_cuda for x in r)
    assert r.ranks.dtype == torch.int64 and r.scores.dtype == torch.float32
    assert r.ptr.dtype == torch.int64 and r.eligible.dtype == torch.int64
    assert r.ranks.shape == r.scores.shape == (len(tgt),) and r.ptr.shape == (31,) and r.eligible.shape == (30,)
    T.check_ranks_band(r.ranks, users, ptr, tgt, S, seen, "NCF.target_ranks")
    lens = np.array([len(x) for x in RC.seen_lists(seen, U)])
    assert np.array_equal(r.eligible.cpu().numpy(), I - lens[users])
    assert np.array_equal(r.ptr.cpu().numpy(), ptr)
    rag = model.target_ranks(users, _split(ptr, tgt), exclude=seen)  # ragged Python lists
    assert all(torch.equal(a, b) for a, b in zip(rag, r))
    one = model.target_ranks(users, tgt[:30])                              # 1-D: one target per user
    two = model.target_ranks(users, torch.as_tensor(tgt[:30].reshape(30, 1), device=DEV))  # 2-D, on the device
    assert one.ranks.shape == one.scores.shape == (30,) and two.ranks.shape == two.scores.shape == (30, 1)
    assert torch.equal(one.ranks, two.ranks[:, 0]) and torch.equal(one.scores, two.scores[:, 0])
    assert (one.eligible == I).all() and torch.equal(one.ptr.cpu(), torch.arange(31))
    wide = model.target_ranks(users, tgt[:90].reshape(30, 3), exclude=seen)
    assert wide.ranks.shape == (30, 3)
    T.check_ranks_band(wide.ranks, users, np.arange(31) * 3, tgt[:90], S, seen, "2-D")
    bad = tgt.copy()
    bad[5] = I
    with pytest.raises(IndexError):
        model.target_ranks(users, ops.CandidateLists(torch.from_numpy(ptr), torch.from_numpy(bad)))
    with pytest.raises(IndexError):
        model.target_ranks(np.full(30, U), cl)
    with pytest.raises(ValueError):
        model.target_ranks(users[:29], cl)
    with pytest.raises(ValueError):
        model.target_ranks(users, tgt[:29])  # 1-D is one target per user, not a shared list
    with pytest.raises(ValueError):
        model.target_ranks(users, ops.CandidateLists(torch.from_numpy(ptr[::-1].copy()), torch.from_numpy(tgt)))
    none = model.target_ranks(users[:0], np.zeros((0, 4), dtype=np.int64))
    assert none.ranks.shape == (0, 4) and none.eligible.shape == (0,)
    empty = model.target_ranks(users[:4], [[], [], [], []])
    assert empty.ranks.shape == (0,) and empty.ptr.tolist() == [0] * 5


def test_trainer_evaluate_ranks_is_evaluate_full():
    import torch.utils.data as data
    from ncf_amd import synthetic
    from ncf_amd.data import NCFData
    from ncf_amd.metrics import rank_report
    from ncf_amd.models import NCF
    from ncf_amd.trainer import Trainer
    ds = synthetic.make_dataset("ml-100k", seed=0)
    Un, In = ds["user_num"], ds["item_num"]
    train = np.stack([ds["train_users"], ds["train_items"]], 1).astype(np.int64).tolist()
    tu = np.repeat(ds["test_users"], 100)
    ti = np.concatenate([ds["test_items"][:, None], ds["test_negatives"]], 1).reshape(-1)
    assert (ds["test_items"] < In).all()
    test = np.stack([tu, ti], 1).astype(np.int64).tolist()
    torch.manual_seed(0)
    model = NCF(Un, In, 8, 3, 0.0, "NeuMF-end").to(DEV)
    loader = data.DataLoader(NCFData(test, In, None, 0, False), batch_size=100, shuffle=False, num_workers=0)
    tr = Trainer(model, NCFData(train, In, None, 4, True), loader, batch_size=256, top_k=10)
    state = torch.get_rng_state()
    r = tr.evaluate_ranks()
    assert torch.equal(state, torch.get_rng_state())  # nothing drawn
    ranks = r.ranks.cpu().numpy()
    assert ranks.shape == (len(ds["test_users"]),) and (ranks < r.eligible.cpu().numpy()).all()
    rep = rank_report(r.ranks, r.ptr, r.eligible, ks=(1, 10, 128))
    for k in (1, 10, 128):
        hr, nd = tr.evaluate_full(k)
        assert hr == [int(x < k) for x in ranks]
        assert nd == np.where(ranks < k, 1.0 / np.log2(ranks + 2.0), 0.0).tolist()
        assert rep["mean"][f"hr@{k}"] == pytest.approx(np.mean(hr), abs=1e-12)
        assert rep["mean"][f"ndcg@{k}"] == pytest.approx(np.mean(nd), abs=1e-12)
    assert (ranks >= 128).any()  # positions recommend cannot report
