"""Dynamic negative sampling on the device: ncf_select_negatives (fused and materialised
paths), NCF.hardest_negatives, EpochPipeline(select=), Trainer(negatives="hard") and the
training script, against the CPU oracle with the near-tie rule of tests/hardneg_checks.py.

Shapes.  Fused path (ncf_supported == 1, dm <= 64): 16-pair tiles; m in {1, 4, 5, 16, 40}
by n in {1, 17, 1000} -- n = 1 is less than one tile; at n = 17, m = 4 gives 4 groups per
tile and a partial fifth tile, m = 5 three groups per tile with an idle lane, m = 40 three
tiles per group, the last partial; n = 17 < 50 users projects the rows' users, n = 1000 the
user table; 4,097 groups of 8 at ml-1m ids are 2,049 tiles for 512 workgroups of 4 waves,
so workgroups walk more than one tile.  Materialised path: the layered shapes, and a fused
shape forced there.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bpr_checks as C
import hardneg_checks as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ML1M = (6041, 3707)
U, I = 50, 80
FUSED_MODELS = [("NeuMF-end", 8, 3), ("NeuMF-end", 16, 3), ("NeuMF-pre", 8, 3), ("MLP", 16, 2), ("GMF", 16, 1)]
MS, NS = [1, 4, 5, 16, 40], [1, 17, 1000]


# --------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def _small(mt, f, Lyr):
    """(oracle scores [U, I] of the model, the model on the device), computed once."""
    ref, m = C.models(mt, f, Lyr, U, I, 11)
    S = H.oracle_scores(ref, np.arange(U), np.tile(np.arange(I), (U, 1)))
    return S, m.to(DEV)


def _select(m, users, cand, n=None, m_arg=None, ws_short=0, outputs=True, sentinel=None):
    """One raw ncf_select_negatives call: (rc, items, slots, scores) as NumPy arrays."""
    import ncf_amd._lib as L
    from ncf_amd import ops
    flat, lay = ops.ensure_flat(m)
    u = torch.as_tensor(np.ascontiguousarray(users, dtype=np.int32), device=DEV)
    c = torch.as_tensor(np.ascontiguousarray(cand, dtype=np.int32), device=DEV)
    n = c.shape[0] if n is None else n
    mm = c.shape[1] if m_arg is None else m_arg
    size = max(c.shape[0], 1) + 8
    items = torch.full((size,), -7 if sentinel is None else sentinel, dtype=torch.int32, device=DEV)
    slots = torch.full((size,), -7, dtype=torch.int32, device=DEV)
    scores = torch.full((size,), float("nan"), dtype=torch.float32, device=DEV)
    need = int(L.hip().ncf_select_negatives_workspace_bytes(ctypes.byref(lay), n, mm))
    ws = torch.empty(max(need, 4096) // 4 + 64, dtype=torch.float32, device=DEV)
    rc = L.hip().ncf_select_negatives(ctypes.byref(lay), flat.data_ptr(), u.data_ptr(), c.data_ptr(), n, mm,
                                      items.data_ptr(), slots.data_ptr() if outputs else None,
                                      scores.data_ptr() if outputs else None, ws.data_ptr(),
                                      need - ws_short if ws_short else ws.numel() * 4, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, items.cpu().numpy(), slots.cpu().numpy(), scores.cpu().numpy(), need


def _ok(m, users, cand):
    rc, items, slots, scores, _ = _select(m, users, cand)
    n = len(cand)
    assert rc == 0
    assert (items[n:] == -7).all() and (slots[n:] == -7).all() and np.isnan(scores[n:]).all()  # nothing past n
    return items[:n], slots[:n], scores[:n]


# --------------------------------------------------------------------------- 1. fused path
@pytest.mark.parametrize("mt,f,Lyr", FUSED_MODELS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n", NS)
def test_fused_vs_oracle(mt, f, Lyr, m, n):
    import ncf_amd._lib as L
    assert L.supported(mt, f, Lyr) == 1
    S_all, model = _small(mt, f, Lyr)
    users, cand = H.draw(n, m, U, I)
    items, slots, scores = _ok(model, users, cand)
    H.check_selection(S_all[users[:, None], cand], cand, items, slots, scores, f"fused {mt}({f},{Lyr}) n={n} m={m}")


def test_fused_ml1m_workgroups_walk_tiles():
    import ncf_amd._lib as L
    assert L.supported("NeuMF-end", 16, 3) == 1
    ref, model = C.models("NeuMF-end", 16, 3, *ML1M, 11)
    users, cand = H.draw(4097, 8, *ML1M)
    items, slots, scores = _ok(model.to(DEV), users, cand)
    H.check_selection(H.oracle_scores(ref, users, cand), cand, items, slots, scores, "fused ml-1m n=4097 m=8")


# --------------------------------------------------------------------------- 2. materialised path
# Model seed per shape, chosen from the oracle alone.  MLP(1,1) has one tower unit: where its
# ReLU is dead every candidate scores exactly the predict bias, and at seed 11 that leaves
# 808 of the 1,000 groups undecided by the oracle's own scores; at seed 15 the unit is
# alive for these pairs (0 undecided; the other shapes: 1, 0, 0, 1 at seed 11).
MATERIALISED = [("NeuMF-end", 32, 3, 11), ("NeuMF-end", 64, 4, 11), ("NeuMF-end", 6, 3, 11), ("GMF", 5, 1, 11),
                ("MLP", 1, 1, 15)]


@pytest.mark.parametrize("mt,f,Lyr,seed", MATERIALISED)
def test_materialised_vs_oracle(mt, f, Lyr, seed):
    import ncf_amd._lib as L
    assert L.supported(mt, f, Lyr) == 2
    ref, model = C.models(mt, f, Lyr, *ML1M, seed)
    users, cand = H.draw(1000, 5, *ML1M)
    items, slots, scores = _ok(model.to(DEV), users, cand)
    H.check_selection(H.oracle_scores(ref, users, cand), cand, items, slots, scores, f"materialised {mt}({f},{Lyr})")


def test_materialised_forced_agrees_with_fused():
    from ncf_amd import ops
    S_all, model = _small("NeuMF-end", 8, 3)
    users, cand = H.draw(1000, 5, U, I)
    S = S_all[users[:, None], cand]
    fused = _ok(model, users, cand)
    with ops._select_materialised():  # restores the path in its finally
        mat = _ok(model, users, cand)
    again = _ok(model, users, cand)
    H.check_selection(S, cand, *mat, "materialised (forced) NeuMF-end(8,3)")
    decided = H.oracle_choice(S, cand)[2]
    assert np.array_equal(fused[0][decided], mat[0][decided])
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(fused, again))  # the fused path is back


# --------------------------------------------------------------------------- 3. exact, against ncf_recommend
def _fused_shapes():
    """Every shape with a fused kernel, from ncf_supported (the serving tables and the training
    table are built from one list; GMF has no tower, so one layer count stands for it)."""
    import ncf_amd._lib as L
    return [(mt, f, Lyr) for mt in ("GMF", "MLP", "NeuMF-end") for f in range(1, 65) for Lyr in (1, 2, 3, 4)
            if (mt != "GMF" or Lyr == 1) and L.supported(mt, f, Lyr) == 1]


@pytest.mark.parametrize("mt,f,Lyr", FUSED_MODELS + [s for s in _fused_shapes() if s not in FUSED_MODELS])
def test_fused_scores_are_recommend_bits(mt, f, Lyr):
    """I = 80 <= 128: recommend(all users, k = 80) yields every pair's score bit for bit; the
    slot must be the first argmax of those bits over the group and the score those bits.
    FUSED_MODELS take the whole n x m grid; the other fused shapes n = 17 with m = 5 (an idle
    lane, a partial tile) and m = 40 (three tiles per group)."""
    full = (mt, f, Lyr) in FUSED_MODELS
    _, model = _small(mt, f, Lyr)
    it, sc = model.recommend(torch.arange(U), k=I, exclude=None)
    R = np.empty((U, I), dtype=np.float32)
    R[np.arange(U)[:, None], it.cpu().numpy()] = sc.cpu().numpy()
    for n in ((17, 1000) if full else (17,)):
        for m in (MS if full else (5, 40)):
            users, cand = H.draw(n, m, U, I, seed=5)
            if m >= 4:  # group 0: its user's best item twice, as the two best candidates
                cand[0, 1] = cand[0, 3] = int(np.argmax(R[users[0]]))
            if m >= 5 and n > 1:  # group 1: one id throughout
                cand[1, :] = cand[1, 0]
            items, slots, scores = _ok(model, users, cand)
            G = R[users[:, None], cand]
            want = np.argmax(G, axis=1)  # the first maximum
            assert np.array_equal(slots, want), (n, m)
            assert np.array_equal(scores.view(np.uint32), G[np.arange(n), want].view(np.uint32)), (n, m)
            assert np.array_equal(items, cand[np.arange(n), want]), (n, m)
            if m >= 4:  # the copy in slot 3 never wins over the one in slot 1
                assert slots[0] <= 1 and items[0] == cand[0, 1]
            if m >= 5 and n > 1:
                assert slots[1] == 0


# --------------------------------------------------------------------------- 4. position independence
@pytest.mark.parametrize("m", MS)
def test_position_independence(m):
    _, model = _small("NeuMF-end", 16, 3)
    users, cand = H.draw(1000, m, U, I, seed=7)
    base = _ok(model, users, cand)
    perm = np.random.default_rng(1).permutation(1000)
    shuffled = _ok(model, users[perm], cand[perm])
    head = _ok(model, users[:17], cand[:17])
    for a, b, c in zip(base, shuffled, head):
        assert np.array_equal(a[perm].view(np.uint32), b.view(np.uint32))
        assert np.array_equal(a[:17].view(np.uint32), c.view(np.uint32))


# --------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("forced", [False, True])
def test_refusals(forced):
    import contextlib
    import ncf_amd._lib as L
    from ncf_amd import ops
    _, model = _small("NeuMF-end", 8, 3)
    users, cand = H.draw(40, 4, U, I)
    wide = np.zeros((40, 65), dtype=np.int32)
    with (ops._select_materialised() if forced else contextlib.nullcontext()):
        assert _select(model, users, cand, m_arg=0)[0] == L.NCF_E_ARG
        assert _select(model, users, wide, m_arg=65)[0] == L.NCF_E_ARG
        rc, _, _, _, need = _select(model, users, cand, ws_short=1)
        assert rc == L.NCF_E_ARG and need > 0
        rc, items, slots, scores, _ = _select(model, users, cand, n=0)
        assert rc == L.NCF_OK and (items == -7).all() and (slots == -7).all() and np.isnan(scores).all()
        # the optional outputs left out; neg_out untouched past n
        rc, items, slots, scores, _ = _select(model, users, cand, n=17, outputs=False)
        assert rc == L.NCF_OK and (items[:17] >= 0).all() and (items[17:] == -7).all()
        assert (slots == -7).all() and np.isnan(scores).all()
        assert np.array_equal(items[:17], _ok(model, users[:17], cand[:17])[0])
    assert L.hip().ncf_debug_set_select_path(5) == L.NCF_E_ARG
    lay = ops.ensure_flat(model)[1]
    assert L.hip().ncf_select_negatives_workspace_bytes(ctypes.byref(lay), 10, 0) == -1
    assert L.hip().ncf_select_negatives_workspace_bytes(ctypes.byref(lay), 10, 65) == -1
    assert L.hip().ncf_select_negatives_workspace_bytes(ctypes.byref(lay), 0, 4) == 0


def test_model_surface_on_device():
    from ncf_amd import ops
    S_all, model = _small("NeuMF-end", 8, 3)
    users, cand = H.draw(300, 4, U, I)
    r = model.hardest_negatives(torch.as_tensor(users), torch.as_tensor(cand, device=DEV))
    assert isinstance(r, ops.HardNegatives) and r.items.is_cuda
    assert r.items.dtype == torch.int64 and r.slots.dtype == torch.int64 and r.scores.dtype == torch.float32
    H.check_selection(S_all[users[:, None], cand], cand, r.items.cpu().numpy(), r.slots.cpu().numpy(),
                      r.scores.cpu().numpy(), "NCF.hardest_negatives")
    bad = cand.copy()
    bad[5, 1] = I
    with pytest.raises(IndexError):
        model.hardest_negatives(users, bad)
    with pytest.raises(IndexError):
        model.hardest_negatives(np.full(300, U), cand)
    with pytest.raises(ValueError):
        model.hardest_negatives(users, np.zeros((300, 65), dtype=np.int32))
    with pytest.raises(ValueError):
        model.hardest_negatives(users, cand[:, 0])
    assert model.hardest_negatives(users[:0], cand[:0]).items.numel() == 0


# --------------------------------------------------------------------------- 6. pipeline and Trainer
def _small_dataset():
    """The 300 x 200 synthetic set of test_gpu_bpr._small_dataset."""
    import torch.utils.data as data
    from ncf_amd.data import NCFData
    Us, Is, ng = 300, 200, 4
    rng = np.random.default_rng(9)
    pairs = np.unique(np.stack([rng.integers(0, Us, 3000), rng.integers(0, Is, 3000)], 1), axis=0)
    test = np.stack([np.repeat(np.arange(Us), 20), rng.integers(0, Is, 20 * Us)], 1)
    mk = lambda: NCFData(pairs, Is, None, ng, True)  # noqa: E731
    loader = data.DataLoader(NCFData(test, Is, None, 0, False), batch_size=20, shuffle=False, num_workers=0)
    return mk, loader, Us, Is, pairs, ng


def _fit_spied(monkeypatch, model, mk, loader, B, **kw):
    """fit(2) under seeds (4, 4) with a spy on engine.set_epoch_stream: the streams, batch
    rows and parameter snapshots it saw, and the generator states afterwards."""
    from ncf_amd.trainer import Trainer
    np.random.seed(4)
    torch.manual_seed(4)
    tr = Trainer(model, mk(), loader, batch_size=B, loss="bpr", verbose=False, **kw)
    seen = []
    real = tr.engine.set_epoch_stream

    def spy(rows, batch_size, checked=False):
        seen.append((rows.clone(), batch_size, tr.engine.flat.clone()))
        return real(rows, batch_size, checked=checked)
    monkeypatch.setattr(tr.engine, "set_epoch_stream", spy)
    tr.fit(2)
    torch.cuda.synchronize()
    return tr, seen, (np.random.get_state()[1].copy(), int(np.random.get_state()[2]), torch.get_rng_state().clone())


def test_trainer_hard_negatives_end_to_end(monkeypatch):
    from ncf_amd import ops
    from ncf_amd.data import consume_test_pass, epoch_permutation
    mk, loader, Us, Is, pairs, ng = _small_dataset()
    P, B = len(pairs), 256
    shape = ("NeuMF-end", 8, 3)
    _, m_host = C.models(*shape, Us, Is, 21)
    _, m_pipe = C.models(*shape, Us, Is, 21)
    # the host draws of the two epochs (a metrics pass between them, as fit() runs them)
    np.random.seed(4)
    torch.manual_seed(4)
    ds = mk()
    cands, perms = [], []
    for e in range(2):
        ds.ng_sample()
        cands.append(ds.arrays()[1][P:].reshape(P, ng).copy())
        perms.append(epoch_permutation(P).numpy())
        consume_test_pass()
    # NCF_HOST_EPOCH=1, then the device pipeline
    monkeypatch.setenv("NCF_HOST_EPOCH", "1")
    tr_h, seen_h, state_h = _fit_spied(monkeypatch, m_host.to(DEV), mk, loader, B, negatives="hard")
    monkeypatch.delenv("NCF_HOST_EPOCH")
    tr, seen, state = _fit_spied(monkeypatch, m_pipe.to(DEV), mk, loader, B, negatives="hard")
    assert tr_h._pipe is None and tr._pipe is not None
    assert tr._pipe.stats["epochs"] == 2 and tr._pipe.stats["prefetch_hits"] == 1
    assert np.array_equal(state[0], state_h[0]) and state[1] == state_h[1] and torch.equal(state[2], state_h[2])
    assert len(seen) == len(seen_h) == 2
    # epoch 0: the same parameters, the same select op -> the same stream, bit for bit
    assert torch.equal(seen[0][0], seen_h[0][0])
    for name, runs in (("pipeline", seen), ("host", seen_h)):
        for e, (rows, batch_rows, snap) in enumerate(runs):
            assert batch_rows == 2 * B and rows.numel() == 2 * P
            u, it, y = C.unpack_rows(rows.cpu().numpy())
            perm, cand = perms[e], cands[e]
            assert np.array_equal(y, np.tile([1, 0], P))
            assert np.array_equal(u[0::2], pairs[perm, 0]) and np.array_equal(it[0::2], pairs[perm, 1])
            assert np.array_equal(u[1::2], pairs[perm, 0])
            assert (cand[perm] == it[1::2, None]).any(axis=1).all(), (name, e, "negative outside its candidates")
            model = tr.model if name == "pipeline" else tr_h.model
            with ops.params_view(model, snap):
                ref = H.state_to_oracle(model.state_dict(), Us, Is, shape[1], shape[2], shape[0])
            S = H.oracle_scores(ref, pairs[perm, 0], cand[perm])
            H.check_selection(S, cand[perm], it[1::2], what=f"{name} epoch {e}")
    # the second epoch was selected at trained parameters, not the initial ones
    assert not torch.equal(seen[1][2], seen[0][2])
    assert len(tr.history) == 2 and all(np.isfinite(h["loss"]) and h["loss"] > 0 for h in tr.history)
    tr._pipe.close()


def test_trainer_uniform_stream_unchanged():
    """Trainer(loss="bpr") without negatives= still produces the uniform stream, bit-equal to
    bpr_host_epoch(ds)."""
    from ncf_amd.trainer import Trainer, bpr_host_epoch
    mk, loader, Us, Is, pairs, ng = _small_dataset()
    _, m = C.models("NeuMF-end", 8, 3, Us, Is, 21)
    np.random.seed(4)
    torch.manual_seed(4)
    host = bpr_host_epoch(mk())
    np.random.seed(4)
    torch.manual_seed(4)
    tr = Trainer(m.to(DEV), mk(), loader, batch_size=256, loss="bpr", verbose=False)
    assert tr.negatives == "uniform"
    got = tr._epoch_stream()
    assert tr._pipe.select is None and got.numel() == 2 * len(pairs) * ng
    assert np.array_equal(got.cpu().numpy(), host)
    tr._pipe.close()


def test_pipeline_select_stub_and_bad_return():
    """EpochPipeline(select=) with a stub: P triples in permutation order; a select that
    returns the wrong thing raises."""
    from ncf_amd.data import epoch_permutation
    from ncf_amd.pipeline import EpochPipeline
    mk, _, Us, Is, pairs, ng = _small_dataset()
    P = len(pairs)
    np.random.seed(4)
    torch.manual_seed(4)
    ds = mk()
    ds.ng_sample()
    cand = ds.arrays()[1][P:].reshape(P, ng).copy()
    perm = epoch_permutation(P).numpy()
    np.random.seed(4)
    torch.manual_seed(4)
    pipe = EpochPipeline(mk(), DEV, 256, Is, user_num=Us, pairwise=True, prefetch=False,
                         select=lambda users, c: c[:, 2].contiguous())
    rows = pipe.next_epoch()
    torch.cuda.synchronize()
    assert pipe.n == P and pipe.n_out == 2 * P and rows.numel() == 2 * P
    u, it, y = C.unpack_rows(rows.cpu().numpy())
    assert np.array_equal(u[0::2], pairs[perm, 0]) and np.array_equal(it[0::2], pairs[perm, 1])
    assert np.array_equal(it[1::2], cand[perm, 2]) and np.array_equal(y, np.tile([1, 0], P))
    assert np.array_equal(pipe.ds.arrays()[1][P:].reshape(P, ng), cand)  # _set_device_negatives: the candidates
    pipe.close()
    bad = EpochPipeline(mk(), DEV, 256, Is, user_num=Us, pairwise=True, prefetch=False,
                        select=lambda users, c: c[:, 2])  # not contiguous
    with pytest.raises(ValueError):
        bad.next_epoch()
    bad.close()


# --------------------------------------------------------------------------- 7. script
def test_train_neumf_script_hard_checkpoint(tmp_path, monkeypatch):
    """scripts/train_neumf.py --loss bpr --negatives hard writes only a _bpr_hard checkpoint."""
    from ncf_amd import synthetic
    from ncf_amd.models import NCF
    monkeypatch.chdir(tmp_path)
    ds = synthetic.make_dataset("ml-100k", seed=0)
    synthetic.write_reference_files(ds, "data/processed")
    script = os.path.join(ROOT, "scripts", "train_neumf.py")
    out = subprocess.run([sys.executable, script, "--loss", "bpr", "--negatives", "hard", "--epochs", "1",
                          "--factor_num", "8", "--num_layers", "3", "--seed", "0"],
                         capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Epoch 001: Loss=" in out.stdout and "Saved best model: NeuMF_end_3l_8f_bpr_hard_best.pth" in out.stdout
    models = os.path.join(str(tmp_path), "results", "models")
    assert os.listdir(models) == ["NeuMF_end_3l_8f_bpr_hard_best.pth"]
    sd = torch.load(os.path.join(models, "NeuMF_end_3l_8f_bpr_hard_best.pth"), map_location="cpu", weights_only=True)
    Un, In = sd["embed_user_GMF.weight"].shape[0], sd["embed_item_GMF.weight"].shape[0]
    NCF(Un, In, 8, 3, 0.0, "NeuMF-end").load_state_dict(sd)
