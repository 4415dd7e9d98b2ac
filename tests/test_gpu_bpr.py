"""Pairwise (BPR) training on the device: ncf_build_pair_stream, NCF_DZ_BPR through every
kernel that forms dz, TrainEngine(loss="bpr"), EpochPipeline(pairwise=True) and
Trainer(loss="bpr"), against the CPU oracle (tests/bpr_checks.py: OracleNCF under torch
autograd with ncf_amd.losses.bpr_loss and torch.optim) at the project's tolerances.

Which shapes reach which dz site (ncf_step.hip train_step_impl, ncf_layered.hip lyr_run):
  * ncf_train.hip ncf_step_kernel<..., BPR> (fused path, ncf_supported == 1): NeuMF(8,3),
    NeuMF(16,3), MLP(16,2), GMF(16,1).  Untuned layouts run the 8-wave kernel (128-row
    tiles), factored layer 0 for the tower shapes (U + I <= 32,768); ncf_layout_tune at
    ml-1m ids keeps the factored kernel from 4,874 rows; ncf_debug_set_geometry forces
    the 64 / 32 / 16-row tiles.
  * ncf_layered.hip lyr_step_chain_kernel<DM, L, false, BPR> (layered, factored layer 0,
    factor_num % 4 == 0, dm <= 128): NeuMF(32,3) -- dm 128 -- on an untuned layout.
  * ncf_chain_wide.inc lyr_wide_chain_kernel<BPR> (layered, factored, dm 512, L 4):
    NeuMF(64,4) on an untuned layout, and on a tuned one from 4,874 rows (2,437 triples:
    the smallest batch ncf_layout_tune leaves factored at ml-1m ids).
  * ncf_layered.hip lyr_predict_kernel<true, NS, BPR> (layered, no chain): factor_num % 4
    != 0 -- NeuMF(6,3), GMF(5,1), MLP(1,1) -- and NeuMF(64,4) with per-row layer 0 (the
    tuned layout at 500 triples).
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
from oracle import ncf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ML1M = (6041, 3707)


# --------------------------------------------------------------------------- helpers
def _pack(users, items, labels):
    from ncf_amd import ops
    return torch.as_tensor(ops.pack_rows_host(users, items, labels), device=DEV)


def _launch(m, lay, rows, batch_rows, dz, dlogit=None, batch=0, world=1):
    """One ncf_train_step + ncf_reduce_slab on global batch `batch` of `rows`; returns
    (return code, logits_out [batch_rows], flat gradient)."""
    import ncf_amd._lib as L
    from ncf_amd import ops
    flat = m._ncf_flat
    gflat = torch.zeros(int(lay.total), device=DEV)
    ws = ops.new_workspace(lay, batch_rows, DEV)
    ctl = ops.new_ctl(rows.numel(), DEV, batch=batch)
    logits = torch.full((batch_rows,), float("nan"), device=DEV)
    st = L.stream_ptr()
    rc = L.hip().ncf_train_step(ctypes.byref(lay), flat.data_ptr(), gflat.data_ptr(), rows.data_ptr(), None,
                                None if dlogit is None else dlogit.data_ptr(), ctl.data_ptr(), batch_rows, world, 0,
                                dz, ws.data_ptr(), ws.numel() * 4, logits.data_ptr(), st)
    if rc == 0:
        L.check(L.hip().ncf_reduce_slab(ctypes.byref(lay), ws.data_ptr(), gflat.data_ptr(), ctl.data_ptr(), st),
                "reduce")
    torch.cuda.synchronize()
    return rc, logits, gflat


def _device_model(m, tuned_rows=None):
    """(model on the device, a private copy of its layout, tuned for tuned_rows if given)."""
    import ncf_amd._lib as L
    from ncf_amd import ops
    m = m.to(DEV)
    lay = ops.ensure_flat(m)[1]
    lay = type(lay).from_buffer_copy(lay)
    if tuned_rows:
        L.check(L.hip().ncf_layout_tune(ctypes.byref(lay), int(tuned_rows)), "tune")
    return m, lay


def _compare_grads(m, lay, gflat, grads_ref, users, items):
    from ncf_amd import ops
    ok = np.asarray(users) >= 0
    for (p, off), (name, _) in zip(ops._segments(m, lay), m.named_parameters()):
        got = gflat[off:off + p.numel()].view_as(p).cpu().numpy()
        if name not in grads_ref:  # unused in this model type (reference grad None): nothing written
            assert not got.any(), name
            continue
        ids = np.asarray(items)[ok] if "item" in name else np.asarray(users)[ok]
        hot = int(np.bincount(ids).max())
        if ops.fact_mode(lay) and name == "MLP_layers.1.weight":
            # factored layer 0: dW0 = sum_u G_u^T Um[u] (+ items), G_u summed by float atomics
            hot = max(int(np.bincount(np.asarray(items)[ok]).max()), int(np.bincount(np.asarray(users)[ok]).max()))
            C.close_grad(got, grads_ref[name].numpy(), name, terms=hot)
            continue
        C.close_grad(got, grads_ref[name].numpy(), name, terms=hot if "embed" in name else None)


def _one_step(mt, f, Lyr, T, U, I, data_seed, tuned=False, path=None, fact=None, seed=11):
    """Logits, loss and every gradient of one NCF_DZ_BPR step over T triples vs the oracle."""
    import ncf_amd._lib as L
    from ncf_amd import ops
    if path is not None:
        assert L.supported(mt, f, Lyr) == path
    ref, m = C.models(mt, f, Lyr, U, I, seed)
    m, lay = _device_model(m, 2 * T if tuned else None)
    if fact is not None:
        assert ops.fact_mode(lay) == fact
    u, ip, ineg = C.draw_triples(ref, T, U, I, data_seed)
    users, items, labels = C.interleave(u, ip, ineg)
    z_ref, loss_ref, g_ref = C.bpr_forward_backward(ref, users, items)
    rc, logits, gflat = _launch(m, lay, _pack(users, items, labels), 2 * T, L.DZ_BPR)
    assert rc == 0
    np.testing.assert_allclose(logits.cpu().numpy(), z_ref.numpy(), rtol=C.LOGIT_RTOL, atol=C.LOGIT_ATOL)
    np.testing.assert_allclose(gflat[lay.loss_slot].item(), loss_ref, rtol=C.LOSS_RTOL)
    _compare_grads(m, lay, gflat, g_ref, users, items)
    return m, lay, (users, items, labels), logits, gflat


# --------------------------------------------------------------------------- pair stream
@pytest.mark.parametrize("P,ng", [(1, 1), (1000, 4)])
@pytest.mark.parametrize("with_perm", [False, True])
def test_build_pair_stream_bit_equal_to_host(P, ng, with_perm):
    from ncf_amd import ops
    rng = np.random.default_rng(P + ng)
    pu = rng.integers(0, 500, P).astype(np.int32)
    pi = rng.integers(0, 700, P).astype(np.int32)
    neg = rng.integers(0, 700, P * ng).astype(np.int32)
    perm = rng.permutation(P * ng).astype(np.int64) if with_perm else None
    got = ops.build_pair_stream(torch.as_tensor(pu, device=DEV), torch.as_tensor(pi, device=DEV),
                                torch.as_tensor(neg, device=DEV), ng,
                                None if perm is None else torch.as_tensor(perm, device=DEV))
    want = ops.bpr_stream_host(pu, pi, neg, ng, perm)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    ops.check_pair_rows(got, 500, 700)


# --------------------------------------------------------------------------- one step
FUSED_MODELS = [("NeuMF-end", 8, 3), ("NeuMF-end", 16, 3), ("NeuMF-pre", 8, 3), ("MLP", 16, 2), ("GMF", 16, 1)]
# data seed per triple count: draws for which the kink redraw stays within 1% (checked on the CPU)
FUSED_T = {8: 3, 9: 3, 64: 3, 65: 3, 1000: 3, 4097: 3}


@pytest.mark.parametrize("mt,f,Lyr", FUSED_MODELS)
@pytest.mark.parametrize("T", list(FUSED_T))
def test_one_step_fused_vs_oracle(mt, f, Lyr, T):
    """Fused kernel, 128-row tiles: fewer rows than a tile, an odd triple count, more than
    one tile, more than one block's tile (4,097 triples = 65 tiles)."""
    _one_step(mt, f, Lyr, T, 50, 80, FUSED_T[T], path=1)


@pytest.mark.parametrize("T", [4096, 34268])
def test_one_step_fused_ml1m_tuned_factored(T):
    """ml-1m ids on the tuned layout: the factored layer 0 runs; 34,268 triples are more
    than 256 tiles of 128 rows (workgroups walk several tiles)."""
    _one_step("NeuMF-end", 16, 3, T, *ML1M, data_seed=3, tuned=True, path=1, fact=True)


@pytest.mark.parametrize("waves", [8, 4, 2, 1])
def test_one_step_fused_forced_geometry(waves):
    import ncf_amd._lib as L
    L.check(L.hip().ncf_debug_set_geometry(waves), "geometry")
    try:
        _, lay, _, _, _ = _one_step("NeuMF-end", 8, 3, 65, 50, 80, 3, tuned=True, path=1)
        assert (8, 4, 2, 1)[(lay.flags >> L.LAYOUT_GEO_SHIFT) & L.LAYOUT_GEO_MASK] == waves
    finally:
        L.hip().ncf_debug_set_geometry(0)


# (model, f, L, triples, tuned, factored) -- the dz site each reaches: module docstring
LAYERED = [("NeuMF-end", 32, 3, 2048, False, True),    # lyr_step_chain_kernel<128, 3>
           ("NeuMF-end", 64, 4, 500, False, True),     # lyr_wide_chain_kernel, a partial 128-row tile
           ("NeuMF-end", 64, 4, 2437, True, True),     # the smallest tuned batch on the wide chain
           ("NeuMF-end", 64, 4, 500, True, False),     # per-row layer 0: lyr_predict_kernel<true, 1>
           ("NeuMF-end", 6, 3, 1501, False, False),    # lyr_predict_kernel (f % 4 != 0)
           ("GMF", 5, 1, 1000, False, False),
           ("MLP", 1, 1, 150, False, False)]


@pytest.mark.parametrize("mt,f,Lyr,T,tuned,fact", LAYERED)
def test_one_step_layered_vs_oracle(mt, f, Lyr, T, tuned, fact):
    _one_step(mt, f, Lyr, T, *ML1M, data_seed=3, tuned=tuned, path=2, fact=fact)


@pytest.mark.parametrize("mt,f,Lyr,T,U,I", [("NeuMF-end", 16, 3, 65, 50, 80), ("NeuMF-end", 32, 3, 300, *ML1M),
                                            ("NeuMF-end", 6, 3, 301, *ML1M)])
def test_self_consistency_with_dlogit_mode(mt, f, Lyr, T, U, I):
    """The same batch through NCF_DZ_DLOGIT, fed the per-row dL/dlogit computed on the host
    from the BPR step's own logits_out, gives the same gradients (gradient rule)."""
    import ncf_amd._lib as L
    m, lay, (users, items, labels), logits, g_bpr = _one_step(mt, f, Lyr, T, U, I, 5)
    z = logits.cpu().numpy().astype(np.float64)
    d = z[0::2] - z[1::2]
    gp = -(1.0 / (1.0 + np.exp(d))) / T
    dl = np.empty(2 * T, dtype=np.float32)
    dl[0::2], dl[1::2] = gp, -gp
    rc, _, g_dl = _launch(m, lay, _pack(users, items, labels), 2 * T, L.DZ_DLOGIT,
                          dlogit=torch.as_tensor(dl, device=DEV))
    assert rc == 0
    from ncf_amd import ops
    for (p, off), (name, _) in zip(ops._segments(m, lay), m.named_parameters()):
        a = g_bpr[off:off + p.numel()].cpu().numpy()
        b = g_dl[off:off + p.numel()].cpu().numpy()
        ids = items if "item" in name else users
        C.close_grad(a, b, name, terms=int(np.bincount(ids).max()) if "embed" in name or "layers.1.weight" in name
                     else None)


@pytest.mark.parametrize("mt,f,Lyr,path", [("NeuMF-end", 8, 3, 1), ("NeuMF-end", 32, 3, 2), ("NeuMF-end", 6, 3, 2)])
def test_partial_last_batch_divides_by_its_triples(mt, f, Lyr, path):
    """Stream of 2 * (3B + 5) rows, batch 2B, B = 64: the fourth step trains 5 triples and
    its loss and gradients divide by 5."""
    import ncf_amd._lib as L
    B, U, I = 64, 50, 80
    ref, m = C.models(mt, f, Lyr, U, I, 11)
    m, lay = _device_model(m)
    u, ip, ineg = C.draw_triples(ref, 3 * B + 5, U, I, 12)
    users, items, labels = C.interleave(u, ip, ineg)
    lu, li = users[-10:], items[-10:]
    z_ref, loss_ref, g_ref = C.bpr_forward_backward(ref, lu, li)  # the mean over the 5 triples
    rc, logits, gflat = _launch(m, lay, _pack(users, items, labels), 2 * B, L.DZ_BPR, batch=3)
    assert rc == 0
    np.testing.assert_allclose(logits[:10].cpu().numpy(), z_ref.numpy(), rtol=C.LOGIT_RTOL, atol=C.LOGIT_ATOL)
    assert torch.isnan(logits[10:]).all()  # nothing written past the batch
    np.testing.assert_allclose(gflat[lay.loss_slot].item(), loss_ref, rtol=C.LOSS_RTOL)
    _compare_grads(m, lay, gflat, g_ref, lu, li)


@pytest.mark.parametrize("mt,f,Lyr", [("NeuMF-end", 8, 3), ("NeuMF-end", 32, 3), ("NeuMF-end", 6, 3)])
def test_padding_pairs_are_skipped_divisor_unchanged(mt, f, Lyr):
    """Padding pairs (both rows user -1) add nothing; T still counts them."""
    import ncf_amd._lib as L
    T, U, I = 200, 50, 80
    ref, m = C.models(mt, f, Lyr, U, I, 11)
    m, lay = _device_model(m)
    u, ip, ineg = C.draw_triples(ref, T, U, I, 13)
    pad = np.zeros(T, dtype=bool)
    pad[[0, 7, 63, 64, 127, 128, 199]] = True
    pad[np.random.default_rng(1).integers(0, T, 20)] = True
    u = np.where(pad, -1, u)
    users, items, labels = C.interleave(u, ip, ineg)
    z_ref, loss_ref, g_ref = C.bpr_forward_backward(ref, users, items, divisor=T)
    rc, logits, gflat = _launch(m, lay, _pack(users, items, labels), 2 * T, L.DZ_BPR)
    assert rc == 0
    ok = users >= 0
    np.testing.assert_allclose(logits.cpu().numpy()[ok], z_ref.numpy()[ok], rtol=C.LOGIT_RTOL, atol=C.LOGIT_ATOL)
    np.testing.assert_allclose(gflat[lay.loss_slot].item(), loss_ref, rtol=C.LOSS_RTOL)
    _compare_grads(m, lay, gflat, g_ref, users, items)


# --------------------------------------------------------------------------- refusals
def test_c_abi_refusals():
    import ncf_amd._lib as L
    from ncf_amd.engine import TrainEngine
    _, m = C.models("NeuMF-end", 8, 3, *ML1M, 11)
    m, lay = _device_model(m)
    users, items, labels = C.interleave(np.arange(64), np.arange(64), np.arange(64) + 1)
    rows = _pack(users, items, labels)
    assert _launch(m, lay, rows, 128, L.DZ_BPR, world=2)[0] == L.NCF_E_ARG
    assert _launch(m, lay, rows, 127, L.DZ_BPR)[0] == L.NCF_E_ARG
    assert _launch(m, lay, rows, 128, L.DZ_BPR)[0] == 0
    # in-step Adam refuses the mode, on a shape and batch where it runs BCE
    eng = TrainEngine(m, lr=1e-3)
    eng.set_epoch_stream(rows, 128)
    assert L.hip().ncf_ais_supported(ctypes.byref(eng.lay)) == 1
    b = eng._ais_bufs()

    def ais(dz):
        return L.hip().ncf_train_step_ais(ctypes.byref(eng.lay), eng.flat.data_ptr(), eng.grads.data_ptr(),
                                          eng.exp_avg.data_ptr(), eng.exp_avg_sq.data_ptr(), ctypes.byref(b),
                                          eng._ranges, eng._nranges, rows.data_ptr(), None, eng.ctl.data_ptr(), 128,
                                          dz, 0.0, 0.0, 0.0, 1e-3, 0.9, 0.999, 1e-8, eng.loss_hist.data_ptr(),
                                          eng.num_batches, 0, L.stream_ptr())
    assert ais(L.DZ_BPR) == L.NCF_E_ARG
    torch.cuda.synchronize()


def test_engine_and_trainer_value_errors():
    from ncf_amd.data import NCFData
    from ncf_amd.engine import TrainEngine
    from ncf_amd.trainer import Trainer
    _, m = C.models("NeuMF-end", 8, 3, 50, 80, 1)
    m = m.to(DEV)
    with pytest.raises(ValueError):
        TrainEngine(m, loss="bpr", world_size=2, dp_mode="allreduce")
    with pytest.raises(ValueError):
        TrainEngine(m, loss="bpr", distill=object())
    with pytest.raises(ValueError):
        TrainEngine(m, loss="hinge")
    eng = TrainEngine(m, loss="bpr")
    assert eng._ais_active is False
    users, items, labels = C.interleave(np.arange(40), np.arange(40), np.arange(40) + 1)
    rows = _pack(users, items, labels)
    with pytest.raises(ValueError):
        eng.set_epoch_stream(rows, 7)           # an odd batch row count
    with pytest.raises(ValueError):
        eng.set_epoch_stream(rows[:79].contiguous(), 8)  # an odd stream length
    bad = _pack(users, items, 1 - labels)
    with pytest.raises(ValueError):
        eng.set_epoch_stream(bad, 8)            # labels (0, 1): check_pair_rows
    with pytest.raises(IndexError):
        eng.set_epoch_stream(_pack(users + 20, items, labels), 8)
    eng.set_epoch_stream(rows, 8)
    assert eng._ais_active is False
    pairs = np.stack([np.arange(30), np.arange(30)], 1)
    with pytest.raises(ValueError):
        Trainer(m, NCFData(pairs, 80, None, 0, True), None, loss="bpr")
    with pytest.raises(ValueError):
        Trainer(m, NCFData(pairs, 80, None, 4, True), None, loss="bpr", world_size=2)


# --------------------------------------------------------------------------- trajectories
TRAJ_U, TRAJ_I, TRAJ_B = 50, 80, 128


@functools.lru_cache(maxsize=None)
def _trajectory(mt, f, Lyr, opt, steps, lr):
    """The oracle's BPR trajectory on the CPU, computed once: a pair stream whose batch t
    is tie-free at the oracle's parameters before step t, the per-step losses and the
    state (parameters, Adam moments) before every step and after the last."""
    ref, _ = C.models(mt, f, Lyr, TRAJ_U, TRAJ_I, 3)
    o = O.make_optimizer(ref, lr, opt)
    rng_seed = 100
    users, items, losses, states, touched = [], [], [], [], 0
    for t in range(steps):
        rng = np.random.default_rng(rng_seed + t)
        u = rng.integers(0, TRAJ_U, TRAJ_B)
        ip = rng.integers(0, TRAJ_I, TRAJ_B)
        ineg = rng.integers(0, TRAJ_I, TRAJ_B)
        u, n = C.untie_triples(ref, u, ip, ineg, TRAJ_U, rng)
        touched += n
        us, its, _ = C.interleave(u, ip, ineg)
        states.append(_snapshot(ref, o))
        losses += C.bpr_train_steps(ref, o, [us], [its])
        users.append(us)
        items.append(its)
    states.append(_snapshot(ref, o))
    assert touched <= C.TIE_MAX_FRACTION * steps * TRAJ_B, f"{touched} triples redrawn"
    users, items = np.stack(users), np.stack(items)
    gap = C.f64_drift(mt, f, Lyr, TRAJ_U, TRAJ_I, 3, users, items, lr, opt)
    return users, items, np.array(losses), states, gap


def _snapshot(ref, o):
    out = {}
    for k, p in ref.named_parameters():
        st = o.state.get(p, {})
        out[k] = (p.detach().clone(), st["exp_avg"].clone() if "exp_avg" in st else None,
                  st["exp_avg_sq"].clone() if "exp_avg_sq" in st else None)
    return out


def _run_trajectory(mt, f, Lyr, opt, steps, lr, use_graph):
    from ncf_amd import ops
    from ncf_amd.engine import TrainEngine
    users, items, losses_ref, states, gap = _trajectory(mt, f, Lyr, opt, steps, lr)
    _, m = C.models(mt, f, Lyr, TRAJ_U, TRAJ_I, 3)
    m = m.to(DEV)
    eng = TrainEngine(m, lr=lr, optimizer=opt, loss="bpr")
    labels = np.tile(np.array([1, 0]), users.size // 2)
    eng.set_epoch_stream(_pack(users.reshape(-1), items.reshape(-1), labels), 2 * TRAJ_B)
    assert eng.num_batches == steps
    # free-running: two fp32 runs may each drift from exact arithmetic by the fp32 oracle's
    # own gap to the float64 oracle
    eng.run(steps, use_graph=use_graph)
    torch.cuda.synchronize()
    tol = max(1e-5, 4 * gap)
    np.testing.assert_allclose(eng.epoch_losses()[:steps], losses_ref, rtol=tol)
    assert eng.state_step() == steps
    # the hard gate: every step from the oracle's state
    segs = ops._segments(m, eng.lay)
    names = [k for k, _ in m.named_parameters()]
    for t in range(steps):
        with torch.no_grad():
            for (p, off), k in zip(segs, names):
                w, ea, es = states[t][k]
                n = w.numel()
                eng.flat[off:off + n].copy_(w.reshape(-1))
                if opt == "adam":
                    eng.exp_avg[off:off + n].copy_(ea.reshape(-1) if ea is not None else torch.zeros(n))
                    eng.exp_avg_sq[off:off + n].copy_(es.reshape(-1) if es is not None else torch.zeros(n))
        eng.ctl[0] = t
        eng.ctl[1] = t
        eng.optimizer_state_set()
        eng.run(1, use_graph=False)
        torch.cuda.synchronize()
        np.testing.assert_allclose(eng.epoch_losses()[t], losses_ref[t], rtol=C.LOSS_RTOL, err_msg=f"loss step {t}")
        for (p, off), k in zip(segs, names):
            got = eng.flat[off:off + p.numel()].view_as(p).cpu().numpy()
            np.testing.assert_allclose(got, states[t + 1][k][0].numpy(), rtol=1e-5, atol=5e-3 * lr,
                                       err_msg=f"{k} after step {t}")


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_bpr_adam_trajectory(use_graph):
    """100 Adam steps of NeuMF-end(8,3), 128 triples per batch, eager and graph-replayed:
    every step teacher-forced from the oracle's state (loss rtol 1e-5, parameters rtol
    1e-5 + 5e-3 * lr), and the free-running per-step losses against the oracle within
    4 x the float32-vs-float64 oracle gap on the same stream, floored at 1e-5.
    Measured on the CPU for these 100 steps: gap 1.40e-07 (so the floor, 1e-5, holds)."""
    _run_trajectory("NeuMF-end", 8, 3, "adam", 100, 1e-3, use_graph)


def test_engine_bpr_sgd_trajectory():
    """10 SGD steps (lr 1e-2); measured float32-vs-float64 gap on the CPU: 1.08e-07."""
    _run_trajectory("NeuMF-end", 8, 3, "sgd", 10, 1e-2, True)


@pytest.mark.parametrize("mt,f,Lyr", [("GMF", 8, 1), ("MLP", 8, 3)])
def test_engine_bpr_gmf_mlp_trajectory(mt, f, Lyr):
    """100 Adam steps, graph-replayed; measured float32-vs-float64 gaps on the CPU:
    GMF 1.39e-07, MLP 1.64e-07."""
    _run_trajectory(mt, f, Lyr, "adam", 100, 1e-3, True)


# --------------------------------------------------------------------------- Trainer
def _small_dataset():
    import torch.utils.data as data
    from ncf_amd.data import NCFData
    U, I, ng = 300, 200, 4
    rng = np.random.default_rng(9)
    pairs = np.unique(np.stack([rng.integers(0, U, 3000), rng.integers(0, I, 3000)], 1), axis=0)
    test = np.stack([np.repeat(np.arange(U), 20), rng.integers(0, I, 20 * U)], 1)
    mk = lambda: NCFData(pairs, I, None, ng, True)  # noqa: E731
    loader = data.DataLoader(NCFData(test, I, None, 0, False), batch_size=20, shuffle=False, num_workers=0)
    return mk, loader, U, I, len(pairs) * ng


def test_trainer_bpr_end_to_end(monkeypatch):
    """Two epochs of Trainer(loss="bpr") on a small synthetic set: the pipeline's streams
    are bit-equal to the NCF_HOST_EPOCH=1 streams under the same seeds, the second epoch
    is a prefetch hit, the first epoch's per-batch losses match the oracle replaying that
    stream teacher-forced, and evaluate() runs."""
    from ncf_amd.data import consume_test_pass
    from ncf_amd.engine import TrainEngine
    from ncf_amd.trainer import Trainer, bpr_host_epoch
    mk, loader, U, I, S = _small_dataset()
    B = 256
    # the host epochs (two, a metrics pass between them, as fit() runs them)
    np.random.seed(4)
    torch.manual_seed(4)
    ds_h = mk()
    host = [bpr_host_epoch(ds_h)]
    consume_test_pass()
    host.append(bpr_host_epoch(ds_h))
    # the same through NCF_HOST_EPOCH=1 (models first: building one seeds the torch generator)
    _, m0 = C.models("NeuMF-end", 8, 3, U, I, 21)
    ref, m = C.models("NeuMF-end", 8, 3, U, I, 21)
    np.random.seed(4)
    torch.manual_seed(4)
    monkeypatch.setenv("NCF_HOST_EPOCH", "1")
    tr_h = Trainer(m0.to(DEV), mk(), loader, batch_size=B, loss="bpr", verbose=False)
    assert np.array_equal(tr_h._epoch_stream().cpu().numpy(), host[0])
    monkeypatch.delenv("NCF_HOST_EPOCH")
    # the device pipeline under fit()
    np.random.seed(4)
    torch.manual_seed(4)
    tr = Trainer(m.to(DEV), mk(), loader, batch_size=B, loss="bpr", verbose=False)
    seen = []
    real = tr.engine.set_epoch_stream

    def spy(rows, batch_size, checked=False):
        seen.append((rows.clone(), batch_size))
        return real(rows, batch_size, checked=checked)
    monkeypatch.setattr(tr.engine, "set_epoch_stream", spy)
    res = tr.fit(2)
    torch.cuda.synchronize()
    assert [b for _, b in seen] == [2 * B, 2 * B]
    for e in range(2):
        assert np.array_equal(seen[e][0].cpu().numpy(), host[e]), f"epoch {e}"
    assert tr._pipe.stats["epochs"] == 2 and tr._pipe.stats["prefetch_hits"] == 1
    assert set(res) == {"best_hr", "best_ndcg", "best_epoch", "parameters", "num_layers", "pretraining",
                        "model_type"}
    assert len(tr.history) == 2 and all(np.isfinite(h["loss"]) and h["loss"] > 0 for h in tr.history)
    hr, nd = tr.evaluate()
    assert len(hr) == len(nd) == U
    tr._pipe.close()
    # the first epoch's stream replayed by the oracle, every batch teacher-forced
    us, its, _ = C.unpack_rows(host[0])
    nb = (S + B - 1) // B
    _, m2 = C.models("NeuMF-end", 8, 3, U, I, 21)
    m2 = m2.to(DEV)
    eng = TrainEngine(m2, lr=1e-3, loss="bpr")
    eng.set_epoch_stream(torch.as_tensor(host[0], device=DEV), 2 * B)
    assert eng.num_batches == nb
    from ncf_amd import ops
    o = torch.optim.Adam(ref.parameters(), lr=1e-3)
    segs = ops._segments(m2, eng.lay)
    for t in range(nb):
        with torch.no_grad():
            for (p, off), rp in zip(segs, ref.parameters()):
                st = o.state.get(rp, {})
                n = rp.numel()
                eng.flat[off:off + n].copy_(rp.detach().reshape(-1))
                eng.exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1) if st else torch.zeros(n))
                eng.exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1) if st else torch.zeros(n))
        eng.ctl[0] = t
        eng.ctl[1] = t
        eng.run(1, use_graph=False)
        lo, hi = 2 * B * t, min(2 * B * (t + 1), 2 * S)
        want = C.bpr_train_steps(ref, o, [us[lo:hi]], [its[lo:hi]])[0]
        torch.cuda.synchronize()
        np.testing.assert_allclose(eng.epoch_losses()[t], want, rtol=C.LOSS_RTOL, err_msg=f"batch {t}")


def test_train_neumf_script_bpr_checkpoint(tmp_path, monkeypatch):
    """scripts/train_neumf.py --loss bpr --epochs 1 writes a _bpr checkpoint that loads."""
    from ncf_amd import synthetic
    from ncf_amd.models import NCF
    monkeypatch.chdir(tmp_path)
    ds = synthetic.make_dataset("ml-100k", seed=0)
    synthetic.write_reference_files(ds, "data/processed")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_neumf.py"), "--loss", "bpr",
                          "--epochs", "1", "--factor_num", "8", "--num_layers", "3", "--seed", "0"],
                         capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Epoch 001: Loss=" in out.stdout and "Saved best model: NeuMF_end_3l_8f_bpr_best.pth" in out.stdout
    models = os.path.join(str(tmp_path), "results", "models")
    assert os.listdir(models) == ["NeuMF_end_3l_8f_bpr_best.pth"]  # no BCE-named checkpoint
    sd = torch.load(os.path.join(models, "NeuMF_end_3l_8f_bpr_best.pth"), map_location="cpu", weights_only=True)
    U, I = sd["embed_user_GMF.weight"].shape[0], sd["embed_item_GMF.weight"].shape[0]
    NCF(U, I, 8, 3, 0.0, "NeuMF-end").load_state_dict(sd)
