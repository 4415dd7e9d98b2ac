"""Distillation (NCF_DZ_KD, ncf_kd_feature_step) on every step kernel, rank shard and
stream edge, against the float64 reference of tests/distill_checks.py (the
ncf_amd.distill modules on stock torch CPU ops in float64, pinned to
tests/golden/G8_distill.npz by tests/test_distill_reference.py).

Criteria: the suite's own, unchanged -- logits rtol 1e-5 / atol 1e-7, loss rtol 1e-5,
gradients by test_gpu_parity._close_grad (terms = the hottest id's row count for an
embedding table), on a draw without ReLU ties (test_gpu_parity._untie); trajectories by
per-step loss rtol 1e-5 and _assert_trajectory_close.  ml-1m ids (6041 x 3707), zipf-hot
items.

Which NCF_DZ_KD epilogue a case reaches (there is no probe of the kernel that ran; the
path follows from the shape as lyr_run / train_step_impl choose it, and each test asserts
the inputs of that choice -- ncf_supported, ncf_fact_mode, the tuned layout flags):
  * fused-per-row, fused-factored (and both at 8 / 4 / 2 / 1 waves): ncf_train.hip;
  * layered-chain (factored, factor_num % 4 == 0, dm 128): lyr_step_chain_kernel;
  * predict-f6, predict-mlp-f11 (factor_num % 4 != 0: no chain), predict-gmf-f5 (no
    tower): lyr_predict_kernel;
  * wide-chain (factored, dm 512, 4 layers: launch_step_chain has no such instantiation,
    wide_chain_applies holds unless NCF_WIDE_CHAIN=0): ncf_chain_wide.inc;
  * test_engine_in_step_adam_response: ncf_train_step_ais.
The feature terms (kd_feature_kernel) run in every `feature` case; FEATURE_CASES add its
S > 64 loops, the identity key and the grid-stride loop.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import distill_checks as C
from test_gpu_parity import _assert_trajectory_close, _close_grad, geometry  # noqa: F401 (geometry: a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEO_OF_WAVES = {8: 0, 4: 1, 2: 2, 1: 3}  # NCF_LAYOUT_GEO field


def _on_device(built):
    teacher, student, d = built
    teacher.to(DEV)
    student.to(DEV)
    d.to(DEV)
    return teacher, student, d, d.device_plan()


def _rows(users, items, labels):
    from ncf_amd import ops
    return torch.as_tensor(ops.pack_rows_host(users, items, labels), device=DEV)


def _feature_step(plan, lay, flat, gflat, rows, ctl, B, world, rank, ws, st):
    """ncf_kd_feature_step with the plan's keys (DeviceDistillPlan.launch's arguments)."""
    import ncf_amd._lib as L
    g = plan.keys.get("gmf_features", (None, None, 0.0))
    m = plan.keys.get("mlp_input", (None, None, 0.0))
    return L.hip().ncf_kd_feature_step(ctypes.byref(lay), flat.data_ptr(), gflat.data_ptr(), ctypes.byref(plan.t_lay),
                                       plan.t_flat.data_ptr(), rows.data_ptr(), ctl.data_ptr(), B, world, rank,
                                       L.ptr(g[0]), L.ptr(g[1]), g[2], L.ptr(m[0]), L.ptr(m[1]), m[2],
                                       ws.data_ptr(), st)


def _one_step_kd(p, world=1, rank=0, tune=False):
    """One distillation step of problem `p` on the device as rank `rank` of `world`:
    teacher logits by ops.forward_logits, ncf_train_step_kd with logits_out,
    ncf_kd_feature_step when the plan has keys, ncf_reduce_slab.  tune: the layout
    ncf_layout_tune shapes for the rank's rows (else the model's own).  Returns (layout,
    loss slot, this rank's logits, {parameter name: gradient})."""
    import ncf_amd._lib as L
    from ncf_amd import ops
    teacher, student, d, plan = _on_device(p.build())
    B = p.B
    per = -(-B // world)
    rows = _rows(p.users, p.items, p.labels)
    tlog = ops.forward_logits(plan.t_flat, plan.t_lay, rows, ws_owner=teacher)
    flat, lay0 = ops.ensure_flat(student)
    lay = type(lay0).from_buffer_copy(lay0)
    if tune:
        L.check(L.hip().ncf_layout_tune(ctypes.byref(lay), per), "tune")
    gflat = torch.zeros(int(lay.total), device=DEV)
    ws = ops.new_workspace(lay, per, DEV)
    ctl = ops.new_ctl(B, DEV)
    logits = torch.full((per,), float("nan"), device=DEV)
    st = L.stream_ptr()
    uord = None
    if L.hip().ncf_uses_user_order(ctypes.byref(lay)):  # as the engine: the rank slices' user order
        uord = torch.empty(B + (B + 1) // 2, dtype=torch.int64, device=DEV)
        L.check(L.hip().ncf_user_order(rows.data_ptr(), B, B, world, p.U, uord.data_ptr(), st), "order")
    L.check(L.hip().ncf_train_step_kd(ctypes.byref(lay), flat.data_ptr(), gflat.data_ptr(), rows.data_ptr(),
                                      L.ptr(uord), tlog.data_ptr(), ctl.data_ptr(), B, world, rank, plan.w_task,
                                      plan.w_resp, plan.temperature, ws.data_ptr(), ws.numel() * 4,
                                      logits.data_ptr(), st), "ncf_train_step_kd")
    assert bool(plan.keys) == (p.strategy == "feature")
    if plan.keys:
        L.check(_feature_step(plan, lay, flat, gflat, rows, ctl, B, world, rank, ws, st), "ncf_kd_feature_step")
    L.check(L.hip().ncf_reduce_slab(ctypes.byref(lay), ws.data_ptr(), gflat.data_ptr(), ctl.data_ptr(), st), "reduce")
    torch.cuda.synchronize()
    grads = {name: gflat[off:off + q.numel()].view_as(q).cpu().numpy().astype(np.float64)
             for (q, off), (name, _) in zip(ops._segments(student, lay), student.named_parameters())}
    return lay, float(gflat[lay.loss_slot].item()), logits.cpu().numpy(), grads


def _compare(p, got, ref, lo=0, hi=None, what=""):
    """Logits, loss and every gradient segment of a device step against a reference step
    over rows [lo, hi) of the problem's batch.  Each figure is printed before it is held."""
    from ncf_amd import ops
    lay, loss, logits, grads = got
    loss_ref, logits_ref, grads_ref = ref
    n = len(logits_ref)
    fact = ops.fact_mode(lay)
    worst = {k: C.grad_excess(grads[k], grads_ref[k], p.terms(k, lo, hi, fact)) for k in grads_ref}
    print(f"{p.case} {p.strategy} {what}: loss rel {abs(loss - loss_ref) / abs(loss_ref):.3g}, logits "
          f"{float((np.abs(logits[:n] - logits_ref) / (C.LOGIT_ATOL + C.LOGIT_RTOL * np.abs(logits_ref))).max()):.3g}"
          f" of tolerance, gradients {max(worst.values()):.3g} of tolerance ({max(worst, key=worst.get)})")
    np.testing.assert_allclose(logits[:n], logits_ref, rtol=C.LOGIT_RTOL, atol=C.LOGIT_ATOL)
    assert np.isnan(logits[n:]).all(), "logits_out written past this rank's rows"
    np.testing.assert_allclose(loss, loss_ref, rtol=C.LOSS_RTOL)
    for name, g in grads.items():
        if name in grads_ref:
            _close_grad(g, grads_ref[name], f"{what} {name}", terms=p.terms(name, lo, hi, fact))
        else:  # a table the loss does not reach (reference grad None): nothing may be written
            assert not g.any(), name


def _assert_path(case, lay, tuned_waves=None):
    """The inputs of the kernel choice for `case` (module doc)."""
    import ncf_amd._lib as L
    from ncf_amd import ops
    mt, f, nl = C.ALL_CASES[case][1]
    dm = f << (nl - 1)
    if case.startswith("fused"):
        assert L.supported(mt, f, nl) == L.PATH_FUSED
        per_row = case == "fused-per-row"
        assert bool(lay.flags & L.LAYOUT_PER_ROW_L0) == per_row and ops.fact_mode(lay) == (not per_row)
        if tuned_waves:  # the forced geometry, or 8 waves where the shape has no narrower kernel
            assert (int(lay.flags) >> L.LAYOUT_GEO_SHIFT) & L.LAYOUT_GEO_MASK in (GEO_OF_WAVES[tuned_waves], 0)
        return
    assert L.supported(mt, f, nl) == L.PATH_LAYERED
    if case == "layered-chain":
        assert ops.fact_mode(lay) and f % 4 == 0 and dm == 128
        assert L.hip().ncf_uses_user_order(ctypes.byref(lay)) == 1
    elif case == "wide-chain":
        assert ops.fact_mode(lay) and f % 4 == 0 and dm == 512 and nl == 4
        assert os.environ.get("NCF_WIDE_CHAIN", "1")[:1] != "0"
    else:
        assert mt == "GMF" or f % 4 != 0  # no chain: lyr_predict_kernel forms dz


@pytest.mark.parametrize("strategy", C.STRATEGIES)
@pytest.mark.parametrize("waves", [0, 8, 4, 2, 1])
@pytest.mark.parametrize("case", ["fused-per-row", "fused-factored"])
def test_one_step_fused(case, waves, strategy, geometry):  # noqa: F811
    """The fused step's NCF_DZ_KD epilogue on the tuned layout: per-row layer 0
    (NeuMF-end(8,3), 1,024 rows) and factored (NeuMF-end(16,3), 8,192 rows), at the tuned
    geometry (waves 0) and with 8 / 4 / 2 / 1-wave workgroups forced."""
    if waves:
        geometry(waves)
    p = C.problem(case, strategy)
    got = _one_step_kd(p, tune=True)
    _assert_path(case, got[0], waves)
    _compare(p, got, p.step(), what=f"waves {waves}")


@pytest.mark.parametrize("strategy", C.STRATEGIES)
@pytest.mark.parametrize("case", [c for c in C.PATH_CASES if not c.startswith("fused")])
def test_one_step_layered(case, strategy):
    """The layered kernels' NCF_DZ_KD epilogues: the step chain, the predict kernel
    (three model types, odd widths and row counts) and the wide chain of NCF(64,4)."""
    p = C.problem(case, strategy)
    got = _one_step_kd(p)
    _assert_path(case, got[0])
    _compare(p, got, p.step())


@pytest.mark.parametrize("case", list(C.FEATURE_CASES))
def test_one_step_feature_kernel_shapes(case):
    """kd_feature_kernel beyond its easiest shapes, feature strategy (T = 2, alpha = 0.5,
    beta = 0.3):
      * s-gt-64: student NeuMF-end(32,3) (mlp_input 256, GMF 32) under teacher
        NeuMF-end(64,4) (1024 / 64) -- the `s += 64` / `o += 64` loops and a 256-term
        (forward) and 1024-term (backward) sequential fp32 dot product per output;
      * identity-gmf: GMF widths equal (no adapter), mlp_input through an adapter;
      * grid-stride: 8,492 rows, more than 2048 blocks x 4 waves.
    _close_grad is kept as it is for s-gt-64: measured on the CPU, the float32 module's
    gradients (ATen's summation order) lie within 0.09 of _close_grad's tolerance of the
    float64 reference at that shape (worst: the first tower weight, 0.092; the user MLP
    table 0.071), so 4x that, the allowance for a second valid fp32 order, is still inside
    the unchanged criterion."""
    p = C.problem(case, "feature")
    got = _one_step_kd(p, tune=True)
    _compare(p, got, p.step())


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("strategy", ["response", "feature"])
@pytest.mark.parametrize("case", list(C.SHARD_CASES))
def test_rank_shards(case, strategy, world):
    """Every rank of world 2 / 3 on the same global batch of 3,001 rows (a fused and a
    layered student): each rank's logits, loss and gradients against the float64 reference
    of its rows [lo, hi) normalised by the global batch, and the ranks' sums against the
    one-rank device step."""
    p = C.problem(case, strategy)
    full = _one_step_kd(p)
    _compare(p, full, p.step(), what="one rank")
    loss, grads = 0.0, {k: np.zeros_like(v) for k, v in full[3].items()}
    for rank in range(world):
        lo, hi = C.shard_bounds(p.B, world, rank)
        got = _one_step_kd(p, world=world, rank=rank)
        _compare(p, got, p.step(lo, hi), lo, hi, what=f"rank {rank}/{world}")
        loss += got[1]
        for k, v in got[3].items():
            grads[k] += v
    from ncf_amd import ops
    fact = ops.fact_mode(full[0])
    np.testing.assert_allclose(loss, full[1], rtol=C.LOSS_RTOL)
    for k, v in full[3].items():
        _close_grad(grads[k], v, f"sum of ranks {k}", terms=p.terms(k, fact=fact))


# ---- stream edges and the engine ------------------------------------------------
ENGINE_STUDENTS = {"fused": ("NeuMF-end", 16, 3), "layered": ("NeuMF-end", 32, 3)}
EU, EI, EB = 600, 400, 1024  # ids small against the batch: factored layer 0, rows hit every step
_traj = {}


def _stream_data(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, EU, n), np.minimum(rng.zipf(1.3, n) - 1, EI - 1),
            (rng.random(n) < 0.2).astype(np.float32))


def _engine_reference(student, strategy, n, steps):
    key = (student, strategy)
    if key not in _traj:
        d64 = C.f64(C.build(C.T_SMALL, ENGINE_STUDENTS[student], strategy, EU, EI, 23)[2])
        _traj[key] = C.trajectory(d64, *_stream_data(n, 47), EB, steps)
    return _traj[key]


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("strategy", ["response", "feature"])
@pytest.mark.parametrize("student", list(ENGINE_STUDENTS))
def test_engine_short_batch_and_wrap(student, strategy, use_graph):
    """TrainEngine(distill=plan) over a stream of 2 B + B // 3 rows for 5 steps: step 2 is
    the short batch (gb < batch_global: the response and feature terms are normalised by
    gb and gb * T), step 3 wraps to batch 0.  run(2) then run(3): with graphs that is an
    eager step, a one-step replay and one replay of the three-step chunk (short batch and
    wrap inside it); the loss history keeps one slot per batch, so it is read after each
    run.  Per-step losses against the float64 trajectory at rtol 1e-5, parameters by
    _assert_trajectory_close."""
    import ncf_amd._lib as L
    from ncf_amd import ops
    from ncf_amd.engine import TrainEngine
    n, steps = 2 * EB + EB // 3, 5
    ref_losses, ref_state = _engine_reference(student, strategy, n, steps)
    sspec = ENGINE_STUDENTS[student]
    _, model, d, plan = _on_device(C.build(C.T_SMALL, sspec, strategy, EU, EI, 23))
    eng = TrainEngine(model, lr=1e-3, distill=plan)
    eng.set_epoch_stream(_rows(*_stream_data(n, 47)), EB)
    assert L.supported(*sspec) == (L.PATH_FUSED if student == "fused" else L.PATH_LAYERED)
    assert ops.fact_mode(eng.lay) and not eng._ais_active and eng.num_batches == 3
    eng.run(2, use_graph=use_graph)
    torch.cuda.synchronize()
    first = eng.epoch_losses()[:3].copy()
    eng.run(3, use_graph=use_graph)
    torch.cuda.synchronize()
    last = eng.epoch_losses()[:3].copy()
    got = np.array([first[0], first[1], last[2], last[0], last[1]])
    print(f"{student} {strategy} graph {use_graph}: loss rel {np.abs(got - ref_losses) / ref_losses}")
    np.testing.assert_allclose(got, ref_losses, rtol=1e-5)
    assert eng.state_step() == steps
    for k, v in model.state_dict().items():
        _assert_trajectory_close(v.cpu().numpy(), ref_state[k], steps, 1e-3, k)


def test_engine_in_step_adam_response():
    """Response distillation at C5's shapes (teacher NeuMF-end(16,3), student MLP(8,2),
    ml-1m ids, 256-row batches) with the in-step Adam launch (ncf_train_step_ais carries
    the teacher logits and its own NCF_DZ_KD epilogue) and without: the two agree as
    test_gpu_ais.py requires of the BCE case (losses rtol 1e-6, parameters by
    _assert_trajectory_close, moments rtol 1e-4 / atol 1e-9), and each matches the float64
    trajectory."""
    from ncf_amd.engine import TrainEngine
    U, I = C.ML1M
    B, T = 256, 12
    tspec, sspec = ("NeuMF-end", 16, 3), ("MLP", 8, 2)
    rng = np.random.default_rng(5)
    data = (rng.integers(0, U, T * B), np.minimum(rng.zipf(1.3, T * B) - 1, I - 1),
            (rng.random(T * B) < 0.2).astype(np.float32))
    ref_losses, ref_state = C.trajectory(C.f64(C.build(tspec, sspec, "response", U, I, 7)[2]), *data, B, T)
    out = []
    for on in (True, False):
        old = TrainEngine.ADAM_IN_STEP
        TrainEngine.ADAM_IN_STEP = on
        try:
            _, model, d, plan = _on_device(C.build(tspec, sspec, "response", U, I, 7))
            eng = TrainEngine(model, lr=1e-3, distill=plan)
            eng.set_epoch_stream(_rows(*data), B)
            assert eng._ais_active == on
            eng.run(T, use_graph=True)
            torch.cuda.synchronize()
            assert not eng._ais_live and eng.state_step() == T
            out.append(({k: v.cpu().numpy().copy() for k, v in model.state_dict().items()},
                        eng.epoch_losses()[:T].copy(),
                        (eng.exp_avg.cpu().numpy().copy(), eng.exp_avg_sq.cpu().numpy().copy())))
        finally:
            TrainEngine.ADAM_IN_STEP = old
    (a, la, sa), (b, lb, sb) = out
    assert np.all(la > 0)
    np.testing.assert_allclose(la, lb, rtol=1e-6)
    for k in a:
        _assert_trajectory_close(a[k], b[k], T, 1e-3, k)
    for x, y in zip(sa, sb):
        np.testing.assert_allclose(x, y, rtol=1e-4, atol=1e-9)
    for state, losses in ((a, la), (b, lb)):
        np.testing.assert_allclose(losses, ref_losses, rtol=1e-5)
        for k in state:
            _assert_trajectory_close(state[k], ref_state[k], T, 1e-3, k)


def test_feature_step_refusals():
    """ncf_kd_feature_step refuses before it launches: student mlp_input above 1024,
    teacher mlp_input above 2048 or a GMF width above 64 are NCF_E_UNSUPPORTED; identity
    with unequal widths, an adapter without a bias or rank >= world are NCF_E_ARG.  Every
    buffer is real and sized for its layout."""
    import ncf_amd._lib as L
    from ncf_amd import ops
    U = I = 4
    rows = _rows(np.arange(1), np.arange(1), np.zeros(1))  # one row: one wave of the control launch
    ctl = ops.new_ctl(1, DEV)
    st = L.stream_ptr()

    def call(sspec, tspec, gmf, mlp, world=1, rank=0):
        """gmf / mlp: None (key off), "id" (identity), "adapter" or "nobias"."""
        sl = L.layout(U, I, sspec[1], sspec[2], sspec[0])
        tl = L.layout(U, I, tspec[1], tspec[2], tspec[0])
        sp, sg = torch.zeros(int(sl.total), device=DEV), torch.zeros(int(sl.total), device=DEV)
        tp = torch.zeros(int(tl.total), device=DEV)
        ws = torch.zeros(int(sl.tower_len) + 64, device=DEV)
        keys, keep = [], []
        for kind, S, T in ((gmf, sspec[1], tspec[1]),
                           (mlp, 2 * (sspec[1] << (sspec[2] - 1)), 2 * (tspec[1] << (tspec[2] - 1)))):
            w = torch.zeros(T * S, device=DEV) if kind in ("adapter", "nobias") else None
            b = torch.zeros(T, device=DEV) if kind == "adapter" else None
            keep += [w, b]
            keys += [L.ptr(w), L.ptr(b), 0.0 if kind is None else 0.1]
        rc = L.hip().ncf_kd_feature_step(ctypes.byref(sl), sp.data_ptr(), sg.data_ptr(), ctypes.byref(tl),
                                         tp.data_ptr(), rows.data_ptr(), ctl.data_ptr(), 1, world, rank, *keys,
                                         ws.data_ptr(), st)
        torch.cuda.synchronize()
        del keep
        return rc

    small, mid = ("NeuMF-end", 8, 2), ("NeuMF-end", 16, 2)
    assert call(small, mid, "adapter", "adapter") == L.NCF_OK  # the control: a supported pair runs
    assert call(("NeuMF-end", 72, 4), small, None, "adapter") == L.NCF_E_UNSUPPORTED   # S = 1152 > 1024
    assert call(small, ("NeuMF-end", 136, 4), None, "adapter") == L.NCF_E_UNSUPPORTED  # T = 2176 > 2048
    assert call(("NeuMF-end", 72, 1), small, "adapter", None) == L.NCF_E_UNSUPPORTED   # GMF S = 72 > 64
    assert call(small, ("NeuMF-end", 72, 1), "adapter", None) == L.NCF_E_UNSUPPORTED   # GMF T = 72 > 64
    assert call(small, mid, "id", None) == L.NCF_E_ARG      # identity, 8 != 16
    assert call(small, mid, None, "id") == L.NCF_E_ARG      # identity, 32 != 64
    assert call(small, mid, "nobias", None) == L.NCF_E_ARG  # adapter without a bias
    assert call(small, mid, "adapter", "adapter", world=2, rank=2) == L.NCF_E_ARG
    assert call(small, mid, "adapter", "adapter", world=2, rank=-1) == L.NCF_E_ARG


def test_stream_switch_keeps_no_stale_teacher_logits():
    """Stream A (n1 rows), stream B (n2 rows), A again, with captured step graphs.  The
    plan keeps one teacher-logit buffer and replaces it when the stream length changes;
    a graph captured for A holds the pointer of the buffer A had then.  Before the third
    run either that graph is gone from eng._graphs or the buffer in use is the one it
    holds (a pointer comparison; a block of A's size is held in between, so the caching
    allocator cannot hand the freed buffer back and hide a stale pointer), and the third
    pass's losses match the float64 trajectory."""
    from ncf_amd.engine import TrainEngine
    B, n1, n2, steps = 256, 3 * 256, 2 * 256 + 100, 3
    sspec = ENGINE_STUDENTS["fused"]
    da, db = _stream_data(n1, 61), _stream_data(n2, 62)
    d64 = C.f64(C.build(C.T_SMALL, sspec, "response", EU, EI, 29)[2])
    opt = torch.optim.Adam(d64.student_model.parameters(), lr=1e-3)
    ref = [C.trajectory(d64, *data, B, steps, opt=opt)[0] for data in (da, db, da)]
    _, model, d, plan = _on_device(C.build(C.T_SMALL, sspec, "response", EU, EI, 29))
    eng = TrainEngine(model, lr=1e-3, distill=plan)
    rows_a, rows_b = _rows(*da), _rows(*db)
    eng.set_epoch_stream(rows_a, B)
    eng.run(steps, use_graph=True)
    key_a = (B, n1, rows_a.data_ptr())
    assert key_a in eng._graphs
    ptr_a = plan.tlog.data_ptr()
    torch.cuda.synchronize()
    np.testing.assert_allclose(eng.epoch_losses()[:steps], ref[0], rtol=1e-5)
    eng.set_epoch_stream(rows_b, B)
    hold = torch.empty(n1, dtype=torch.float32, device=DEV)  # takes the block A's logits had, if freed
    eng.run(steps, use_graph=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(eng.epoch_losses()[:steps], ref[1], rtol=1e-5)
    eng.set_epoch_stream(rows_a, B)
    assert key_a not in eng._graphs or plan.tlog.data_ptr() == ptr_a
    eng.run(steps, use_graph=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(eng.epoch_losses()[:steps], ref[2], rtol=1e-5)
    del hold
