"""GPU tests of ncf_fold_in (fold-in of unseen users) against the float64 reference of
tests/fold_in_checks.py: the gradient and loss at a general point on every kind of shape and
both paths, Adam against the library's dense Adam (bit for bit) and torch's, the step loop
as the composition of its steps, independence of a user from the rest of the call,
free-running trajectories, with_users, the C ABI's refusals, graph capture and the backends.

Tolerances: _close_grad's gate per user (rtol 1e-4, atol 1e-6 * max|g|), the project's loss
gate (rtol 1e-5), _teacher_forced_steps' one-step bound (rtol 1e-5 + atol 5e-3 * lr)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fold_in_checks as C  # noqa: E402
from recommend_checks import check_topk, oracle_scores  # noqa: E402

U, I = 50, 1007
DEV = "cuda:0"
EDGES = [0, 1, 15, 16, 17, 63, 64, 65, 200]  # the tile and four-wave edges
LONG = 3000  # 960 KB of rows at NeuMF-end(16, 3)
# (model type, f, layers, forced generic, counts)
GENERAL = [("GMF", 5, 1, False, EDGES + [LONG]), ("MLP", 6, 2, False, EDGES + [LONG]),
           ("NeuMF-end", 8, 3, False, EDGES + [LONG]), ("NeuMF-end", 16, 3, False, EDGES + [LONG]),
           ("NeuMF-pre", 16, 3, False, EDGES + [LONG]), ("NeuMF-end", 64, 4, False, [n for n in EDGES if n <= 65]),
           ("NeuMF-end", 16, 3, True, EDGES + [LONG])]
FUSED_SHAPES = {("NeuMF-end", 8, 3), ("NeuMF-end", 16, 3), ("NeuMF-pre", 16, 3)}


def _path(generic):
    from ncf_amd import ops
    import contextlib
    return ops._fold_generic() if generic else contextlib.nullcontext()


def _start(m, q, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((q, m.embed_user_GMF.weight.shape[1]), generator=g) * 0.5,
            torch.randn((q, m.embed_user_MLP.weight.shape[1]), generator=g) * 0.5)


def _fold(m, ex, gmf0, mlp0, steps, lr=0.01, betas=(0.9, 0.999), eps=1e-8, wd=0.0, state=None, grad=False,
          generic=False):
    """ops.fold_in on the device; with grad=True also grad_out [Q, f + dm]."""
    from ncf_amd import ops
    q = ex.ptr.numel() - 1
    g = torch.full((q, gmf0.shape[1] + mlp0.shape[1]), float("nan"), device=DEV) if grad else None
    with _path(generic):
        out = ops.fold_in(m, ex, gmf0, mlp0, steps, lr, betas, eps, wd, state, g)
    torch.cuda.synchronize()
    return (out, g) if grad else out


@pytest.fixture(scope="module")
def general_cases():
    """Model, examples (kink-free), start vectors and the float64 references, once per shape."""
    cache = {}

    def get(mt, f, nl, counts, wd):
        key = (mt, f, nl, len(counts))
        if key not in cache:
            m = C.make_model(mt, f, nl, U, I, seed=3, device=DEV)
            m64 = C.to64(m)
            rng = np.random.default_rng(f * 10 + nl)
            gmf0, mlp0 = _start(m, len(counts), 11)
            ex = C.untie(m64, C.make_examples(counts, I, rng, soft=(mt == "MLP")), gmf0, mlp0, rng)
            cache[key] = [m, m64, ex, gmf0, mlp0, {}]
        m, m64, ex, gmf0, mlp0, refs = cache[key]
        if wd not in refs:
            refs[wd] = C.ref_fold(m64, ex, gmf0, mlp0, 1, lr=0.02, weight_decay=wd)
        return m, ex, gmf0, mlp0, refs[wd]
    return get


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("mt,f,nl,generic,counts", GENERAL)
def test_gradient_and_loss_at_a_general_point(general_cases, mt, f, nl, generic, counts, wd):
    import ncf_amd._lib as L
    assert L.supported(mt, f, nl) == (L.PATH_FUSED if (mt, f, nl) in FUSED_SHAPES else L.PATH_LAYERED)
    m, ex, gmf0, mlp0, ref = general_cases(mt, f, nl, counts, wd)
    got, grad = _fold(m, ex, gmf0, mlp0, 1, lr=0.02, wd=wd, grad=True, generic=generic)
    assert not torch.isnan(grad).any()
    C.check_one_step(got, grad, ref, gmf0, mlp0, mt, 0.02, f"{mt}({f},{nl}) generic={generic} wd={wd}")
    # the user without examples
    assert got.loss[0, 0].item() == 0.0
    p0 = torch.cat((gmf0[0], mlp0[0]))
    active = torch.cat((torch.full((f,), mt != "MLP"), torch.full((mlp0.shape[1],), mt != "GMF")))
    np.testing.assert_allclose(grad[0].cpu().numpy(), (wd * p0 * active).numpy(), rtol=1e-6, atol=0)
    if wd == 0.0:
        assert torch.equal(got.gmf[0].cpu(), gmf0[0]) and torch.equal(got.mlp[0].cpu(), mlp0[0])
        assert not got.state.exp_avg[0].any() and not got.state.exp_avg_sq[0].any()


def _adam_case():
    m = C.make_model("NeuMF-end", 16, 3, U, I, seed=3, device=DEV)
    rng = np.random.default_rng(21)
    counts = [0, 1, 17, 64, 130, 300]
    gmf0, mlp0 = _start(m, len(counts), 5)
    ex = C.make_examples(counts, I, rng)
    g = torch.Generator().manual_seed(6)
    from ncf_amd import ops
    state = ops.FoldState(torch.randn((len(counts), 80), generator=g) * 1e-2,
                          torch.rand((len(counts), 80), generator=g) * 1e-3, 7)
    return m, ex, gmf0, mlp0, state


@pytest.mark.parametrize("generic", [False, True])
def test_adam_is_the_librarys_dense_adam(generic):
    import ncf_amd._lib as L
    from ncf_amd import ops
    m, ex, gmf0, mlp0, state = _adam_case()
    lr, betas, eps = 0.03, (0.85, 0.995), 1e-7
    got, grad = _fold(m, ex, gmf0, mlp0, 1, lr=lr, betas=betas, eps=eps, wd=0.01, state=state, grad=True,
                      generic=generic)
    assert got.state.step == 8
    # ncf_adam_step on the same flat arrays: step t = 8 from (p, g, m, v)
    p = torch.cat((gmf0, mlp0), 1).reshape(-1).to(DEV).contiguous()
    mm = state.exp_avg.reshape(-1).to(DEV).contiguous()
    vv = state.exp_avg_sq.reshape(-1).to(DEV).contiguous()
    g = grad.reshape(-1).clone()
    ctl = ops.new_ctl(1, torch.device(DEV), batch=1, adam_t=8)
    ranges = (ctypes.c_int64 * 2)(0, p.numel())
    L.check(L.hip().ncf_adam_step(p.data_ptr(), g.data_ptr(), mm.data_ptr(), vv.data_ptr(), ranges, 1, ctl.data_ptr(),
                                  lr, betas[0], betas[1], eps, -1, None, 0, L.stream_ptr(torch.device(DEV))),
            "ncf_adam_step")
    torch.cuda.synchronize()
    assert torch.equal(torch.cat((got.gmf, got.mlp), 1).reshape(-1), p)
    assert torch.equal(got.state.exp_avg.reshape(-1), mm) and torch.equal(got.state.exp_avg_sq.reshape(-1), vv)
    # torch.optim.Adam on the CPU from the same gradient (weight decay already inside it)
    tp = torch.cat((gmf0, mlp0), 1).clone().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=eps)
    opt.state[tp] = {"step": torch.tensor(7.0), "exp_avg": state.exp_avg.clone(), "exp_avg_sq": state.exp_avg_sq.clone()}
    tp.grad = grad.cpu().clone()
    opt.step()
    np.testing.assert_allclose(torch.cat((got.gmf, got.mlp), 1).cpu().numpy(), tp.detach().numpy(), rtol=1e-5,
                               atol=5e-3 * lr)
    np.testing.assert_allclose(got.state.exp_avg.cpu().numpy(), opt.state[tp]["exp_avg"].numpy(), rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(got.state.exp_avg_sq.cpu().numpy(), opt.state[tp]["exp_avg_sq"].numpy(), rtol=1e-5,
                               atol=1e-12)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("mt,f,nl", [("NeuMF-end", 16, 3), ("GMF", 8, 1), ("MLP", 8, 2)])
def test_loop_is_the_composition_of_its_steps(mt, f, nl, generic):
    m, ex, gmf0, mlp0, state = _adam_case()
    if (mt, f, nl) != ("NeuMF-end", 16, 3):
        m = C.make_model(mt, f, nl, U, I, seed=3, device=DEV)
        gmf0, mlp0 = _start(m, 6, 5)
        state = None
    one = _fold(m, ex, gmf0, mlp0, 5, lr=0.05, wd=0.001, state=state, generic=generic)
    cur_g, cur_m, cur_s, losses = gmf0, mlp0, state, []
    for _ in range(5):
        step = _fold(m, ex, cur_g, cur_m, 1, lr=0.05, wd=0.001, state=cur_s, generic=generic)
        cur_g, cur_m, cur_s = step.gmf, step.mlp, step.state
        losses.append(step.loss)
    assert cur_s.step == one.state.step == (12 if state is not None else 5)
    assert torch.equal(one.gmf, cur_g) and torch.equal(one.mlp, cur_m)
    assert torch.equal(one.state.exp_avg, cur_s.exp_avg) and torch.equal(one.state.exp_avg_sq, cur_s.exp_avg_sq)
    assert torch.equal(one.loss, torch.cat(losses, 1))


@pytest.mark.parametrize("generic", [False, True])
def test_a_user_does_not_depend_on_the_rest_of_the_call(generic):
    from ncf_amd import ops
    m = C.make_model("NeuMF-end", 16, 3, U, I, seed=3, device=DEV)
    rng = np.random.default_rng(31)
    n_users, probe_n = 300, 117
    counts = rng.integers(0, 60, n_users)
    positions = [0, 150, 299, 77]  # first, middle, last, and a duplicate elsewhere
    counts[positions] = probe_n
    ex = C.make_examples(counts, I, rng)
    gmf0, mlp0 = _start(m, n_users, 8)
    items, labels = ex.items.clone(), ex.labels.clone()
    p0 = int(ex.ptr[positions[0]])
    for pos in positions[1:]:
        a = int(ex.ptr[pos])
        items[a:a + probe_n] = items[p0:p0 + probe_n]
        labels[a:a + probe_n] = labels[p0:p0 + probe_n]
        gmf0[pos], mlp0[pos] = gmf0[positions[0]], mlp0[positions[0]]
    ex = ops.FoldExamples(ex.ptr, items, labels)
    many = _fold(m, ex, gmf0, mlp0, 4, lr=0.05, generic=generic)
    alone_ex = ops.FoldExamples(torch.tensor([0, probe_n]), items[p0:p0 + probe_n], labels[p0:p0 + probe_n])
    alone = _fold(m, alone_ex, gmf0[:1], mlp0[:1], 4, lr=0.05, generic=generic)
    for pos in positions:
        assert torch.equal(many.gmf[pos], alone.gmf[0]) and torch.equal(many.mlp[pos], alone.mlp[0])
        assert torch.equal(many.loss[pos], alone.loss[0])
        assert torch.equal(many.state.exp_avg[pos], alone.state.exp_avg[0])
        assert torch.equal(many.state.exp_avg_sq[pos], alone.state.exp_avg_sq[0])
    again = _fold(m, ex, gmf0, mlp0, 4, lr=0.05, generic=generic)
    assert torch.equal(again.gmf, many.gmf) and torch.equal(again.mlp, many.mlp) and torch.equal(again.loss, many.loss)


def test_position_does_not_matter_beyond_the_ordered_call_size():
    """Calls of more than 16,384 users are not ordered longest first: the same bits."""
    from ncf_amd import ops
    m = C.make_model("NeuMF-end", 8, 2, U, I, seed=3, device=DEV)
    rng = np.random.default_rng(61)
    n_users = 16385
    counts = rng.integers(0, 4, n_users)
    counts[[0, 9000, n_users - 1]] = 40
    ex = C.make_examples(counts, I, rng)
    gmf0, mlp0 = _start(m, n_users, 4)
    big = _fold(m, ex, gmf0, mlp0, 3, lr=0.05)
    keep = torch.arange(0, n_users, 3)  # a third of the users, in an ordered call
    sub_ptr = torch.cat((torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.as_tensor(counts[keep.numpy()]), 0)))
    pick = torch.cat([torch.arange(int(ex.ptr[u]), int(ex.ptr[u + 1])) for u in keep.tolist()])
    small = _fold(m, ops.FoldExamples(sub_ptr, ex.items[pick], ex.labels[pick]), gmf0[keep], mlp0[keep], 3, lr=0.05)
    assert torch.equal(big.gmf[keep.to(DEV)], small.gmf) and torch.equal(big.mlp[keep.to(DEV)], small.mlp)
    assert torch.equal(big.loss[keep.to(DEV)], small.loss)
    assert small.loss[0, 0] > 0


def _as_ref(got):
    z = torch.zeros(0)
    return C.Ref(got.gmf.detach().cpu().double(), got.mlp.detach().cpu().double(), got.loss.detach().cpu().double(),
                 z, z, z)


@pytest.mark.parametrize("f", [16, 8])
def test_free_running_trajectory(f):
    """At most 5 % of the users may leave the bounds (a ReLU unit within rounding of 0 flips
    and Adam's normalisation carries the flip forward); the fp32 torch CPU run of the same
    inputs must itself be within that cap."""
    m = C.make_model("NeuMF-end", f, 3, U, I, seed=3, device=DEV)
    m64 = C.to64(m)
    rng = np.random.default_rng(41 + f)
    counts = rng.integers(1, 300, 200)
    gmf0, mlp0 = _start(m, 200, 9)
    ex = C.untie(m64, C.make_examples(counts, I, rng), gmf0, mlp0, rng)
    ref = C.ref_fold(m64, ex, gmf0, mlp0, 20, lr=0.05)
    cpu = C.make_model("NeuMF-end", f, 3, U, I, seed=3).fold_in(ex, steps=20, lr=0.05, init=(gmf0, mlp0))
    out = {"cpu fp32": C.check_trajectory(cpu, ref, "torch CPU fp32")}
    fused = _fold(m, ex, gmf0, mlp0, 20, lr=0.05)
    generic = _fold(m, ex, gmf0, mlp0, 20, lr=0.05, generic=True)
    out["fused"] = int(C.trajectory_outside(fused, ref).sum())
    out["generic"] = int(C.trajectory_outside(generic, ref).sum())
    out["fused vs generic"] = int(C.trajectory_outside(generic, _as_ref(fused)).sum())
    print(f"NeuMF-end({f},3): users outside the bounds of 200: {out}")
    C.check_trajectory(fused, ref, "fused")
    C.check_trajectory(generic, ref, "generic")
    C.check_trajectory(generic, _as_ref(fused), "generic against fused")
    assert fused.loss[:, -1].mean() < fused.loss[:, 0].mean()


def test_with_users_serves_rows_like_the_original():
    m = C.make_model("NeuMF-end", 16, 3, U, I, seed=3, device=DEV).eval()
    rows = torch.tensor([7, 0, 49, 7, 23])
    w = m.with_users((m.embed_user_GMF.weight[rows.to(DEV)], m.embed_user_MLP.weight[rows.to(DEV)]))
    assert w.user_num == 5 and w.embed_user_GMF.weight.is_cuda
    items = torch.arange(I, device=DEV)
    with torch.no_grad():
        for q, u in enumerate(rows.tolist()):
            assert torch.equal(w(torch.full((I,), q, device=DEV), items), m(torch.full((I,), u, device=DEV), items))
    a, b = w.recommend(torch.arange(5), 20), m.recommend(rows, 20)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # folded users through recommend and similar_users: the checker of the recommend tests
    rng = np.random.default_rng(4)
    lists = [np.sort(rng.choice(I, n, replace=False)) for n in (3, 40, 120, 1)]
    from ncf_amd import ops
    ex = ops.fold_examples(lists, I, 4, torch.Generator().manual_seed(1))
    folded = m.fold_in(ex, steps=10, lr=0.05)
    served = m.with_users(folded)
    seen = ops.seen_csr(np.concatenate([np.full(len(x), q) for q, x in enumerate(lists)]), np.concatenate(lists), 4,
                        DEV, I)
    S = oracle_scores(served)
    for excl in (None, seen):
        items_k, scores_k = served.recommend(torch.arange(4), 10, excl)
        check_topk(items_k, scores_k, np.arange(4), S, 10, excl)
    ids, _ = served.similar_users([0, 1], 3)
    assert ids.shape == (2, 3)


def _raw_args(m, ex, gmf, mlp, steps):
    from ncf_amd import ops
    flat, lay = ops.ensure_flat(m)
    q, e = ex.ptr.numel() - 1, ex.items.numel()
    opt = ops.fold_opt(steps, 0.01, (0.9, 0.999), 1e-8, 0.0, 0)
    need = ops.L.hip().ncf_fold_in_workspace_bytes(ctypes.byref(lay), q, e, steps)
    ws = torch.empty(max(need, 4) // 4, dtype=torch.float32, device=DEV)
    return flat, lay, opt, need, ws


def test_c_abi_refusals():
    import ncf_amd._lib as L
    from ncf_amd import ops
    m = C.make_model("NeuMF-end", 16, 3, U, I, seed=3, device=DEV)
    ex = C.make_examples([5, 20], I, np.random.default_rng(0))
    ex = ops.FoldExamples(ex.ptr.to(DEV), ex.items.to(DEV), ex.labels.to(DEV))
    gmf0, mlp0 = _start(m, 2, 1)
    gmf, mlp = gmf0.to(DEV), mlp0.to(DEV)
    st_m, st_v = torch.zeros((2, 80), device=DEV), torch.zeros((2, 80), device=DEV)
    flat, lay, opt, need, ws = _raw_args(m, ex, gmf, mlp, 3)
    lib = L.hip()
    stream = L.stream_ptr(torch.device(DEV))

    def call(lay_=lay, params=flat.data_ptr(), ptr=ex.ptr.data_ptr(), items=ex.items.data_ptr(),
             labels=ex.labels.data_ptr(), q=2, e=25, ug=gmf.data_ptr(), um=mlp.data_ptr(), ea=st_m.data_ptr(),
             eas=st_v.data_ptr(), opt_=opt, ws_=ws.data_ptr(), wsb=need):
        return lib.ncf_fold_in(None if lay_ is None else ctypes.byref(lay_), params, ptr, items, labels, q, e, ug, um,
                               ea, eas, None if opt_ is None else ctypes.byref(opt_), None, None, ws_, wsb, stream)

    for name in ("lay_", "params", "ptr", "items", "labels", "ug", "um", "opt_", "ws_"):
        assert call(**{name: None}) == L.NCF_E_ARG, name
    assert call(ea=None) == L.NCF_E_ARG and call(eas=None) == L.NCF_E_ARG  # only one of the two state pointers
    assert call(q=-1) == L.NCF_E_ARG and call(e=-1) == L.NCF_E_ARG
    assert call(opt_=ops.fold_opt(0, 0.01, (0.9, 0.999), 1e-8, 0.0, 0)) == L.NCF_E_ARG
    assert call(opt_=ops.fold_opt(3, 0.01, (0.9, 0.999), 1e-8, 0.0, -1)) == L.NCF_E_ARG
    assert call(wsb=need - 1) == L.NCF_E_ARG
    torch.cuda.synchronize()
    assert torch.equal(gmf.cpu(), gmf0) and torch.equal(mlp.cpu(), mlp0)  # a refused call launches nothing
    # n_users == 0: NCF_OK, nothing launched -- the outputs keep their sentinel
    sent_g, sent_m = torch.full((2, 16), 7.0, device=DEV), torch.full((2, 64), 7.0, device=DEV)
    loss = torch.full((2, 3), 7.0, device=DEV)
    rc = lib.ncf_fold_in(ctypes.byref(lay), flat.data_ptr(), ex.ptr.data_ptr(), None, None, 0, 0, sent_g.data_ptr(),
                         sent_m.data_ptr(), None, None, ctypes.byref(opt), loss.data_ptr(), None, None, 0, stream)
    torch.cuda.synchronize()
    assert rc == L.NCF_OK and (sent_g == 7).all() and (sent_m == 7).all() and (loss == 7).all()
    assert lib.ncf_fold_in_workspace_bytes(ctypes.byref(lay), 0, 0, 3) == 0
    for bad in ((-1, 0, 3), (2, -1, 3), (2, 25, 0)):
        assert lib.ncf_fold_in_workspace_bytes(ctypes.byref(lay), *bad) == -1
    assert lib.ncf_debug_set_fold_path(3) == L.NCF_E_ARG
    # workspace_bytes is exact: a buffer of exactly that size, guarded on both sides
    pad = 1024
    buf = torch.full((need // 4 + 2 * pad,), 3.0, dtype=torch.float32, device=DEV)
    assert call(ws_=buf.data_ptr() + 4 * pad, wsb=need) == L.NCF_OK
    torch.cuda.synchronize()
    assert (buf[:pad] == 3).all() and (buf[-pad:] == 3).all()
    want = _fold(m, ex, gmf0, mlp0, 3)
    assert torch.equal(gmf, want.gmf) and torch.equal(mlp, want.mlp)


def test_python_argument_errors():
    from ncf_amd import ops
    m = C.make_model("NeuMF-end", 16, 3, U, I, seed=3, device=DEV)
    ex = C.make_examples([5, 20], I, np.random.default_rng(0))
    with pytest.raises(ValueError):
        m.fold_in(ex, steps=0)
    with pytest.raises(ValueError):
        m.fold_in(ex, init="median")
    bad = ex.items.clone()
    bad[7] = I
    with pytest.raises(IndexError):
        m.fold_in(ops.FoldExamples(ex.ptr, bad, ex.labels))
    bad[7] = -1
    with pytest.raises(IndexError):
        m.fold_in(ops.FoldExamples(ex.ptr, bad, ex.labels))
    lab = ex.labels.clone()
    lab[3] = -0.25
    with pytest.raises(ValueError):
        m.fold_in(ops.FoldExamples(ex.ptr, ex.items, lab))
    out = m.fold_in(ops.FoldExamples(torch.zeros(1, dtype=torch.int64), ex.items[:0], ex.labels[:0]))  # no users
    assert out.gmf.shape == (0, 16) and out.mlp.shape == (0, 64) and out.loss.shape == (0, 50)


@pytest.mark.parametrize("generic", [False, True])
def test_fold_in_captured_in_a_graph(generic):
    from ncf_amd import ops
    m = C.make_model("NeuMF-end", 16, 3, U, I, seed=3, device=DEV)
    ex = C.make_examples([0, 3, 40, 130], I, np.random.default_rng(2))
    ex = ops.FoldExamples(ex.ptr.to(DEV), ex.items.to(DEV), ex.labels.to(DEV))
    gmf0, mlp0 = _start(m, 4, 3)
    with _path(generic):
        flat, lay, opt, need, ws = _raw_args(m, ex, gmf0, mlp0, 3)
        opt = ops.fold_opt(3, 0.05, (0.9, 0.999), 1e-8, 0.0, 0)

        def fresh():
            return (gmf0.to(DEV), mlp0.to(DEV), torch.zeros((4, 80), device=DEV), torch.zeros((4, 80), device=DEV),
                    torch.zeros((4, 3), device=DEV))
        eager = fresh()
        for _ in range(2):  # also the one-time kernel attribute call
            ops.fold_in_into(flat, lay, ex, eager[0], eager[1], eager[2], eager[3], opt, eager[4], None, ws)
        torch.cuda.synchronize()
        cap = fresh()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):  # one linear capture
            ops.fold_in_into(flat, lay, ex, cap[0], cap[1], cap[2], cap[3], opt, cap[4], None, ws)
        for dst, src in zip(cap, fresh()):
            dst.copy_(src)
        g.replay()
        g.replay()
        torch.cuda.synchronize()
    for a, b in zip(cap, eager):
        assert torch.equal(a, b)
    assert not torch.equal(cap[0], gmf0.to(DEV))


@pytest.mark.parametrize("mt,f,nl", [("GMF", 8, 1), ("MLP", 8, 2), ("NeuMF-end", 16, 3)])
def test_backends_pass_the_same_check(mt, f, nl):
    hip = C.make_model(mt, f, nl, U, I, seed=3, device=DEV)
    cpu = C.make_model(mt, f, nl, U, I, seed=3)
    m64 = C.to64(cpu)
    rng = np.random.default_rng(51)
    counts = [0, 9, 16, 75, 210]
    gmf0, mlp0 = _start(cpu, len(counts), 2)
    ex = C.untie(m64, C.make_examples(counts, I, rng, soft=True), gmf0, mlp0, rng)
    ref1 = C.ref_fold(m64, ex, gmf0, mlp0, 1, lr=0.02, weight_decay=0.01)
    ref8 = C.ref_fold(m64, ex, gmf0, mlp0, 8, lr=0.02, weight_decay=0.01)
    for name, model in (("cpu", cpu), ("hip", hip)):
        one = model.fold_in(ex, steps=1, lr=0.02, weight_decay=0.01, init=(gmf0, mlp0))
        assert one.gmf.device.type == ("cuda" if name == "hip" else "cpu")
        C.close_loss(one.loss[:, 0].cpu().numpy(), ref1.loss[:, 0].numpy(), f"{name}: loss")
        for k, got, want in (("gmf", one.gmf, ref1.gmf), ("mlp", one.mlp, ref1.mlp)):
            np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-5, atol=5e-3 * 0.02, err_msg=f"{name} {k}")
        C.check_trajectory(model.fold_in(ex, steps=8, lr=0.02, weight_decay=0.01, init=(gmf0, mlp0)), ref8, name)
