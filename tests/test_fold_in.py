"""CPU tests of fold-in: NCF.fold_in on a CPU model (stock torch autograd and
torch.optim.Adam) against the float64 reference of tests/fold_in_checks.py, fold_examples,
NCF.with_users, scripts/fold_in.py, and the header's declarations against ncf_amd._lib."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fold_in_checks as C  # noqa: E402

U, I = 40, 203
COUNTS = [0, 1, 15, 16, 17, 63, 64, 65, 200]
SHAPES = [("GMF", 5, 1), ("MLP", 6, 2), ("NeuMF-end", 8, 3), ("NeuMF-pre", 16, 3)]


def _start(m, q, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((q, m.embed_user_GMF.weight.shape[1]), generator=g) * 0.5,
            torch.randn((q, m.embed_user_MLP.weight.shape[1]), generator=g) * 0.5)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("mt,f,nl", SHAPES)
def test_cpu_fold_in_matches_float64(mt, f, nl, wd):
    m = C.make_model(mt, f, nl, U, I, seed=3)
    m64 = C.to64(m)
    rng = np.random.default_rng(7)
    gmf0, mlp0 = _start(m, len(COUNTS), 11)
    ex = C.untie(m64, C.make_examples(COUNTS, I, rng, soft=(mt == "MLP")), gmf0, mlp0, rng)
    lr = 0.05
    # one step from a general point: loss, and the step the gradient gives
    got = m.fold_in(ex, steps=1, lr=lr, weight_decay=wd, init=(gmf0, mlp0))
    ref = C.ref_fold(m64, ex, gmf0, mlp0, 1, lr=lr, weight_decay=wd)
    C.close_loss(got.loss[:, 0].numpy(), ref.loss[:, 0].numpy(), "loss")
    assert got.loss[0, 0] == 0  # the empty user
    for k, g, r, s in (("gmf", got.gmf, ref.gmf, gmf0), ("mlp", got.mlp, ref.mlp, mlp0)):
        if (mt, k) in (("MLP", "gmf"), ("GMF", "mlp")):
            assert torch.equal(g, s), f"the untrained {k} half moved"
        else:
            np.testing.assert_allclose(g.numpy(), r.numpy(), rtol=1e-5, atol=5e-3 * lr, err_msg=k)
    if wd == 0.0:
        assert torch.equal(got.gmf[0], gmf0[0]) and torch.equal(got.mlp[0], mlp0[0])
    # a trajectory, continued from the returned state: the composition of its parts
    a = m.fold_in(ex, steps=6, lr=lr, weight_decay=wd, init=(gmf0, mlp0))
    b1 = m.fold_in(ex, steps=2, lr=lr, weight_decay=wd, init=(gmf0, mlp0))
    b2 = m.fold_in(ex, steps=4, lr=lr, weight_decay=wd, init=(b1.gmf, b1.mlp), state=b1.state)
    assert a.state.step == b2.state.step == 6
    assert torch.equal(a.gmf, b2.gmf) and torch.equal(a.mlp, b2.mlp)
    assert torch.equal(a.loss, torch.cat((b1.loss, b2.loss), 1))
    assert torch.equal(a.state.exp_avg, b2.state.exp_avg) and torch.equal(a.state.exp_avg_sq, b2.state.exp_avg_sq)
    ref6 = C.ref_fold(m64, ex, gmf0, mlp0, 6, lr=lr, weight_decay=wd)
    C.check_trajectory(a, ref6, f"{mt} cpu")
    assert a.loss[1:, -1].mean() < a.loss[1:, 0].mean()  # the fit lowers the loss


def test_init_modes_and_argument_errors():
    m = C.make_model("NeuMF-end", 8, 2, U, I, seed=5)
    rng = np.random.default_rng(1)
    ex = C.make_examples([5, 0, 9], I, rng)
    zero = m.fold_in(ex, steps=1, init="zeros")
    mean = m.fold_in(ex, steps=1, init="mean")
    # the empty user stays at its start: that is the init
    assert torch.equal(zero.gmf[1], torch.zeros(8)) and torch.equal(zero.mlp[1], torch.zeros(16))
    assert torch.equal(mean.gmf[1], m.embed_user_GMF.weight.detach().mean(0))
    assert torch.equal(mean.mlp[1], m.embed_user_MLP.weight.detach().mean(0))
    pair = (torch.ones(3, 8), torch.full((3, 16), 0.25))
    got = m.fold_in(ex, steps=1, init=pair)
    assert torch.equal(got.gmf[1], pair[0][1]) and not torch.equal(got.gmf[0], pair[0][0])
    assert got.gmf.shape == (3, 8) and got.mlp.shape == (3, 16) and got.loss.shape == (3, 1)
    assert not any(p.grad is not None for p in m.parameters())  # the model itself is frozen and untouched
    from ncf_amd import ops
    with pytest.raises(ValueError):
        m.fold_in(ex, steps=0)
    with pytest.raises(ValueError):
        m.fold_in(ex, steps=1.5)
    with pytest.raises(ValueError):
        m.fold_in(ex, init="median")
    with pytest.raises(ValueError):
        m.fold_in(ex, init=(torch.ones(2, 8), torch.ones(2, 16)))
    bad = ex.items.clone()
    bad[3] = I
    with pytest.raises(IndexError):
        m.fold_in(ops.FoldExamples(ex.ptr, bad, ex.labels))
    lab = ex.labels.clone()
    lab[0] = 1.5
    with pytest.raises(ValueError):
        m.fold_in(ops.FoldExamples(ex.ptr, ex.items, lab))
    with pytest.raises(ValueError):
        m.fold_in(ops.FoldExamples(ex.ptr[:-1], ex.items, ex.labels))


def test_fold_examples():
    from ncf_amd import ops
    rng = np.random.default_rng(3)
    lists = [np.sort(rng.choice(I, n, replace=False)) for n in (7, 0, 150, 1, I - 1)]
    g = torch.Generator().manual_seed(9)
    ex = ops.fold_examples(lists, I, num_ng=4, generator=g)
    assert ex.ptr.dtype == torch.int64 and ex.items.dtype == torch.int32 and ex.labels.dtype == torch.float32
    assert ex.ptr.tolist() == np.concatenate([[0], np.cumsum([5 * len(x) for x in lists])]).tolist()
    for q, h in enumerate(lists):
        lo, hi = int(ex.ptr[q]), int(ex.ptr[q + 1])
        items, labels = ex.items[lo:hi].numpy(), ex.labels[lo:hi].numpy()
        n = len(h)
        assert np.array_equal(items[:n], h) and (labels[:n] == 1).all() and (labels[n:] == 0).all()
        assert not np.isin(items[n:], h).any() and (items >= 0).all() and (items < I).all()
    assert (ex.items[int(ex.ptr[4]) + I - 1:] == np.setdiff1d(np.arange(I), lists[4])[0]).all()  # the one free item
    neg = ex.items[int(ex.ptr[2]) + 150:int(ex.ptr[3])].numpy()
    assert len(np.unique(neg)) > 40  # spread over the 53 free items, not stuck on a few
    # the same seed, the same output; another seed, other negatives
    again = ops.fold_examples(lists, I, 4, torch.Generator().manual_seed(9))
    other = ops.fold_examples(lists, I, 4, torch.Generator().manual_seed(10))
    assert all(torch.equal(a, b) for a, b in zip(ex, again)) and not torch.equal(ex.items, other.items)
    # the three input forms agree
    users = np.concatenate([np.full(len(x), q) for q, x in enumerate(lists)])
    flat = np.concatenate(lists)
    mixed_u = users[rng.permutation(len(users))]  # users interleaved, each user's items in its own order
    mixed_i = np.empty_like(flat)
    for q, h in enumerate(lists):
        mixed_i[mixed_u == q] = h
    pair = ops.fold_examples((mixed_u, mixed_i), I, 4, torch.Generator().manual_seed(9))
    csr = ops.fold_examples(ops.seen_csr(users, flat, len(lists), None, I), I, 4, torch.Generator().manual_seed(9))
    for form in (pair, csr):
        assert all(torch.equal(a, b) for a, b in zip(ex, form))
    assert ops.fold_examples(lists, I, 0).items.numel() == sum(len(x) for x in lists)
    with pytest.raises(ValueError):
        ops.fold_examples([np.arange(I)], I)
    with pytest.raises(IndexError):
        ops.fold_examples([[0, I]], I)


@pytest.mark.parametrize("mt", ["GMF", "NeuMF-end"])
def test_with_users_cpu(mt):
    m = C.make_model(mt, 8, 2, U, I, seed=2).eval()
    rows = torch.tensor([7, 0, 39, 7])
    state = torch.get_rng_state()
    w = m.with_users((m.embed_user_GMF.weight[rows], m.embed_user_MLP.weight[rows]))
    assert torch.equal(torch.get_rng_state(), state)  # building the copy draws nothing from the global stream
    assert w.user_num == 4 and w.item_num == I and w.model_type == mt and not w.training
    items = torch.arange(I)
    for q, u in enumerate(rows.tolist()):
        assert torch.equal(w(torch.full((I,), q), items), m(torch.full((I,), u), items))
    a, b = w.recommend(torch.arange(4), 10), m.recommend(rows, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with torch.no_grad():
        w.predict_layer.bias += 1.0  # a copy: the original is not touched
    assert not torch.equal(w.predict_layer.bias, m.predict_layer.bias)
    folded = m.fold_in(C.make_examples([12, 30], I, np.random.default_rng(0)), steps=3)
    served = m.with_users(folded)
    assert torch.equal(served.embed_user_GMF.weight, folded.gmf) and torch.equal(served.embed_user_MLP.weight, folded.mlp)
    with pytest.raises(ValueError):
        m.with_users((torch.zeros(2, 8), torch.zeros(3, 16)))


def test_fold_in_script_cpu(tmp_path):
    from ncf_amd import ops
    m = C.make_model("NeuMF-end", 8, 2, U, I, seed=6).eval()
    ckpt = tmp_path / "m.pth"
    torch.save(m.state_dict(), ckpt)
    lists = {"carol": [5, 17, 200, 3], "alice": [9], "bob": [100, 101, 102, 0, 77, 5]}
    order = ["carol", "bob", "alice"]  # first appearance below
    lines = ["carol\t5", "bob\t100", "carol\t17", "alice\t9", "bob\t101", "bob\t102", "carol\t200", "bob\t0", "bob\t77",
             "carol\t3", "bob\t5"]
    inter = tmp_path / "new.tsv"
    inter.write_text("\n".join(lines) + "\n")
    out = tmp_path / "folded.npz"
    env = dict(os.environ, PYTHONPATH=ROOT)
    script = os.path.join(ROOT, "scripts", "fold_in.py")
    done = subprocess.run([sys.executable, script, "--checkpoint", str(ckpt), "--model", "NeuMF-end", "--interactions",
                           str(inter), "--num_ng", "3", "--steps", "8", "--lr", "0.02", "--seed", "4", "--top_k", "6",
                           "--out", str(out), "--device", "cpu"], check=True, cwd=tmp_path, env=env,
                          capture_output=True, text=True)
    assert len(done.stdout.strip().splitlines()) == 1 and "top-6" in done.stdout and "folded 3 users" in done.stdout
    z = np.load(out)
    assert z["users"].tolist() == order
    hist = [np.asarray(lists[k]) for k in order]
    ex = ops.fold_examples(hist, I, 3, torch.Generator().manual_seed(4))
    want = m.fold_in(ex, steps=8, lr=0.02)
    np.testing.assert_array_equal(z["gmf"], want.gmf.numpy())
    np.testing.assert_array_equal(z["mlp"], want.mlp.numpy())
    np.testing.assert_array_equal(z["loss"], want.loss.numpy())
    seen_u = np.concatenate([np.full(len(h), q) for q, h in enumerate(hist)])
    items, scores = m.with_users(want).recommend(torch.arange(3), 6, (seen_u, np.concatenate(hist)))
    np.testing.assert_array_equal(z["items"], items.numpy())
    np.testing.assert_array_equal(z["scores"], scores.numpy())
    for q, h in enumerate(hist):
        assert not np.isin(z["items"][q], h).any()


def test_header_declares_what_lib_carries():
    import ctypes
    import ncf_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "ncf_hip.h")).read()
    assert int(re.search(r"#define NCF_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == 21
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int64_t\s+ncf_fold_in_workspace_bytes\s*\(", code)
    assert re.search(r"\bint\s+ncf_fold_in\s*\(", code)
    assert re.search(r"\bint\s+ncf_debug_set_fold_path\s*\(", code)
    for name, nargs in (("ncf_fold_in_workspace_bytes", 4), ("ncf_fold_in", 17), ("ncf_debug_set_fold_path", 1)):
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", code).group(1)
        assert len(proto.split(",")) == nargs == len(L._HIP_PROTOS[name][1])
        assert hasattr(L.hip(), name)
    body = re.search(r"typedef struct ncf_fold_opt \{(.*?)\} ncf_fold_opt;", code, flags=re.S).group(1)
    fields = [(t, n.strip()) for t, names in re.findall(r"(double|float|int32_t|int64_t)\s+([^;]+);", body)
              for n in names.split(",")]
    ctype = {"double": ctypes.c_double, "float": ctypes.c_float, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    assert [(n, ctype[t]) for t, n in fields] == list(L.NcfFoldOpt._fields_)
    assert ctypes.sizeof(L.NcfFoldOpt) == 48
