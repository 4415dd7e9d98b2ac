"""Pairwise (BPR) training, host side: the ABI, ``bpr_loss``, the pair stream in NumPy,
its validation, and the host epoch path's use of the two generators.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import bpr_checks as C
from oracle import ncf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_21_and_exports():
    import ncf_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "ncf_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    want = int(re.search(r"#define NCF_ABI_VERSION (\d+)", hdr).group(1))
    assert want == 21 == L.ABI_VERSION == L.hip().ncf_abi_version()
    assert int(re.search(r"ncf_abi_version\(\) == (\d+)", doc).group(1)) == want
    assert int(re.search(r"#define NCF_DZ_BPR (\d+)", hdr).group(1)) == 3 == L.DZ_BPR
    assert hasattr(L.hip(), "ncf_build_pair_stream")
    assert "ncf_build_pair_stream" in L._HIP_PROTOS


def test_bpr_loss_value_and_gradients_vs_float64_closed_form():
    from ncf_amd.losses import bpr_loss
    rng = np.random.default_rng(0)
    zp = np.concatenate([rng.normal(0, 3, 200), [40.0, -40.0, 0.0, 1e-4]]).astype(np.float32)
    zn = np.concatenate([rng.normal(0, 3, 200), [-40.0, 40.0, 0.0, -1e-4]]).astype(np.float32)
    d = zp.astype(np.float64) - zn.astype(np.float64)
    want = np.mean(np.logaddexp(0.0, -d))         # softplus(-d)
    gpos = -(1.0 / (1.0 + np.exp(d))) / len(d)    # (sigmoid(d) - 1) / T
    a = torch.tensor(zp, requires_grad=True)
    b = torch.tensor(zn, requires_grad=True)
    loss = bpr_loss(a, b)
    loss.backward()
    np.testing.assert_allclose(loss.item(), want, rtol=1e-6)
    np.testing.assert_allclose(a.grad.numpy(), gpos, rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(b.grad.numpy(), -gpos, rtol=1e-5, atol=1e-12)
    with pytest.raises(ValueError):
        bpr_loss(torch.zeros(3), torch.zeros(4))


def test_bpr_stream_host_hand_written():
    from ncf_amd import ops
    pu, pi = [7, 7, 9], [1, 2, 3]
    neg = [10, 11, 12, 13, 14, 15]  # positive p's negatives at [2p, 2p + 2)
    R = lambda u, i, y: (u & 0xFFFFFFFF) | (i << 32) | ((-(1 << 63)) if y else 0)  # noqa: E731
    want = [R(7, 1, 1), R(7, 10, 0), R(7, 1, 1), R(7, 11, 0), R(7, 2, 1), R(7, 12, 0),
            R(7, 2, 1), R(7, 13, 0), R(9, 3, 1), R(9, 14, 0), R(9, 3, 1), R(9, 15, 0)]
    got = ops.bpr_stream_host(pu, pi, neg, 2)
    assert got.dtype == np.int64 and got.tolist() == want
    perm = [5, 0, 3, 2, 4, 1]
    wantp = []
    for t in perm:
        wantp += [R(pu[t // 2], pi[t // 2], 1), R(pu[t // 2], neg[t], 0)]
    assert ops.bpr_stream_host(pu, pi, neg, 2, perm).tolist() == wantp
    ops.check_pair_rows(got, 10, 16)  # a valid stream passes
    with pytest.raises(ValueError):
        ops.bpr_stream_host(pu, pi, neg, 2, perm[:5])


def test_check_pair_rows_rejections():
    from ncf_amd import ops
    ok = ops.bpr_stream_host([3, 4], [5, 6], [7, 8], 1)
    ops.check_pair_rows(ok, 5, 9)
    pad = ops.pack_rows_host([-1, -1], [0, 0])
    ops.check_pair_rows(np.concatenate([ok, pad]), 5, 9)  # a padding pair is allowed
    with pytest.raises(ValueError, match="odd"):
        ops.check_pair_rows(ok[:3], 5, 9)
    bad = ok.copy()
    bad[1] = ops.pack_rows_host([3], [7], [1])[0]  # labels (1, 1)
    with pytest.raises(ValueError, match="labels"):
        ops.check_pair_rows(bad, 5, 9)
    bad = ok.copy()
    bad[0] = ops.pack_rows_host([3], [5], [0])[0]  # labels (0, 0)
    with pytest.raises(ValueError, match="labels"):
        ops.check_pair_rows(bad, 5, 9)
    bad = ok.copy()
    bad[3] = ops.pack_rows_host([2], [8], [0])[0]  # users (4, 2)
    with pytest.raises(ValueError, match="users"):
        ops.check_pair_rows(bad, 5, 9)
    bad = ok.copy()
    bad[2] = ops.pack_rows_host([-1], [0], [1])[0]  # half a padding pair
    with pytest.raises(ValueError, match="users"):
        ops.check_pair_rows(bad, 5, 9)
    with pytest.raises(IndexError):
        ops.check_pair_rows(ok, 4, 9)  # user 4 out of range
    with pytest.raises(IndexError):
        ops.check_pair_rows(ok, 5, 8)  # item 8 out of range


def _dataset(seed=5, U=40, I=60, P=300, ng=3):
    from ncf_amd.data import NCFData
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, U, P), rng.integers(0, I, P)], 1), axis=0)
    return lambda: NCFData(pairs, I, None, ng, True), pairs, ng


@pytest.mark.parametrize("seed", [0, 123])
def test_host_epoch_negatives_order_and_generators(seed):
    """bpr_host_epoch: the negatives are ng_sample()'s, the triple order is
    epoch_permutation(S), and both generators end where a reference epoch
    (ng_sample + one DataLoader(shuffle=True) pass) leaves them."""
    from ncf_amd import ops
    from ncf_amd.data import epoch_permutation
    from ncf_amd.trainer import bpr_host_epoch
    mk, pairs, ng = _dataset()
    P, S = len(pairs), len(pairs) * ng

    np.random.seed(seed)
    torch.manual_seed(seed)
    got = bpr_host_epoch(mk())
    end_np, end_t = np.random.get_state(), torch.get_rng_state()

    np.random.seed(seed)
    torch.manual_seed(seed)
    ds = mk()
    ds.ng_sample()
    neg = np.asarray(ds.arrays()[1][P:])
    perm = epoch_permutation(S).numpy()
    ref_np, ref_t = np.random.get_state(), torch.get_rng_state()

    assert got.shape == (2 * S,)
    u, it, y = C.unpack_rows(got)
    assert np.array_equal(y, np.tile([1, 0], S))
    assert np.array_equal(it[1::2], neg[perm])                       # the negatives, in triple order
    assert np.array_equal(it[0::2], pairs[perm // ng, 1])
    assert np.array_equal(u[0::2], pairs[perm // ng, 0]) and np.array_equal(u[0::2], u[1::2])
    assert np.array_equal(got, ops.bpr_stream_host(pairs[:, 0], pairs[:, 1], neg, ng, perm))
    # the oracle's restatement of the sampler and of the DataLoader protocol agree
    assert np.array_equal(neg, O.ng_sample_py(pairs[:, 0], pairs[:, 1], 60, ng, seed))
    torch.manual_seed(seed)
    assert np.array_equal(perm, O.epoch_order(S))
    # generators: where ng_sample + a DataLoader(shuffle=True) epoch leave them
    assert end_np[0] == ref_np[0] and np.array_equal(end_np[1], ref_np[1]) and end_np[2:] == ref_np[2:]
    assert torch.equal(end_t, ref_t)
    assert torch.equal(torch.get_rng_state(), ref_t)  # (epoch_order above made the same two draws)


def test_trainer_and_engine_refuse_on_cpu_arguments():
    """Argument checks that need no device."""
    from ncf_amd import ops
    with pytest.raises(ValueError):
        ops.bpr_stream_host([1, 2], [3], [4, 5], 1)
