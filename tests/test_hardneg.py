"""Dynamic negative sampling, host side: NCF.hardest_negatives on a CPU model against the
oracle (tests/hardneg_checks.py), the host epoch with a select function, and the argument
checks.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import bpr_checks as C
import hardneg_checks as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, I = 50, 80


def test_abi_exports_and_docs():
    import ncf_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "ncf_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"#define NCF_ABI_VERSION (\d+)", hdr).group(1)) == 21 == L.ABI_VERSION
    for name in ("ncf_select_negatives_workspace_bytes", "ncf_select_negatives", "ncf_debug_set_select_path"):
        assert name in hdr and name in L._HIP_PROTOS and hasattr(L.hip(), name), name
    assert "ncf_select_negatives" in doc


@pytest.mark.parametrize("mt,f,Lyr", [("NeuMF-end", 8, 3), ("MLP", 16, 2), ("GMF", 16, 1)])
@pytest.mark.parametrize("m", [1, 5, 16, 40])
def test_cpu_hardest_negatives_vs_oracle(mt, f, Lyr, m):
    from ncf_amd import ops
    ref, model = C.models(mt, f, Lyr, U, I, 11)
    users, cand = H.draw(1000, m, U, I)
    S = H.oracle_scores(ref, users, cand)
    model.train()  # dropout never applies, whatever the mode
    r = model.hardest_negatives(torch.as_tensor(users), torch.as_tensor(cand))
    assert isinstance(r, ops.HardNegatives)
    assert r.items.dtype == torch.int64 and r.slots.dtype == torch.int64 and r.scores.dtype == torch.float32
    assert r.items.shape == r.slots.shape == r.scores.shape == (1000,)
    H.check_selection(S, cand, r.items.numpy(), r.slots.numpy(), r.scores.numpy(), f"cpu {mt}({f},{Lyr}) m={m}")
    # a group's result depends on that group alone
    r17 = model.hardest_negatives(users[:17], cand[:17])
    assert torch.equal(r17.items, r.items[:17]) and torch.equal(r17.slots, r.slots[:17])


@pytest.mark.parametrize("mt,f,Lyr", [("NeuMF-end", 8, 3), ("MLP", 16, 2), ("GMF", 16, 1)])
def test_cpu_duplicates_resolve_to_lowest_slot(mt, f, Lyr):
    ref, model = C.models(mt, f, Lyr, U, I, 11)
    users, cand = H.draw(200, 6, U, I)
    S = H.oracle_scores(ref, users, cand)
    slot, item, decided = H.oracle_choice(S, cand)
    # the oracle's winner copied into two more slots, one of them in front of the original
    rows = np.arange(200)
    cand2 = np.concatenate([item[:, None].astype(np.int32), cand, item[:, None].astype(np.int32)], axis=1)
    r = model.hardest_negatives(users, cand2)
    assert np.array_equal(r.items.numpy()[decided], item[decided])
    assert (r.slots.numpy()[decided] == 0).all()
    # and rows of one repeated id: slot 0
    same = np.repeat(cand[:, :1], 5, axis=1)
    r = model.hardest_negatives(users, same)
    assert (r.slots.numpy() == 0).all() and np.array_equal(r.items.numpy(), same[rows, 0])


def test_hardest_negatives_argument_errors():
    _, model = C.models("NeuMF-end", 8, 3, U, I, 11)
    users, cand = H.draw(10, 4, U, I)
    with pytest.raises(ValueError):
        model.hardest_negatives(users, np.zeros((10, 0), dtype=np.int32))      # m = 0
    with pytest.raises(ValueError):
        model.hardest_negatives(users, np.zeros((10, 65), dtype=np.int32))     # m = 65
    with pytest.raises(ValueError):
        model.hardest_negatives(users, cand[:, 0])                             # candidates not [n, m]
    with pytest.raises(ValueError):
        model.hardest_negatives(users[:9], cand)                               # n differs
    with pytest.raises(ValueError):
        model.hardest_negatives(users.reshape(5, 2), cand)                     # users not [n]
    bad = cand.copy()
    bad[3, 2] = I
    with pytest.raises(IndexError):
        model.hardest_negatives(users, bad)
    bad[3, 2] = -1
    with pytest.raises(IndexError):
        model.hardest_negatives(users, bad)
    with pytest.raises(IndexError):
        model.hardest_negatives(np.full(10, U, dtype=np.int32), cand)
    r = model.hardest_negatives(np.zeros(0, dtype=np.int32), np.zeros((0, 4), dtype=np.int32))
    assert r.items.numel() == r.slots.numel() == r.scores.numel() == 0


def _dataset(ng=4):
    from ncf_amd.data import NCFData
    rng = np.random.default_rng(9)
    pairs = np.unique(np.stack([rng.integers(0, 30, 200), rng.integers(0, 40, 200)], 1), axis=0)
    return NCFData(pairs, 40, None, ng, True), pairs


def test_bpr_host_epoch_with_select_stub():
    """select= turns the host epoch into P triples: the same ng_sample() and torch draws, a
    randperm over P, the stub's choice as the negative."""
    from ncf_amd.data import epoch_permutation
    from ncf_amd.trainer import bpr_host_epoch
    ds, pairs = _dataset()
    P = len(pairs)
    seen = {}

    def last(users, cand):  # the stub: each positive's last candidate
        seen["users"], seen["cand"] = np.array(users), np.array(cand)
        return cand[:, -1]

    np.random.seed(4)
    torch.manual_seed(4)
    rows = bpr_host_epoch(ds, select=last)
    np_after, torch_after = np.random.get_state()[1].copy(), torch.get_rng_state().clone()
    # the same draws by hand
    ds2, _ = _dataset()
    np.random.seed(4)
    torch.manual_seed(4)
    ds2.ng_sample()
    cand = ds2.arrays()[1][P:].reshape(P, 4)
    perm = epoch_permutation(P).numpy()
    assert np.array_equal(np.random.get_state()[1], np_after) and torch.equal(torch.get_rng_state(), torch_after)
    assert seen["cand"].shape == (P, 4) and np.array_equal(seen["cand"], cand)
    assert np.array_equal(seen["users"], pairs[:, 0])
    assert rows.dtype == np.int64 and rows.shape == (2 * P,)
    u, it, y = C.unpack_rows(rows)
    assert np.array_equal(y, np.tile([1, 0], P))
    assert np.array_equal(u[0::2], pairs[perm, 0]) and np.array_equal(u[1::2], pairs[perm, 0])
    assert np.array_equal(it[0::2], pairs[perm, 1]) and np.array_equal(it[1::2], cand[perm, -1])
    # without select: the uniform stream, 2 P num_ng rows, unchanged
    np.random.seed(4)
    torch.manual_seed(4)
    assert bpr_host_epoch(ds).shape == (2 * P * 4,)
    with pytest.raises(ValueError):
        bpr_host_epoch(ds, select=lambda users, cand: cand[:-1, 0])


def test_script_refuses_hard_without_bpr():
    """scripts/train_neumf.py: --negatives hard is only valid with --loss bpr (argparse error)."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_neumf.py"), "--negatives", "hard"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--negatives hard is only valid with --loss bpr" in out.stderr


def test_trainer_and_pipeline_value_errors():
    from ncf_amd.pipeline import EpochPipeline
    from ncf_amd.trainer import Trainer
    _, model = C.models("NeuMF-end", 8, 3, 30, 40, 1)
    ds, _ = _dataset()
    with pytest.raises(ValueError):
        Trainer(model, ds, None, loss="bce", negatives="hard")
    with pytest.raises(ValueError):
        Trainer(model, ds, None, negatives="hard")  # the default loss is bce
    with pytest.raises(ValueError):
        Trainer(model, ds, None, loss="bpr", negatives="hardest")
    with pytest.raises(ValueError):
        EpochPipeline(ds, "cpu", 256, 40, pairwise=False, select=lambda users, cand: cand[:, 0])
