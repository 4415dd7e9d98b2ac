"""Candidate ranking, host side: NCF.rank on a CPU model against the oracle
(tests/rank_checks.py), the three forms of `candidates`, the argument checks, the ABI
exports and scripts/rank.py.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bpr_checks as C
import hardneg_checks as H
import rank_checks as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, I = 50, 80
MODELS = [("NeuMF-end", 8, 3), ("MLP", 16, 2), ("GMF", 16, 1)]


def _scores(ref):
    return H.oracle_scores(ref, np.arange(U), np.tile(np.arange(I), (U, 1)))


def test_abi_exports_and_docs():
    import ncf_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "ncf_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert int(re.search(r"#define NCF_ABI_VERSION (\d+)", hdr).group(1)) == 21 == L.ABI_VERSION
    for name in ("ncf_rank_candidates_workspace_bytes", "ncf_rank_candidates", "ncf_debug_set_rank_path"):
        assert name in hdr and name in L._HIP_PROTOS and hasattr(L.hip(), name), name
    assert "ncf_rank_candidates" in doc


@pytest.mark.parametrize("mt,f,Lyr", MODELS)
@pytest.mark.parametrize("k", [1, 10, 128])
def test_cpu_rank_vs_oracle(mt, f, Lyr, k):
    from ncf_amd import ops
    ref, model = C.models(mt, f, Lyr, U, I, 11)
    S = _scores(ref)
    users, ptr, items = R.ragged(R.cycle_lengths(40), U, I)
    model.train()  # dropout never applies, whatever the mode
    r = model.rank(users, ops.CandidateLists(torch.from_numpy(ptr), torch.from_numpy(items)), k)
    assert isinstance(r, ops.Ranked)
    assert r.items.dtype == torch.int64 and r.slots.dtype == torch.int64 and r.scores.dtype == torch.float32
    R.check_ranked(r.items, r.slots, r.scores, users, ptr, items, S, k, f"cpu {mt}({f},{Lyr}) k={k}")
    # a list's result depends on that list alone
    head = model.rank(users[:7], ops.CandidateLists(torch.from_numpy(ptr[:8]), torch.from_numpy(items[:ptr[7]])), k)
    for a, b in zip(head, r):
        assert torch.equal(a, b[:7])


def test_cpu_candidate_forms_agree():
    from ncf_amd import ops
    _, model = C.models("NeuMF-end", 8, 3, U, I, 11)
    rng = np.random.default_rng(5)
    users = rng.integers(0, U, 12).astype(np.int64)
    shared = rng.permutation(I)[:30].astype(np.int64)
    grid = np.tile(shared, (12, 1))
    base = model.rank(users, shared, k=10)                                  # 1-D: one shared list
    forms = [model.rank(users, grid, k=10),                                 # 2-D
             model.rank(torch.from_numpy(users), torch.from_numpy(grid), k=10),
             model.rank(users, ops.candidate_lists(grid), k=10),            # CandidateLists
             model.rank(users, ops.candidate_lists([list(shared)] * 12), k=10),
             model.rank(users, ops.CandidateLists(torch.arange(13) * 30, torch.from_numpy(grid.reshape(-1))), k=10)]
    for r in forms:
        for a, b in zip(base, r):
            assert torch.equal(a, b)
    assert base.items.shape == (12, 10) and (base.slots >= 0).all()
    assert np.array_equal(base.items.numpy(), shared[base.slots.numpy()])
    # ragged lists through candidate_lists
    cl = ops.candidate_lists([[3, 4, 5], [], [7]])
    assert cl.ptr.tolist() == [0, 3, 3, 4] and cl.items.tolist() == [3, 4, 5, 7]
    r = model.rank([1, 2, 3], cl, k=2)
    assert r.items[1].tolist() == [-1, -1] and r.slots[2].tolist() == [0, -1] and r.items[2, 0] == 7
    assert torch.isneginf(r.scores[1]).all() and torch.isneginf(r.scores[2, 1])


def test_cpu_duplicates_order_by_slot():
    _, model = C.models("NeuMF-end", 8, 3, U, I, 11)
    r = model.rank([4], np.full((1, 40), 9), k=10)
    assert r.slots[0].tolist() == list(range(10)) and (r.items == 9).all()
    assert len(set(r.scores[0].tolist())) == 1
    lst = np.array([[5, 9, 5, 9, 5, 9]])
    r = model.rank([4], lst, k=6)
    s = r.slots[0].numpy()
    assert sorted(s.tolist()) == list(range(6))
    for item in (5, 9):  # the copies of one id: equal scores, ascending slots, adjacent
        pos = np.flatnonzero(r.items[0].numpy() == item)
        assert np.array_equal(pos, np.arange(pos[0], pos[0] + 3)) and (np.diff(s[pos]) > 0).all()


def test_rank_argument_errors():
    from ncf_amd import ops
    _, model = C.models("NeuMF-end", 8, 3, U, I, 11)
    users = np.arange(10)
    cand = np.tile(np.arange(6), (10, 1))
    for k in (0, 129, 2.5, True):
        with pytest.raises(ValueError):
            model.rank(users, cand, k=k)
    with pytest.raises(ValueError):
        model.rank(users, cand[:9])                                  # users / ptr length mismatch
    with pytest.raises(ValueError):
        model.rank(users.reshape(5, 2), cand)                        # users not [n]
    with pytest.raises(ValueError):
        model.rank(users, cand.reshape(10, 3, 2))                    # candidates with three dimensions
    with pytest.raises(ValueError):
        model.rank(users[:2], ops.CandidateLists(torch.tensor([0, 4, 2]), torch.arange(4)))   # non-monotone ptr
    with pytest.raises(ValueError):
        model.rank(users[:2], ops.CandidateLists(torch.tensor([0, 2, 3]), torch.arange(4)))   # ptr[n] != len(items)
    with pytest.raises(ValueError):
        model.rank(users[:2], ops.CandidateLists(torch.tensor([1, 2, 4]), torch.arange(4)))   # ptr[0] != 0
    with pytest.raises(ValueError):
        model.rank(users[:2], ops.CandidateLists(torch.tensor([0, 2, 4], dtype=torch.int32), torch.arange(4)))
    bad = cand.copy()
    bad[3, 2] = I
    with pytest.raises(IndexError):
        model.rank(users, bad)
    bad[3, 2] = -1
    with pytest.raises(IndexError):
        model.rank(users, bad)
    with pytest.raises(IndexError):
        model.rank(np.full(10, U), cand)
    with pytest.raises(ValueError):
        ops.candidate_lists(np.arange(4))                            # a shared list without n_users
    r = model.rank(np.zeros(0, dtype=np.int64), np.zeros((0, 4), dtype=np.int64), k=3)
    assert r.items.shape == r.slots.shape == r.scores.shape == (0, 3)


def test_rank_script_end_to_end(tmp_path):
    """scripts/rank.py on a tiny checkpoint: one list per distinct user in file order."""
    ref, model = C.models("NeuMF-end", 8, 3, U, I, 11)
    ckpt = os.path.join(str(tmp_path), "tiny.pth")
    torch.save(model.state_dict(), ckpt)
    # interleaved users, a duplicate candidate, a user with a single line
    pairs = [(7, 3), (2, 10), (7, 5), (2, 11), (7, 3), (40, 79), (2, 12), (7, 60)]
    tsv = os.path.join(str(tmp_path), "cand.tsv")
    with open(tsv, "w") as fh:
        fh.writelines(f"{u}\t{i}\n" for u, i in pairs)
    out = os.path.join(str(tmp_path), "ranked.npz")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rank.py"), "--checkpoint", ckpt, "--model",
                          "NeuMF-end", "--top_k", "3", "--candidates", tsv, "--out", out, "--device", "cpu"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    z = np.load(out)
    assert z["users"].tolist() == [7, 2, 40]
    ptr = np.array([0, 4, 7, 8])
    cand = np.array([3, 5, 3, 60, 10, 11, 12, 79])
    R.check_ranked(z["items"], z["slots"], z["scores"], z["users"], ptr, cand, _scores(ref), 3, "scripts/rank.py")
    assert z["items"][2].tolist() == [79, -1, -1]
