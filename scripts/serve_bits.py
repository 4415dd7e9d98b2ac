#!/usr/bin/env python3
"""sha256 of what the serving entry points compute, per shape -- run it under two library
builds (NCF_HIP_LIB=<variant>; scripts/build_prev.sh builds the parent commit's as `prev`)
to check that a change that claims to keep the arithmetic gives bitwise the same outputs.

Per fused shape (every (type, f, layers) ncf_supported calls fused), at U = 50, I = 80:
  rec    ncf_recommend, all users: k = 10 with a seen CSR, k = 80 without (items, scores)
  sel    ncf_select_negatives: n in {17, 1000} x m in {5, 40}, all three outputs
  fold   ncf_fold_in: 20 users with lists of 1 .. 40 examples, 5 steps; ug, um, both moments,
         loss_out and grad_out
  rank   ncf_rank_candidates: n_lists in {17, 1100} (17 < U: row-indexed projections, several
         splits; 1100: one split, the user table) x k in {10, 128}, list lengths cycling
         through 0, 1, 15, 16, 17, 80, 200 with repeated ids; all three outputs
  tgt    ncf_target_ranks: the same lists as targets, with the seen CSR and without (ranks, scores)
The same five for one shape without a fused kernel, NeuMF-end(6,3), through the
materialised / generic paths, and one ncf_neighbors call (NeuMF-end(16,3): item side, concat
space, cosine, k = 10).  Each of these is a fixed-order computation, so two runs of one
library must agree bit for bit; --cmp checks that first (A against A2) and then B against A.
One process per library (the library is chosen at import).

--cpu hashes instead what NCF.recommend, rank, target_ranks, hardest_negatives, similar_items and
fold_in give on a CPU model (stock torch ops, no library) for GMF(8,1), MLP(8,2) and NeuMF-end(16,3),
from the same seeds and inputs: the check of a change to the Python serving layer.
usage: serve_bits.py [--cpu] --save DIR  (the hashed arrays as DIR/<shape>.npz; prints BITS lines)
       serve_bits.py --cmp DIR_A DIR_A2 DIR_B"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U, I = 50, 80


def shapes():
    import ncf_amd._lib as L
    fused = [(mt, f, nl) for mt in ("GMF", "MLP", "NeuMF-end") for f in range(1, 65) for nl in (1, 2, 3, 4)
             if (mt != "GMF" or nl == 1) and L.supported(mt, f, nl) == 1]
    assert L.supported("NeuMF-end", 6, 3) == 2
    return fused + [("NeuMF-end", 6, 3)]


CPU_SHAPES = [("GMF", 8, 1), ("MLP", 8, 2), ("NeuMF-end", 16, 3)]
RANK_LENGTHS = (0, 1, 15, 16, 17, 80, 200)


def outputs(mt, f, nl, cpu=False):
    """name -> array of everything the entry points (cpu: the NCF methods) give for this shape."""
    import numpy as np
    import torch
    from ncf_amd import ops
    from ncf_amd.models import NCF
    dev = "cpu" if cpu else "cuda:0"
    torch.manual_seed(11)
    m = NCF(U, I, f, nl, 0.0, mt).to(dev)
    recommend = m.recommend if cpu else (lambda u, k, s: ops.recommend(m, u, k, s))
    hardest = m.hardest_negatives if cpu else (lambda u, c: ops.select_negatives(m, u, c))
    rank = m.rank if cpu else (lambda u, c, k: ops.rank_candidates(m, u, c, k))
    target_ranks = m.target_ranks if cpu else (lambda u, t, s: ops.target_ranks(m, u, t, s))
    with torch.no_grad():  # spread tables: logits and ReLU masks are not degenerate
        for emb in (m.embed_user_GMF, m.embed_item_GMF, m.embed_user_MLP, m.embed_item_MLP):
            emb.weight.normal_(0.0, 0.3)
    rng = np.random.default_rng(5)
    out = {}
    su, si = np.nonzero(rng.random((U, I)) < 0.2)
    seen = ops.seen_csr(su, si, U, dev, I)
    for name, k, s in (("rec_k10_seen", 10, seen), ("rec_k80", I, None)):
        it, sc = recommend(torch.arange(U), k, s)
        out[name + "_items"], out[name + "_scores"] = it.cpu().numpy(), sc.cpu().numpy()
    for n in (17, 1000):
        for mm in (5, 40):
            r = hardest(rng.integers(0, U, n), rng.integers(0, I, (n, mm)))
            for key, v in zip(("items", "slots", "scores"), r):
                out[f"sel_n{n}_m{mm}_{key}"] = v.cpu().numpy()
    lengths = np.linspace(1, 40, 20).round().astype(np.int64)
    ex = ops.FoldExamples(torch.as_tensor(np.concatenate([[0], np.cumsum(lengths)])),
                          torch.as_tensor(np.concatenate([rng.choice(I, n, replace=False) for n in lengths]), dtype=torch.int32),
                          torch.as_tensor(rng.random(int(lengths.sum())) < 0.4, dtype=torch.float32))
    dm = f << (nl - 1)
    gmf0 = torch.as_tensor(rng.normal(0, 0.3, (20, f)), dtype=torch.float32)
    mlp0 = torch.as_tensor(rng.normal(0, 0.3, (20, dm)), dtype=torch.float32)
    if cpu:
        r = m.fold_in(ex, 5, 0.05, (0.9, 0.999), 1e-8, 0.01, init=(gmf0, mlp0))
    else:
        grad = torch.zeros((20, f + dm), device=dev)
        r = ops.fold_in(m, ex, gmf0, mlp0, 5, 0.05, (0.9, 0.999), 1e-8, 0.01, grad_out=grad)
        torch.cuda.synchronize()
        out["fold_grad"] = grad.cpu().numpy()
    out.update(fold_ug=r.gmf.cpu().numpy(), fold_um=r.mlp.cpu().numpy(), fold_m=r.state.exp_avg.cpu().numpy(),
               fold_v=r.state.exp_avg_sq.cpu().numpy(), fold_loss=r.loss.cpu().numpy())
    if cpu or (mt, f, nl) == ("NeuMF-end", 16, 3):
        ids, sc = (m.similar_items(torch.arange(I), 10, "concat", "cosine") if cpu
                   else ops.neighbors(m, "item", torch.arange(I), 10, "concat", "cosine"))
        out["nb_ids"], out["nb_scores"] = ids.cpu().numpy(), sc.cpu().numpy()
    for n in (17, 1100):  # drawn after everything else: the arrays above keep their earlier inputs
        lens = np.resize(RANK_LENGTHS, n)
        lists = ops.CandidateLists(torch.as_tensor(np.concatenate([[0], np.cumsum(lens)])),
                                   torch.as_tensor(rng.integers(0, I, int(lens.sum()))))
        users = torch.as_tensor(rng.integers(0, U, n))
        for k in (10, 128):
            for key, v in zip(("items", "slots", "scores"), rank(users, lists, k)):
                out[f"rank_n{n}_k{k}_{key}"] = v.cpu().numpy()
        for tag, s in (("seen", seen), ("all", None)):
            r = target_ranks(users, lists, s)
            out[f"tgt_n{n}_{tag}_ranks"], out[f"tgt_n{n}_{tag}_scores"] = r.ranks.cpu().numpy(), r.scores.cpu().numpy()
    assert all(np.isfinite(v[v > -np.inf]).all() for k, v in out.items() if v.dtype == np.float32)
    return out


def save(dest, cpu=False):
    sys.path.insert(0, ROOT)
    import numpy as np
    os.makedirs(dest, exist_ok=True)
    lib = "cpu" if cpu else os.environ.get("NCF_HIP_LIB", "") or "default"
    for mt, f, nl in (CPU_SHAPES if cpu else shapes()):
        out = outputs(mt, f, nl, cpu)
        name = f"{mt}_{f}_{nl}"
        np.savez(os.path.join(dest, name + ".npz"), **out)
        sha = lambda pre: hashlib.sha256(b"".join(out[k].tobytes() for k in sorted(out) if k.startswith(pre))
                                         ).hexdigest()[:16]
        nb = f" nb={sha('nb')}" if "nb_ids" in out else ""
        print(f"BITS {name} lib={lib} rec={sha('rec')} sel={sha('sel')} fold={sha('fold')} rank={sha('rank')} "
              f"tgt={sha('tgt')}{nb}", flush=True)


def cmp(da, da2, db):
    import numpy as np
    bad = 0
    names = sorted(os.listdir(da))
    for name in names:
        a, a2, b = (np.load(os.path.join(d, name)) for d in (da, da2, db))
        assert sorted(a.files) == sorted(a2.files) == sorted(b.files)
        for k in a.files:
            bits = lambda x: x.view(np.uint32) if x.dtype == np.float32 else x
            own, new = np.array_equal(bits(a[k]), bits(a2[k])), np.array_equal(bits(b[k]), bits(a[k]))
            if not (own and new):
                bad += 1
                diff = lambda x, y: float(np.abs(np.nan_to_num(x.astype(np.float64) - y, nan=0.0, posinf=0.0,
                                                               neginf=0.0)).max())
                print(f"CMP {name[:-4]} {k}: A==A2 {own} (max|A-A2|={diff(a[k], a2[k]):.3e}) "
                      f"B==A {new} (max|B-A|={diff(b[k], a[k]):.3e})")
    n_arrays = sum(len(np.load(os.path.join(da, n)).files) for n in names)
    print(f"CMP {len(names)} shapes, {n_arrays} arrays: {n_arrays - bad} bitwise equal in A, A2 and B; {bad} differ")
    return 1 if bad else 0


def main():
    args = sys.argv[1:]
    cpu = args[:1] == ["--cpu"]
    if len(args) == 2 + cpu and args[cpu] == "--save":
        return save(args[-1], cpu)
    if len(args) == 4 and args[0] == "--cmp":
        return cmp(*args[1:])
    raise SystemExit(__doc__)


if __name__ == "__main__":
    sys.exit(main())
