#!/usr/bin/env python3
"""Fold-in of unseen users: ncf_fold_in against the same contract in stock torch-ROCm ops.

Shape and data: an ml-1m-shaped NCF(6041, 3707, 16, 3) NeuMF-end and Q = 4,096 synthetic
users whose interaction lists are the training lists of 4,096 users of the synthetic ml-1m
(so the list lengths follow the training set's distribution), num_ng = 4 sampled negatives
per item, 50 full-batch Adam steps.  On the same GPU, in one process, device events around
each call, every shape warmed up:

  fused     one ncf_fold_in call (ops.fold_in_into, preallocated buffers), users in the
            caller's order, and again with the users sorted longest list first by the
            caller (the call orders its workgroups longest first itself, so the two should
            agree; before it did, this was the A/B of that ordering: DESIGN.md 3.10)
  torch     the same contract with stock torch-ROCm ops: users sorted by length and cut
            into padded batches of at most --pad_budget padded examples, functional
            forward (F.embedding / F.linear / relu), autograd, one torch.optim.Adam over
            the [Q, f] and [Q, dm] vectors -- the comparison point
  generic   ncf_fold_in through its generic path (ncf_debug_set_fold_path)

Reported per candidate: median / min / max of the repeats, microseconds per user-step
(time / (Q * steps)) and users per second; how far the three results agree (largest
differences, and the share of users outside the bounds of the trajectory tests: loss beyond
rtol 1e-5 at some step or a vector element beyond 1e-4 of the user's largest); the
algorithmic FLOPs and bytes of a call computed from the shapes.  One JSON document (--out).
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from ncf_amd import ops, synthetic  # noqa: E402
from ncf_amd.models import NCF  # noqa: E402
from serve_bench import alternate, emit, stats  # noqa: E402


def fold_stats(ms, q, steps):
    """serve_bench.stats plus the per-user figures."""
    s = stats(ms)
    return dict(s, us_per_user_step=s["median_ms"] * 1e3 / (q * steps), users_per_s=q / (s["median_ms"] * 1e-3))


def algorithmic_cost(f, nl, item_num, q, n_examples, steps):
    """FLOPs (2 per MAC) and compulsory bytes of one fused call, from the shapes alone."""
    dm = f << (nl - 1)
    tail = sum((dm >> (j - 1)) * (dm >> j) for j in range(1, nl))  # layers 1..L-1, MACs per example
    per_example = 2 * tail + 2 * f + 2 * f + 2 * dm  # forward + data gradient, predict, GMF, add/mask of width dm
    per_user_step = 2 * dm * dm  # Pu and W0u^T S
    flops = 2 * (steps * (n_examples * per_example + q * per_user_step) + item_num * dm * dm)
    # every step streams each example's Pi row, GMF row, id and label (from L2); vectors and state once
    bytes_ = steps * n_examples * 4 * (dm + f + 2) + 4 * item_num * 2 * dm + 4 * q * 4 * (f + dm)
    return {"flops": flops, "bytes": bytes_}


class Fused:
    def __init__(self, model, ex, gmf0, mlp0, steps, lr):
        self.flat, self.lay = ops.ensure_flat(model)
        dev = self.flat.device
        self.ex = ops.FoldExamples(ex.ptr.to(dev), ex.items.to(dev), ex.labels.to(dev))
        q = ex.ptr.numel() - 1
        self.start = (gmf0.to(dev), mlp0.to(dev))
        self.gmf, self.mlp = torch.empty_like(self.start[0]), torch.empty_like(self.start[1])
        self.loss = torch.empty((q, steps), device=dev)
        self.opt = ops.fold_opt(steps, lr, (0.9, 0.999), 1e-8, 0.0, 0)
        self.q, self.steps, self.model = q, steps, model

    def reset(self):
        self.gmf.copy_(self.start[0])
        self.mlp.copy_(self.start[1])

    def __call__(self):
        ws = ops.fold_in_workspace(self.lay, self.q, self.ex.items.numel(), self.steps, self.model, self.flat.device)
        ops.fold_in_into(self.flat, self.lay, self.ex, self.gmf, self.mlp, None, None, self.opt, self.loss, None, ws)


class TorchFold:
    """Padded batches, autograd and torch.optim.Adam with stock torch-ROCm ops."""

    def __init__(self, model, ex, gmf0, mlp0, steps, lr, pad_budget):
        dev = model.embed_item_GMF.weight.device
        self.w = [p.detach() for p in model.ordered_params()]  # ug, ig, um, im, (W, b) x L, wp, bp
        self.nl, self.steps, self.lr = model.num_layers, steps, lr
        ptr = ex.ptr.numpy()
        counts = np.diff(ptr)
        order = np.argsort(-counts, kind="stable")
        self.batches = []
        b = 0
        while b < len(order):
            width = max(int(counts[order[b]]), 1)
            rows = max(1, min(len(order) - b, pad_budget // width))
            users = order[b:b + rows]
            items = np.zeros((rows, width), dtype=np.int64)
            labels = np.zeros((rows, width), dtype=np.float32)
            weight = np.zeros((rows, width), dtype=np.float32)
            for r, u in enumerate(users):
                n = int(counts[u])
                items[r, :n] = ex.items[ptr[u]:ptr[u + 1]].numpy()
                labels[r, :n] = ex.labels[ptr[u]:ptr[u + 1]].numpy()
                weight[r, :n] = 1.0 / max(n, 1)
            self.batches.append((torch.as_tensor(users, device=dev), torch.as_tensor(items, device=dev),
                                 torch.as_tensor(labels, device=dev), torch.as_tensor(weight, device=dev)))
            b += rows
        self.start = (gmf0.to(dev), mlp0.to(dev))
        self.q = len(counts)
        self.reset()

    def reset(self):
        self.gmf = self.start[0].clone().requires_grad_(True)
        self.mlp = self.start[1].clone().requires_grad_(True)
        self.opt = torch.optim.Adam([self.gmf, self.mlp], lr=self.lr)
        self.loss = torch.zeros((self.q, self.steps), device=self.gmf.device)

    def __call__(self):
        w = self.w
        for s in range(self.steps):
            self.opt.zero_grad(set_to_none=True)
            for users, items, labels, weight in self.batches:
                rows, width = items.shape
                ug = self.gmf[users].unsqueeze(1)
                um = self.mlp[users].unsqueeze(1).expand(rows, width, -1)
                x = torch.cat((um, F.embedding(items, w[3])), -1)
                for k in range(self.nl):
                    x = torch.relu(F.linear(x, w[4 + 2 * k], w[5 + 2 * k]))
                out = torch.cat((ug * F.embedding(items, w[1]), x), -1)
                z = F.linear(out, w[-2], w[-1]).squeeze(-1)
                per = F.binary_cross_entropy_with_logits(z, labels, reduction="none") * weight
                self.loss[users, s] = per.detach().sum(1)
                per.sum().backward()
            self.opt.step()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--users", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--num_ng", type=int, default=4)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--slow_repeats", type=int, default=3, help="repeats of the torch and the generic runs")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pad_budget", type=int, default=1 << 21, help="padded examples per batch of the torch run")
    ap.add_argument("--out", default="profiles/fold_in.json")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_fold_in.py needs a HIP device: there is no CPU timing")
    dev = torch.device("cuda", 0)
    U, I, f, nl = 6041, 3707, 16, 3
    ds = synthetic.make_dataset("ml-1m", seed=0)
    seen = ops.seen_csr(ds["train_users"], ds["train_items"], U, None, I)
    rng = np.random.default_rng(0)
    picked = rng.choice(np.arange(1, U), size=min(args.users, U - 1), replace=False)  # user 0 does not occur
    ptr, items = seen.ptr.numpy(), seen.items.numpy()
    lists = [items[ptr[u]:ptr[u + 1]].astype(np.int64) for u in picked]
    q = len(lists)
    ex = ops.fold_examples(lists, I, args.num_ng, torch.Generator().manual_seed(0))
    lengths = np.diff(ex.ptr.numpy())
    by_length = np.argsort(-lengths, kind="stable")
    ex_sorted = ops.FoldExamples(
        torch.from_numpy(np.concatenate([[0], np.cumsum(lengths[by_length])]).astype(np.int64)),
        torch.cat([ex.items[int(ex.ptr[u]):int(ex.ptr[u + 1])] for u in by_length]),
        torch.cat([ex.labels[int(ex.ptr[u]):int(ex.ptr[u + 1])] for u in by_length]))
    torch.manual_seed(0)
    model = NCF(U, I, f, nl, 0.0, "NeuMF-end").to(dev)
    with torch.no_grad():  # spread tables, as after training: logits and masks are not degenerate
        for emb in (model.embed_user_GMF, model.embed_item_GMF, model.embed_user_MLP, model.embed_item_MLP):
            emb.weight.normal_(0.0, 0.3)
    gmf0 = model.embed_user_GMF.weight.detach().mean(0, keepdim=True).repeat(q, 1).cpu()
    mlp0 = model.embed_user_MLP.weight.detach().mean(0, keepdim=True).repeat(q, 1).cpu()

    fused = Fused(model, ex, gmf0, mlp0, args.steps, args.lr)
    fused_sorted = Fused(model, ex_sorted, gmf0, mlp0, args.steps, args.lr)
    base = TorchFold(model, ex, gmf0, mlp0, args.steps, args.lr, args.pad_budget)

    # every candidate has a reset(): alternate() calls it before each call, outside the timing
    times = alternate({"fused": fused, "sorted": fused_sorted}, args.warmup, args.repeats)
    t_f, t_s = times["fused"], times["sorted"]
    t_b = alternate({"torch": base}, 1, args.slow_repeats)["torch"]
    with ops._fold_generic():
        generic = Fused(model, ex, gmf0, mlp0, args.steps, args.lr)
        t_g = alternate({"generic": generic}, 1, args.slow_repeats)["generic"]
    torch.cuda.synchronize()

    def gap(a, b):
        return float((a - b).abs().max())

    def outside(a_gmf, a_mlp, a_loss, b_gmf, b_mlp, b_loss):
        va, vb = torch.cat((a_gmf, a_mlp), 1).double(), torch.cat((b_gmf, b_mlp), 1).double()
        bad = ((va - vb).abs() > 1e-4 * vb.abs().max(1, keepdim=True).values).any(1)
        bad |= ((a_loss.double() - b_loss.double()).abs() > 1e-5 * b_loss.double().abs()).any(1)
        return float(bad.double().mean())
    vec_scale = float(torch.cat((fused.gmf, fused.mlp), 1).abs().max())
    back = torch.as_tensor(np.argsort(by_length), device=dev)  # caller's order from the sorted call
    doc = {
        "device": torch.cuda.get_device_name(0),
        "shape": {"user_num": U, "item_num": I, "factor_num": f, "num_layers": nl, "model_type": "NeuMF-end",
                  "folded_users": q, "examples": int(ex.items.numel()), "num_ng": args.num_ng, "steps": args.steps,
                  "examples_per_user": {"min": int(lengths.min()), "median": float(np.median(lengths)),
                                        "mean": float(lengths.mean()), "max": int(lengths.max())}},
        "fused": dict(fold_stats(t_f, q, args.steps),
                      algorithmic=algorithmic_cost(f, nl, I, q, int(ex.items.numel()), args.steps)),
        "fused_presorted": fold_stats(t_s, q, args.steps),
        "torch_rocm": dict(fold_stats(t_b, q, args.steps), padded_batches=len(base.batches),
                           padded_examples=int(sum(b[1].numel() for b in base.batches))),
        "generic": fold_stats(t_g, q, args.steps),
        "agreement": {
            "largest_vector_magnitude": vec_scale,
            "fused_vs_torch_max_abs_vector": max(gap(fused.gmf, base.gmf.detach()), gap(fused.mlp, base.mlp.detach())),
            "fused_vs_generic_max_abs_vector": max(gap(fused.gmf, generic.gmf), gap(fused.mlp, generic.mlp)),
            "fused_vs_torch_max_abs_loss": gap(fused.loss, base.loss),
            "users_outside_bounds_fused_vs_torch": outside(fused.gmf, fused.mlp, fused.loss, base.gmf.detach(),
                                                           base.mlp.detach(), base.loss),
            "users_outside_bounds_generic_vs_torch": outside(generic.gmf, generic.mlp, generic.loss,
                                                             base.gmf.detach(), base.mlp.detach(), base.loss),
            "users_outside_bounds_fused_vs_generic": outside(fused.gmf, fused.mlp, fused.loss, generic.gmf,
                                                             generic.mlp, generic.loss),
            "sorted_call_bitwise_equal": bool(torch.equal(fused_sorted.gmf[back], fused.gmf)
                                              and torch.equal(fused_sorted.mlp[back], fused.mlp)
                                              and torch.equal(fused_sorted.loss[back], fused.loss)),
            "mean_loss_first_last": [float(fused.loss[:, 0].mean()), float(fused.loss[:, -1].mean())],
        },
    }
    doc["torch_over_fused"] = doc["torch_rocm"]["median_ms"] / doc["fused"]["median_ms"]
    doc["generic_over_fused"] = doc["generic"]["median_ms"] / doc["fused"]["median_ms"]
    emit(doc, args.out)


if __name__ == "__main__":
    main()
