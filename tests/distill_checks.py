"""Shared pieces of the distillation tests (tests/test_distill_reference.py on the CPU,
tests/test_gpu_distill_paths.py on the device).

The reference of every numeric check is the ``ncf_amd.distill`` module itself -- the
restatement of the reference project's ``src/distillation`` that tests/test_distill_host.py
pins to that project's outputs -- evaluated with stock torch CPU ops in **float64**
(``module.double()``, labels as double) under torch autograd and ``torch.optim.Adam``;
never the device plan under test.  tests/test_distill_reference.py ties the float64
evaluation to tests/golden/G8_distill.npz.

Tolerances: the project's own (tests/test_gpu_parity.py), restated here.
  * logits  rtol 1e-5, atol 1e-7            * loss  rtol 1e-5
  * gradients (``test_gpu_parity._close_grad``): rtol 1e-4 with atol 1e-6 * max|g|, or for embedding
    tables whose rows sum `terms` contributions in float-atomic order
    max(1e-6, 2e-8 * sqrt(terms)) * max|g|

``wrong=`` turns the reference into a deliberately wrong one (what a plausible kernel
slip would compute); tests/test_distill_reference.py asserts that each lies outside the
criteria above at every shape the device tests use, so a device result cannot satisfy
both:
  * "no_gb"  -- a rank shard normalised by its own row count instead of the global batch
               size; at one rank: the row sums left undivided (a missing ``/ s.gb``)
  * "shift"  -- the teacher logit read one row off (``m`` where ``s.base + m`` belongs)
"""
import copy

import numpy as np
import torch

LOGIT_RTOL, LOGIT_ATOL, LOSS_RTOL = 1e-5, 1e-7, 1e-5
ML1M = (6041, 3707)
STRATEGIES = ("response", "soft", "feature")


def grad_excess(got, exp, terms=None):
    """Largest |got - exp| in units of test_gpu_parity._close_grad's tolerance (<= 1 passes)."""
    scale = max(float(np.abs(exp).max()), 1e-30)
    atol = 1e-6 * scale if terms is None else max(1e-6, 2e-8 * float(np.sqrt(terms))) * scale
    return float((np.abs(got - exp) / (atol + 1e-4 * np.abs(exp))).max())


def make(strategy, teacher, student):
    """The distillation module of a strategy name at the settings the tests use:
    response -- ResponseDistillation (the logit MSE: the device plan's T = 0);
    soft -- SoftTargetDistillation's defaults (T = 4, alpha = 0.7);
    feature -- FeatureDistillation (T = 2, alpha = 0.5, beta = 0.3);
    attention -- AttentionDistillation (T = 2, alpha = 0.5, gamma = 0.2)."""
    from ncf_amd import distill as D
    if strategy == "response":
        return D.ResponseDistillation(teacher, student, temperature=2.0, alpha=0.5)
    if strategy == "soft":
        return D.SoftTargetDistillation(teacher, student)
    if strategy == "feature":
        return D.FeatureDistillation(teacher, student, temperature=2.0, alpha=0.5, beta=0.3)
    if strategy == "attention":
        return D.AttentionDistillation(teacher, student, temperature=2.0, alpha=0.5, gamma=0.2)
    raise ValueError(strategy)


def build(tspec, sspec, strategy, U, I, seed):
    """(teacher, student, module) on the CPU in float32 from one generator seed; specs are
    (model_type, factor_num, num_layers).  The same arguments give the same parameters, so
    the device side and the float64 side each build their own."""
    from ncf_amd.models import NCF
    torch.manual_seed(seed)
    teacher = NCF(U, I, tspec[1], tspec[2], 0.0, tspec[0])
    student = NCF(U, I, sspec[1], sspec[2], 0.0, sspec[0])
    return teacher, student, make(strategy, teacher, student)


def f64(d):
    """A float64 copy of a distillation module (teacher, student and adapters)."""
    return copy.deepcopy(d).double()


def draw(student, B, U, I, data_seed, untie, zipf=1.3):
    """users, zipf-hot items (atomic contention) and float labels of B rows; `untie`
    (test_gpu_parity._untie) redraws the users of rows near a ReLU kink of `student`."""
    rng = np.random.default_rng(data_seed)
    users = rng.integers(0, U, B)
    items = np.minimum(rng.zipf(zipf, B) - 1, I - 1)
    labels = (rng.random(B) < 0.2).astype(np.float32)
    if untie is not None:
        users = untie(student, users, items, U, rng)
    return users, items, labels


class _Wrong:
    """Context: the module evaluates a deliberately wrong loss (module doc)."""

    def __init__(self, d, wrong):
        self.d, self.wrong = d, wrong

    def __enter__(self):
        d = self.d
        if self.wrong == "shift":
            t = d.teacher_model
            fwd = t.forward
            t.forward = lambda u, i: fwd(u, i).roll(1)
        return self

    def __exit__(self, *exc):
        self.d.teacher_model.__dict__.pop("forward", None)


def step_reference(d64, users, items, labels, lo=0, hi=None, wrong=None):
    """One batch on the float64 module: (loss, student logits, {name: student gradient}).
    With [lo, hi): those rows of the global batch only, normalised by the global batch
    size -- what rank r of a data-parallel step contributes (the ranks' sums are the
    one-rank step).  Parameters without a gradient (tables the loss does not reach) are
    absent from the dict."""
    gb = len(users)
    hi = gb if hi is None else hi
    for p in d64.parameters():
        p.grad = None
    u = torch.as_tensor(np.asarray(users[lo:hi]), dtype=torch.int64)
    i = torch.as_tensor(np.asarray(items[lo:hi]), dtype=torch.int64)
    y = torch.as_tensor(np.asarray(labels[lo:hi]), dtype=torch.float64)
    with _Wrong(d64, wrong):
        loss = d64(u, i, y)
    if wrong == "no_gb":
        loss = loss * (hi - lo) if hi - lo == gb else loss
    else:
        loss = loss * ((hi - lo) / gb)
    loss.backward()
    s = d64.student_model
    with torch.no_grad():
        logits = s(u, i).numpy().copy()
    grads = {k: p.grad.numpy().copy() for k, p in s.named_parameters() if p.grad is not None}
    return float(loss.item()), logits, grads


def batch_slices(n, B, steps):
    """Stream slices of `steps` consecutive steps over n rows in batches of B: the last
    batch of an epoch is short (DataLoader drop_last=False), then the stream wraps."""
    nb = (n + B - 1) // B
    return [slice((t % nb) * B, min(n, (t % nb + 1) * B)) for t in range(steps)]


def trajectory(d64, users, items, labels, B, steps, lr=1e-3, opt=None):
    """`steps` steps of the float64 module plus torch.optim.Adam on the student over the
    stream (batch_slices): (per-step losses, student state_dict as numpy).  opt: an
    optimizer to go on with (a run over several streams)."""
    s = d64.student_model
    if opt is None:
        opt = torch.optim.Adam(s.parameters(), lr=lr)
    losses = []
    for sl in batch_slices(len(users), B, steps):
        opt.zero_grad()
        loss = d64(torch.as_tensor(np.asarray(users[sl]), dtype=torch.int64),
                   torch.as_tensor(np.asarray(items[sl]), dtype=torch.int64),
                   torch.as_tensor(np.asarray(labels[sl]), dtype=torch.float64))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return np.array(losses), {k: v.detach().numpy().copy() for k, v in s.state_dict().items()}


def shard_bounds(gb, world, rank):
    """Rows [lo, hi) of a global batch of gb rows that rank `rank` of `world` takes
    (include/ncf_hip.h: ceil(gb / world) each)."""
    per = -(-gb // world)
    return min(rank * per, gb), min((rank + 1) * per, gb)


# ---- the one-step cases of tests/test_gpu_distill_paths.py: (teacher, student, rows).
# The teacher of the path cases is small and fused, and its tower widths (dm 16) differ
# from every student's, so no tower feature key matches (DeviceDistillPlan refuses those).
T_SMALL = ("NeuMF-end", 8, 2)
PATH_CASES = {
    "fused-per-row": (T_SMALL, ("NeuMF-end", 8, 3), 1024),
    "fused-factored": (T_SMALL, ("NeuMF-end", 16, 3), 8192),
    "layered-chain": (T_SMALL, ("NeuMF-end", 32, 3), 4096),
    "predict-f6": (T_SMALL, ("NeuMF-end", 6, 3), 3001),
    "predict-mlp-f11": (T_SMALL, ("MLP", 11, 2), 777),
    "predict-gmf-f5": (T_SMALL, ("GMF", 5, 1), 2000),
    "wide-chain": (T_SMALL, ("NeuMF-end", 64, 4), 1000),
}
FEATURE_CASES = {
    "s-gt-64": (("NeuMF-end", 64, 4), ("NeuMF-end", 32, 3), 777),       # mlp_input 256 -> 1024, GMF 32 -> 64
    "identity-gmf": (("NeuMF-end", 8, 3), ("NeuMF-end", 8, 2), 1000),   # GMF 8 == 8, mlp_input 32 -> 64
    "grid-stride": (("NeuMF-end", 16, 3), ("MLP", 8, 2), 8192 + 300),   # > 2048 blocks x 4 rows
}
SHARD_CASES = {  # (teacher, student, rows): 3 does not divide the rows
    "fused": (T_SMALL, ("NeuMF-end", 16, 3), 3001),
    "layered": (T_SMALL, ("NeuMF-end", 32, 3), 3001),
}
ALL_CASES = {**PATH_CASES, **FEATURE_CASES, **SHARD_CASES}
SEED, DATA_SEED = 11, 3
_problems = {}


class Problem:
    """One case's data (a draw without ReLU ties of the student, zipf-hot items at the
    ml-1m id space) and its float64 module; step() is cached per (lo, hi, wrong)."""

    def __init__(self, case, strategy):
        from test_gpu_parity import _untie
        self.case, self.strategy = case, strategy
        self.tspec, self.sspec, self.B = ALL_CASES[case]
        self.U, self.I = ML1M
        self.d64 = f64(self.build()[2])
        self.users, self.items, self.labels = draw(self.d64.student_model, self.B, self.U, self.I, DATA_SEED,
                                                   _untie)
        self._steps = {}

    def build(self):
        """A fresh float32 (teacher, student, module) on the CPU with this case's parameters."""
        return build(self.tspec, self.sspec, self.strategy, self.U, self.I, SEED)

    def step(self, lo=0, hi=None, wrong=None):
        key = (lo, hi, wrong)
        if key not in self._steps:
            loss, logits, grads = step_reference(self.d64, self.users, self.items, self.labels, lo, hi, wrong)
            logits.flags.writeable = False
            for g in grads.values():
                g.flags.writeable = False
            self._steps[key] = (loss, logits, grads)
        return self._steps[key]

    def terms(self, name, lo=0, hi=None, fact=False):
        """_close_grad's `terms` of a parameter over rows [lo, hi): the hottest id's row
        count for an embedding table -- and, with the factored layer 0 (`fact`), for the
        first tower weight, whose gradient is formed from per-user / per-item sums added in
        arrival order -- None elsewhere."""
        hot_u = int(np.bincount(self.users[lo:hi]).max())
        hot_i = int(np.bincount(self.items[lo:hi]).max())
        if fact and name == "MLP_layers.1.weight":
            return max(hot_u, hot_i)
        if "embed" not in name:
            return None
        return hot_i if "item" in name else hot_u


def problem(case, strategy):
    """The shared Problem of (case, strategy): built once per session, never modified."""
    key = (case, strategy)
    if key not in _problems:
        _problems[key] = Problem(case, strategy)
    return _problems[key]
