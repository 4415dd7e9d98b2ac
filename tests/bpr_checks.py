"""Shared pieces of the pairwise (BPR) tests (tests/test_bpr.py on the CPU,
tests/test_gpu_bpr.py on the device).

The reference of every numeric check is ``oracle.ncf_oracle.OracleNCF`` under torch
autograd on the CPU with ``ncf_amd.losses.bpr_loss`` (plain torch) and
``torch.optim.Adam`` / ``SGD`` -- never the code under test.

Tolerances: the project's own (tests/test_gpu_parity.py), restated here.
  * logits  rtol 1e-5, atol 1e-7            * loss  rtol 1e-5
  * gradients (``close_grad``): rtol 1e-4 with atol 1e-6 * max|g|, or for embedding
    tables whose rows sum `terms` contributions in float-atomic order
    max(1e-6, 2e-8 * sqrt(terms)) * max|g|
  * teacher-forced steps: rtol 1e-5 + atol 5e-3 * lr

ReLU kinks: a triple is redrawn (its user) when either of its rows has a tower
pre-activation within 1e-6 of 0 -- there two correct fp32 summation orders may take
different sides of the ReLU.  ``untie_triples`` reports how many triples it touched; the
callers assert at most 1% (the project's flip sweep found single rows per several
thousand).
"""
import numpy as np
import torch

from oracle import ncf_oracle as O

LOGIT_RTOL, LOGIT_ATOL, LOSS_RTOL = 1e-5, 1e-7, 1e-5
TIE_TAU, TIE_MAX_FRACTION = 1e-6, 0.01


def close_grad(got, exp, name, terms=None):
    scale = max(float(np.abs(exp).max()), 1e-30)
    atol = 1e-6 * scale if terms is None else max(1e-6, 2e-8 * float(np.sqrt(terms))) * scale
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=atol, err_msg=name)


def tie_mask(ref, users, items, tau=TIE_TAU):
    """Rows with a tower pre-activation within tau of a ReLU kink at ref's parameters."""
    pres = []
    hs = [mm.register_forward_hook(lambda mod, i, o: pres.append(o.detach())) for mm in ref.MLP_layers
          if isinstance(mm, torch.nn.Linear)]
    with torch.no_grad():
        ref(torch.as_tensor(users), torch.as_tensor(items))
    for h in hs:
        h.remove()
    if not pres or ref.model_type == "GMF":
        return np.zeros(len(users), dtype=bool)
    return (torch.stack([p.abs().min(dim=1).values for p in pres]).min(dim=0).values < tau).numpy()


def untie_triples(ref, u, ip, ineg, U, rng, rounds=20):
    """(users, touched): the user of every triple with a row near a kink redrawn until
    none is; touched = number of distinct triples redrawn."""
    u = np.array(u, copy=True)
    touched = np.zeros(len(u), dtype=bool)
    for _ in range(rounds):
        near = tie_mask(ref, u, ip) | tie_mask(ref, u, ineg)
        if not near.any():
            return u, int(touched.sum())
        touched |= near
        u[near] = rng.integers(0, U, int(near.sum()))
    raise AssertionError("no tie-free draw")


def draw_triples(ref, T, U, I, data_seed, zipf=1.3):
    """T tie-free (user, item+, item-) triples with zipf-hot items (atomic contention);
    asserts the redraw touched at most 1% of them."""
    rng = np.random.default_rng(data_seed)
    u = rng.integers(0, U, T)
    ip = np.minimum(rng.zipf(zipf, T) - 1, I - 1)
    ineg = rng.integers(0, I, T)
    u, touched = untie_triples(ref, u, ip, ineg, U, rng)
    assert touched <= TIE_MAX_FRACTION * T, f"{touched} of {T} triples redrawn"
    return u, ip, ineg


def interleave(u, ip, ineg):
    """(users, items, labels) of the 2T-row pair stream of T triples."""
    T = len(u)
    users = np.repeat(np.asarray(u), 2)
    items = np.empty(2 * T, dtype=np.int64)
    items[0::2], items[1::2] = ip, ineg
    labels = np.tile(np.array([1, 0], dtype=np.int64), T)
    return users, items, labels


def bpr_forward_backward(ref, users, items, divisor=None):
    """Oracle: logits of the 2T rows (padding rows, user < 0, excluded from the loss),
    bpr loss and {name: grad}.  divisor: triples the sum is divided by (None: the valid
    triples, i.e. bpr_loss's mean)."""
    from ncf_amd.losses import bpr_loss
    ref.zero_grad(set_to_none=True)
    users = np.asarray(users)
    ok = users[0::2] >= 0
    uu = torch.as_tensor(np.where(users < 0, 0, users), dtype=torch.int64)
    ii = torch.as_tensor(np.where(users < 0, 0, np.asarray(items)), dtype=torch.int64)
    z = ref(uu, ii)
    okt = torch.from_numpy(ok)
    loss = bpr_loss(z[0::2][okt], z[1::2][okt])
    if divisor is not None:
        loss = loss * (float(ok.sum()) / float(divisor))
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
    return z.detach(), float(loss.item()), grads


def bpr_train_steps(ref, opt, users, items):
    """The reference loop body with the pairwise loss over pre-formed pair batches
    (users / items: [steps][2T]).  Returns the losses."""
    from ncf_amd.losses import bpr_loss
    losses = []
    for t in range(len(users)):
        u = torch.as_tensor(np.asarray(users[t]), dtype=torch.int64)
        i = torch.as_tensor(np.asarray(items[t]), dtype=torch.int64)
        opt.zero_grad()
        z = ref(u, i)
        loss = bpr_loss(z[0::2], z[1::2])
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses


def unpack_rows(rows):
    """(users int64 with -1 padding, items, labels) of packed int64 rows (numpy)."""
    r = np.asarray(rows).astype(np.int64)
    u = (r & 0xFFFFFFFF).astype(np.int64)
    u = np.where(u == 0xFFFFFFFF, -1, u)
    return u, (r >> 32) & 0x7FFFFFFF, (r >> 63) & 1


# The four embedding tables of every test model are multiplied by this (std 0.01 at the
# reference's initialisation -> 0.3, the scale of trained tables).  At std 0.01 every
# tower output is its bias to ~1e-2, so z+ - z- ~ 1e-3 for every triple: sigmoid(d) is 0.5
# throughout (the kernel's sigmoid would go unexercised) and the pair's +dz / -dz terms
# of the tower gradients cancel to ~1e-3 of their size, which leaves the fp32 oracle's own
# summation noise (measured against a float64 oracle) above the gradient rule's atol of
# 1e-6 * max|g|.  It also puts ~5% of NeuMF(64,4)'s triples (960 tower units per row) within
# 1e-6 of a ReLU kink whatever the seed.  With trained-size tables the differences are
# O(0.1), the rule holds for the oracle with margin, and ties stay under 1%.
EMB_SCALE = 30.0
# ... and the predict bias is set to this.  The pairwise loss does not depend on it (it
# cancels in z+ - z-; its gradient is 0).  With trained-size tables a logit is a sum of
# O(0.3) terms, evaluated in fp32 to ~1e-7 absolute whatever its value, and some of a few
# thousand logits land within 1e-2 of 0, where rtol 1e-5 + atol 1e-7 asks for more than
# that: the fp32 oracle itself misses it there against a float64 oracle (worst logit at
# up to 1.28x the tolerance at NeuMF(64,4), 1.07x at NeuMF(16,3)).  Away from 0 the rtol
# governs, as it does for the init-size logits the tolerance was written for (fp32 oracle
# against float64: at most 0.03x the logit tolerance and 0.26x the gradient rule over the
# cases of test_gpu_bpr.py).
PREDICT_BIAS = 1.0


def models(mt, f, L, U, I, seed, emb_scale=EMB_SCALE, predict_bias=PREDICT_BIAS):
    """(oracle on the CPU, ncf_amd NCF on the CPU) with identical parameters, the
    embedding tables of both multiplied by emb_scale and the predict bias set to
    predict_bias (EMB_SCALE, PREDICT_BIAS above)."""
    from ncf_amd.models import NCF
    torch.manual_seed(seed)
    ref = O.OracleNCF(U, I, f, L, 0.0, mt)
    torch.manual_seed(seed)
    m = NCF(U, I, f, L, 0.0, mt)
    if emb_scale != 1.0:
        with torch.no_grad():
            for mod in (ref, m):
                for k, p in mod.named_parameters():
                    if k.startswith("embed"):
                        p.mul_(emb_scale)
    if predict_bias is not None:
        with torch.no_grad():
            ref.predict_layer.bias.fill_(predict_bias)
            m.predict_layer.bias.fill_(predict_bias)
    for (k1, v1), (k2, v2) in zip(ref.state_dict().items(), m.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    return ref, m


def f64_drift(mt, f, L, U, I, seed, users, items, lr, kind="adam"):
    """Largest relative gap between the float32 and the float64 oracle's per-step
    losses on the same pair batches (both on the CPU)."""
    ref, _ = models(mt, f, L, U, I, seed)
    ref64, _ = models(mt, f, L, U, I, seed)
    ref64 = ref64.double()
    l32 = np.array(bpr_train_steps(ref, O.make_optimizer(ref, lr, kind), users, items))
    l64 = np.array(bpr_train_steps(ref64, O.make_optimizer(ref64, lr, kind), users, items))
    return float(np.max(np.abs(l32 - l64) / np.abs(l64)))
