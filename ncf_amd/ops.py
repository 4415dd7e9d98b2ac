"""Device-side operators of the NeuMF hot path (torch tensors -> C ABI pointers).

``ensure_flat`` packs a HIP-resident NCF's parameters into one flat fp32 buffer
laid out by ``ncf_layout_init`` (include/ncf_hip.h) and rebinds every
``nn.Parameter`` to a view of it, so the kernels read the live weights and the
module's ``state_dict`` / stock optimizers keep working.

``ncf_forward`` is the autograd-visible forward of ``NCF`` on a HIP device
(reference models.py:97-118); its backward is the same fused kernel in
``NCF_DZ_DLOGIT`` mode (replacing the ATen autograd graph that
``loss.backward()`` walks in train_neumf.py:114).  Everything runs on
``torch.cuda.current_stream()``.
"""
from __future__ import annotations

import collections
import contextlib

import numpy as np
import torch

from . import _lib as L


def _segments(model, lay):
    """(param, flat offset) in model.ordered_params() order."""
    offs = [lay.ug, lay.ig, lay.um, lay.im]
    for k in range(model.num_layers):
        offs += [lay.w[k], lay.b[k]]
    offs += [lay.wp, lay.bp]
    return list(zip(model.ordered_params(), offs))


@contextlib.contextmanager
def params_view(model, flat_snapshot):
    """The model's parameters temporarily viewing `flat_snapshot` (a copy of its
    flat buffer): e.g. a checkpoint of the parameters as an earlier step left them
    while later steps are already queued.  Nothing may repack the model inside."""
    lay = model._ncf_layout
    segs = _segments(model, lay)
    saved = [p.data for p, _ in segs]
    try:
        for p, off in segs:
            p.data = flat_snapshot[off:off + p.numel()].view_as(p)
        yield model
    finally:
        for (p, _), d in zip(segs, saved):
            p.data = d


def active_mask(model):
    """Which ordered params receive gradients (reference: unused tables keep
    .grad None in GMF / MLP mode, so torch Adam skips them)."""
    n_tower = 2 * model.num_layers
    if model.model_type == "GMF":
        return [True, True, False, False] + [False] * n_tower + [True, True]
    if model.model_type == "MLP":
        return [False, False, True, True] + [True] * n_tower + [True, True]
    return [True] * (4 + n_tower + 2)


def ensure_flat(model, min_floats=0):
    """Return (flat, layout) for a HIP-resident NCF, (re)packing if needed.
    ``min_floats``: the flat buffer is at least this long (zero padding after
    ``lay.total``; the sharded data-parallel optimizer needs world * shard floats)."""
    lay = getattr(model, "_ncf_layout", None)
    flat = getattr(model, "_ncf_flat", None)
    dev = model.embed_user_GMF.weight.device
    if lay is None:
        lay = L.layout(model.user_num, model.item_num, model.factor_num, model.num_layers, model.model_type)
        model._ncf_layout = lay
    if flat is not None and flat.device == dev and flat.numel() >= min_floats:
        ok = all(p.data_ptr() == flat.data_ptr() + 4 * off for p, off in _segments(model, lay))
        if ok:
            return flat, lay
    if not L.supported(model.model_type, model.factor_num, model.num_layers):
        raise NotImplementedError(
            f"no HIP path for model_type={model.model_type} factor_num={model.factor_num} "
            f"num_layers={model.num_layers}")
    flat = torch.zeros(max(int(lay.total), int(min_floats)), dtype=torch.float32, device=dev)
    with torch.no_grad():
        for p, off in _segments(model, lay):
            n = p.numel()
            view = flat[off:off + n].view_as(p)
            view.copy_(p.data)
            p.data = view
    model._ncf_flat = flat
    return flat, lay


def _as_i32(x, dev):
    x = torch.as_tensor(x, device=dev)
    if x.dtype != torch.int32:
        x = x.to(torch.int32)
    return x.contiguous()


def pack_rows(users_i32, items_i32, labels_f32=None, out=None):
    """Packed uint64 rows (stored as int64): user | item << 32 | (label != 0) << 63
    (include/ncf_hip.h NCF_ROW_PACK), built on the device by ncf_pack_rows."""
    n = users_i32.numel()
    dev = users_i32.device
    if items_i32.numel() != n or (labels_f32 is not None and labels_f32.numel() != n):
        raise ValueError("users/items/labels must have equal length")
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=dev)
    L.check(L.hip().ncf_pack_rows(users_i32.data_ptr(), items_i32.data_ptr(),
                                  None if labels_f32 is None else labels_f32.data_ptr(), n, out.data_ptr(),
                                  L.stream_ptr(dev)), "ncf_pack_rows")
    return out


def check_ids(users, items, user_num, item_num):
    """nn.Embedding's range check (reference models.py:98-112 raise IndexError on an
    id outside the table) for host arrays; the kernels do not bound-check gathers."""
    u = np.asarray(users)
    i = np.asarray(items)
    if u.size and (int(u.min()) < 0 or int(u.max()) >= user_num):
        raise IndexError("index out of range in self (user id)")
    if i.size and (int(i.min()) < 0 or int(i.max()) >= item_num):
        raise IndexError("index out of range in self (item id)")


def check_rows(rows, user_num, item_num):
    """Range check of a packed device stream (padding rows, user -1, allowed): a
    few reductions on the device and one host read."""
    if rows.numel() == 0:
        return
    u = (rows & 0xFFFFFFFF).to(torch.int64)
    it = (rows >> 32) & 0x7FFFFFFF
    pad = u == 0xFFFFFFFF
    bad_u = ((u >= user_num) & ~pad).any()
    bad_i = ((it >= item_num) & ~pad).any()
    bu, bi = torch.stack([bad_u, bad_i]).tolist()
    if bu:
        raise IndexError("index out of range in self (user id)")
    if bi:
        raise IndexError("index out of range in self (item id)")


def pack_rows_host(users, items, labels=None):
    """Host-side NCF_ROW_PACK of numpy arrays -> int64 numpy array."""
    r = np.asarray(users).astype(np.int64) & 0xFFFFFFFF
    r |= (np.asarray(items).astype(np.int64) & 0x7FFFFFFF) << 32
    if labels is not None:
        r |= (np.asarray(labels) != 0).astype(np.int64) << 63
    return r


# ---------------------------------------------------------------------------
# Pairwise (BPR) training stream (include/ncf_hip.h NCF_DZ_BPR, ncf_build_pair_stream)
def bpr_stream_host(pos_users, pos_items, neg, num_ng, perm=None):
    """The pair stream of ncf_build_pair_stream in NumPy (int64 packed rows, length
    2 * S, S = len(pos_users) * num_ng): triple k is t = perm[k] (identity when None),
    positive p = t // num_ng -- row 2k (pos_users[p], pos_items[p], label 1), row 2k + 1
    (pos_users[p], neg[t], label 0)."""
    pu = np.asarray(pos_users).astype(np.int64).reshape(-1)
    pi = np.asarray(pos_items).astype(np.int64).reshape(-1)
    ng = int(num_ng)
    S = pu.size * ng
    neg = np.asarray(neg).astype(np.int64).reshape(-1)
    if pu.size != pi.size or ng < 0 or neg.size < S:
        raise ValueError("bpr_stream_host: one item per positive and num_ng negatives per positive")
    t = np.arange(S, dtype=np.int64) if perm is None else np.asarray(perm).astype(np.int64).reshape(-1)
    if t.size != S:
        raise ValueError("bpr_stream_host: perm must order the n_pos * num_ng triples")
    p = t // max(ng, 1)
    out = np.empty(2 * S, dtype=np.int64)
    out[0::2] = pack_rows_host(pu[p], pi[p], np.ones(S, dtype=np.int64))
    out[1::2] = pack_rows_host(pu[p], neg[t])
    return out


def build_pair_stream(pos_users_i32, pos_items_i32, neg_i32, num_ng, perm=None, out=None):
    """ncf_build_pair_stream on the current stream: int32 device tensors of the positives
    and their negatives (ncf_build_rows' layout), perm an int64 device permutation of the
    S = n_pos * num_ng triples (None: identity) -> 2 * S packed int64 rows."""
    dev = pos_users_i32.device
    P, ng = pos_users_i32.numel(), int(num_ng)
    S = P * ng
    for t, what in ((pos_users_i32, "pos_users"), (pos_items_i32, "pos_items"), (neg_i32, "neg")):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"build_pair_stream: {what} must be a contiguous int32 tensor on one device")
    if pos_items_i32.numel() != P or ng < 0 or (S > 0 and (neg_i32 is None or neg_i32.numel() < S)):
        raise ValueError("build_pair_stream: one item per positive and num_ng negatives per positive")
    if perm is not None and (perm.dtype != torch.int64 or perm.numel() != S or not perm.is_contiguous()
                             or perm.device != dev):
        raise ValueError("build_pair_stream: perm must be a contiguous int64 permutation of the triples")
    if out is None:
        out = torch.empty(2 * S, dtype=torch.int64, device=dev)
    elif out.numel() != 2 * S or out.dtype != torch.int64 or not out.is_contiguous() or out.device != dev:
        raise ValueError("build_pair_stream out: 2 * n_pos * num_ng contiguous int64")
    L.check(L.hip().ncf_build_pair_stream(pos_users_i32.data_ptr(), pos_items_i32.data_ptr(), P,
                                          neg_i32.data_ptr() if S else None, ng,
                                          None if perm is None else perm.data_ptr(), out.data_ptr(),
                                          L.stream_ptr(dev)), "ncf_build_pair_stream")
    return out


def check_pair_rows(rows, user_num, item_num):
    """check_rows for a pair stream (NCF_DZ_BPR): also ValueError for an odd length, a
    pair whose labels are not (1, 0) or whose users differ (padding pairs: both rows
    with user -1).  `rows`: packed int64, a device tensor or a host array."""
    if not isinstance(rows, torch.Tensor):
        rows = torch.from_numpy(np.ascontiguousarray(np.asarray(rows), dtype=np.int64))
    n = rows.numel()
    if n % 2:
        raise ValueError("pair stream: an odd number of rows")
    if n == 0:
        return
    a, b = rows[0::2], rows[1::2]
    ua, ub = a & 0xFFFFFFFF, b & 0xFFFFFFFF
    pad = ua == 0xFFFFFFFF
    bad_y = (((a >> 63) & 1) != 1) | (((b >> 63) & 1) != 0)
    flags = torch.stack([(bad_y & ~pad).any(), (ua != ub).any()]).tolist()
    if flags[1]:
        raise ValueError("pair stream: the two rows of a pair have different users")
    if flags[0]:
        raise ValueError("pair stream: the labels of a pair are not (1, 0)")
    check_rows(rows, user_num, item_num)


def default_canonical():
    """True when torch.distributed runs more than one rank (the grouping must then be
    NCF_PREP_CANONICAL so every rank's stream is identical)."""
    import torch.distributed as dist
    return bool(dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)


_CHECK_W = {}


def stream_checksum(rows):
    """Order-sensitive int64 checksum of a device epoch stream (a few launches per
    chunk, no host sync): sum_k rows[k] * w_k (mod 2^64), w_k = (k * K) | 1.  Chunked:
    w of a chunk at offset o is (j * K + o * K) | 1 from one cached chunk-sized j * K,
    so no stream-length temporary is kept or allocated (C4: 99M rows)."""
    n = rows.numel()
    K = -7046029254386353131
    c = min(n, _CHECK_CHUNK)
    key = (c, rows.device)
    base = _CHECK_W.get(key)
    if base is None:
        base = torch.arange(c, dtype=torch.int64, device=rows.device) * K
        _CHECK_W.clear()
        _CHECK_W[key] = base
    total = torch.zeros((), dtype=torch.int64, device=rows.device)
    for o in range(0, n, c):
        m = min(c, n - o)
        # o * K wraps in int64 like the device product does
        ok = ((o * K + (1 << 63)) % (1 << 64)) - (1 << 63)
        total += (rows[o:o + m] * ((base[:m] + ok) | 1)).sum()
    return total


_CHECK_CHUNK = 1 << 22


class EpochPrep:
    """ncf_prepare_epoch with its device workspace kept between epochs (stable
    pointers, so the output can feed a captured step graph).  canonical: the rows
    of one item inside a batch in (user, label) order (NCF_PREP_CANONICAL), so that
    every data-parallel rank building the stream gets the same positions."""

    def __init__(self, device, canonical=None):
        """canonical None: on whenever torch.distributed is initialised with more than
        one rank (a data-parallel caller needs it; TrainEngine also checks that the
        ranks' streams agree)."""
        self.device = torch.device(device)
        self.ws = None
        self.out = None
        self.canonical = default_canonical() if canonical is None else bool(canonical)

    def __call__(self, rows, perm, batch_size, item_num, out=None):
        """On the current stream; into `out` (n int64 on the device) if given."""
        n = rows.numel()
        need = int(L.hip().ncf_prepare_epoch_workspace(n, int(batch_size), int(item_num)))
        if need < 0:
            raise ValueError("bad ncf_prepare_epoch sizes")
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if out is None:
            if self.out is None or self.out.numel() != n:
                self.out = torch.empty(n, dtype=torch.int64, device=self.device)
            out = self.out
        elif out.numel() != n or out.dtype != torch.int64 or not out.is_contiguous():
            raise ValueError("prepare_epoch out: n contiguous int64")
        L.check(L.hip().ncf_prepare_epoch2(rows.data_ptr(), perm.data_ptr(), n, int(batch_size), int(item_num),
                                           L.PREP_CANONICAL if self.canonical else 0, out.data_ptr(),
                                           self.ws.data_ptr(), self.ws.numel(), L.stream_ptr(self.device)),
                "ncf_prepare_epoch2")
        return out


def _ws(owner, attr, nbytes, dev):
    """Device workspace of at least nbytes, cached on `owner` (grown, never shrunk)."""
    if nbytes <= 0:
        return None
    ws = getattr(owner, attr, None)
    if ws is None or ws.numel() * 4 < nbytes or ws.device != dev:
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        setattr(owner, attr, ws)
    return ws


def _ws_args(ws):
    """(pointer, bytes) of a workspace tensor for the C ABI; None is a call that needs none."""
    return (None, 0) if ws is None else (ws.data_ptr(), ws.numel() * 4)


def _serve_ws(entry, attr, lay, owner, dev, *sizes):
    """The workspace ncf_<entry>_workspace_bytes(lay, *sizes) asks for, cached on owner.<attr>."""
    need = int(getattr(L.hip(), f"ncf_{entry}_workspace_bytes")(L.ctypes.byref(lay), *map(int, sizes)))
    if need < 0:
        raise ValueError(f"ncf_{entry}_workspace_bytes failed")
    return _ws(owner, attr, need, dev)


@contextlib.contextmanager
def _forced_path(entry):
    """ncf_debug_set_<entry>_path(PATH_LAYERED) for the block: that entry point's materialised
    (ncf_fold_in: generic) path whatever the shape."""
    setter = getattr(L.hip(), f"ncf_debug_set_{entry}_path")
    L.check(setter(L.PATH_LAYERED), f"ncf_debug_set_{entry}_path")
    try:
        yield
    finally:
        setter(0)


def check_id_range(*checks):
    """IndexError, as nn.Embedding raises it, for the first (ids, bound, name) whose ids leave
    [0, bound): "index out of range in self (<name> id)", without the suffix for name None.
    The kernels do not bound-check their gathers.  Tensors on any device, empty ones pass; one
    host read for the whole call."""
    live = [c for c in checks if c[0].numel()]
    if not live:
        return
    # with tensors on both sides the extremes meet on the HIP device: still one read
    dev = next((t.device for t, _, _ in live if t.is_cuda), live[0][0].device)
    lo_hi = torch.stack([f().to(dev, torch.int64) for t, _, _ in live for f in (t.min, t.max)]).tolist()
    for (_, bound, name), lo, hi in zip(live, lo_hi[0::2], lo_hi[1::2]):
        if lo < 0 or hi >= bound:
            raise IndexError("index out of range in self" + (f" ({name} id)" if name else ""))


def check_csr_ptr(ptr, n_entries, message):
    """ValueError(message) unless ptr (at least one entry) starts at 0, ends at n_entries and
    never descends; one host read."""
    first, last, descends = torch.stack([ptr[0], ptr[-1], (ptr[1:] < ptr[:-1]).any().to(ptr.dtype)]).tolist()
    if first != 0 or last != n_entries or descends:
        raise ValueError(message)


def forward_logits(flat, lay, rows, out=None, ws_owner=None):
    n = rows.numel()
    dev = flat.device
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=dev)
    need = int(L.hip().ncf_forward_workspace_bytes(L.ctypes.byref(lay), n))
    ws = _ws(ws_owner if ws_owner is not None else _scratch, "_ncf_fwd_ws", need, dev)
    L.check(L.hip().ncf_forward(L.ctypes.byref(lay), flat.data_ptr(), rows.data_ptr(), n, out.data_ptr(),
                                *_ws_args(ws), L.stream_ptr(dev)), "ncf_forward")
    return out


def fact_mode(lay):
    """Whether the factored layer-0 path runs for this layout (include/ncf_hip.h
    ncf_fact_mode; fused or layered path)."""
    return bool(L.hip().ncf_fact_mode(L.ctypes.byref(lay)))


def new_workspace(lay, rows, dev):
    """ncf_train_step workspace for up to `rows` rows per launch (float32 storage)."""
    need = int(L.hip().ncf_workspace_bytes(L.ctypes.byref(lay), int(rows)))
    if need < 0:
        raise ValueError("ncf_workspace_bytes failed")
    return torch.zeros((need + 3) // 4, dtype=torch.float32, device=dev)


def fused_backward(flat, lay, rows, dlogit, gflat, ws, ctl):
    """grads of sum_i dlogit[i] * logit[i] into gflat (zero-initialised)."""
    n = rows.numel()
    dev = flat.device
    st = L.stream_ptr(dev)
    L.check(L.hip().ncf_train_step(L.ctypes.byref(lay), flat.data_ptr(), gflat.data_ptr(), rows.data_ptr(), None,
                                   dlogit.data_ptr(), ctl.data_ptr(), int(n), 1, 0, L.DZ_DLOGIT,
                                   ws.data_ptr(), ws.numel() * 4, None, st), "ncf_train_step")
    L.check(L.hip().ncf_reduce_slab(L.ctypes.byref(lay), ws.data_ptr(), gflat.data_ptr(), ctl.data_ptr(), st),
            "ncf_reduce_slab")


class _Scratch:
    pass


_scratch = _Scratch()


def new_ctl(n_total, dev, batch=0, adam_t=0):
    """ncf_step_ctl: batch, adam_t, n_total, reserved, snap_batch, snap_t."""
    return torch.tensor([batch, adam_t, n_total, 0, 0, 0], dtype=torch.int64, device=dev)


def dropout_seed(dev):
    """The dropout hash seed: the device generator's seed (torch.manual_seed sets it)."""
    return int(torch.cuda.initial_seed()) & 0xFFFFFFFF


def set_dropout(lay, model):
    """Copy the model's tower dropout into a training layout (GMF has no tower)."""
    p = float(getattr(model, "dropout", 0.0) or 0.0)
    if p > 0 and model.model_type != "GMF":
        lay.dropout = p
        lay.dropout_seed = dropout_seed(model.embed_user_GMF.weight.device)
    else:
        lay.dropout = 0.0


def _dropout_layout(model):
    """Training-mode layout with the model's dropout, or None when dropout is off."""
    if not model.training:
        return None
    lay = type(model._ncf_layout).from_buffer_copy(model._ncf_layout)
    set_dropout(lay, model)
    if not lay.dropout > 0:
        return None
    model._ncf_drop_t = getattr(model, "_ncf_drop_t", -1) + 1  # a fresh mask per forward
    return lay, model._ncf_drop_t


def _dropout_logits(model, rows, drop):
    """Training-mode logits under dropout: the train step with dL/dlogit = 0 (same
    masks as the backward, which reruns it with the same step index)."""
    lay, t = drop
    flat = model._ncf_flat
    dev = flat.device
    n = rows.numel()
    logits = torch.empty(n, dtype=torch.float32, device=dev)
    scratch = torch.zeros(int(lay.total), dtype=torch.float32, device=dev)
    ws = new_workspace(lay, n, dev)
    ctl = new_ctl(n, dev, adam_t=t)
    dl = torch.zeros(n, dtype=torch.float32, device=dev)
    L.check(L.hip().ncf_train_step(L.ctypes.byref(lay), flat.data_ptr(), scratch.data_ptr(), rows.data_ptr(), None,
                                   dl.data_ptr(), ctl.data_ptr(), int(n), 1, 0, L.DZ_DLOGIT,
                                   ws.data_ptr(), ws.numel() * 4, logits.data_ptr(), L.stream_ptr(dev)),
            "ncf_train_step")
    return logits


class _NCFFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, model, *params):
        flat, lay = model._ncf_flat, model._ncf_layout
        drop = _dropout_layout(model)
        if drop is None:
            logits = forward_logits(flat, lay, rows, ws_owner=model)
        else:
            logits = _dropout_logits(model, rows, drop)
        ctx.model = model
        ctx.drop = drop
        ctx.save_for_backward(rows)
        return logits

    @staticmethod
    def backward(ctx, grad_out):
        (rows,) = ctx.saved_tensors
        model = ctx.model
        flat, lay = model._ncf_flat, model._ncf_layout
        if ctx.drop is not None:
            lay = ctx.drop[0]
        dev = flat.device
        gflat = torch.zeros(int(lay.total), dtype=torch.float32, device=dev)
        ws = new_workspace(lay, rows.numel(), dev)
        ctl = new_ctl(rows.numel(), dev, adam_t=ctx.drop[1] if ctx.drop is not None else 0)
        dlogit = grad_out.contiguous().to(torch.float32)
        fused_backward(flat, lay, rows, dlogit, gflat, ws, ctl)
        grads = []
        for (p, off), act in zip(_segments(model, lay), active_mask(model)):
            grads.append(gflat[off:off + p.numel()].view_as(p) if act and p.requires_grad else None)
        return (None, None, *grads)


def ncf_forward(model, user, item):
    flat, lay = ensure_flat(model)
    dev = flat.device
    u = _as_i32(user, dev).view(-1)
    i = _as_i32(item, dev).view(-1)
    if u.numel() != i.numel():
        raise ValueError("user and item must have the same number of elements")
    check_id_range((u, model.user_num, None), (i, model.item_num, None))  # as nn.Embedding (models.py:98-103)
    rows = pack_rows(u, i)
    if torch.is_grad_enabled() and any(p.requires_grad for p in model.ordered_params()):
        return _NCFFunction.apply(rows, model, *model.ordered_params())
    drop = _dropout_layout(model)  # train mode: nn.Dropout applies under no_grad too
    if drop is not None:
        return _dropout_logits(model, rows, drop)
    return forward_logits(flat, lay, rows, ws_owner=model)


# ---------------------------------------------------------------------------
# Full-catalogue top-K recommendation (include/ncf_hip.h ncf_recommend, ABI 20)
MAX_TOP_K = 128  # ncf_recommend's limit


class SeenCSR(collections.namedtuple("SeenCSR", "ptr items")):
    """Items to leave out per user: ptr int64 [user_num + 1] indexed by user id, items
    int32, ascending and unique inside a user (the seen_ptr / seen_items of ncf_recommend)."""
    __slots__ = ()


def _is_dok(x):
    return hasattr(x, "keys") and hasattr(x, "shape") and not isinstance(x, (np.ndarray, torch.Tensor))


def seen_csr(users, items=None, user_num=None, device=None, item_num=None):
    """SeenCSR of the (user, item) pairs: sorted, de-duplicated, range-checked
    (IndexError on a user id outside [0, user_num) or an item id outside [0, item_num)).
    `users` may also be the scipy DOK ``train_mat`` that ``load_all`` returns (its keys
    are the pairs; user_num / item_num default to its shape)."""
    if _is_dok(users):
        mat = users
        ks = np.array(list(mat.keys()), dtype=np.int64).reshape(-1, 2)
        u, i = ks[:, 0], ks[:, 1]
        if user_num is None:
            user_num = int(mat.shape[0])
        if item_num is None:
            item_num = int(mat.shape[1])
    else:
        if items is None:
            raise ValueError("seen_csr: items is required with user / item arrays")
        u = np.asarray(users.cpu() if isinstance(users, torch.Tensor) else users).astype(np.int64).reshape(-1)
        i = np.asarray(items.cpu() if isinstance(items, torch.Tensor) else items).astype(np.int64).reshape(-1)
        if u.size != i.size:
            raise ValueError("seen_csr: users and items must have equal length")
    if user_num is None:
        raise ValueError("seen_csr: user_num is required")
    user_num = int(user_num)
    if u.size and (int(u.min()) < 0 or int(u.max()) >= user_num):
        raise IndexError("index out of range in self (user id)")
    hi = (1 << 31) - 1 if item_num is None else int(item_num)
    if i.size and (int(i.min()) < 0 or int(i.max()) >= hi):
        raise IndexError("index out of range in self (item id)")
    key = np.unique(u * (1 << 32) + i)  # sorted by (user, item), duplicates dropped
    su = key >> 32
    ptr = np.zeros(user_num + 1, dtype=np.int64)
    np.cumsum(np.bincount(su, minlength=user_num), out=ptr[1:])
    dev = torch.device("cpu") if device is None else torch.device(device)
    return SeenCSR(torch.from_numpy(ptr).to(dev), torch.from_numpy((key & 0xFFFFFFFF).astype(np.int32)).to(dev))


def as_seen(exclude, model, device):
    """None, a SeenCSR, a DOK matrix or a (users, items) pair -> SeenCSR on `device` (or None)."""
    if exclude is None:
        return None
    if isinstance(exclude, SeenCSR):
        if exclude.ptr.numel() != model.user_num + 1 or exclude.ptr.dtype != torch.int64 \
                or exclude.items.dtype != torch.int32:
            raise ValueError("exclude: SeenCSR needs ptr int64 [user_num + 1] and int32 items")
        return SeenCSR(exclude.ptr.to(device).contiguous(), exclude.items.to(device).contiguous())
    if _is_dok(exclude):
        return seen_csr(exclude, None, model.user_num, device, model.item_num)
    u, i = exclude
    return seen_csr(u, i, model.user_num, device, model.item_num)


def check_top_k(k):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_TOP_K:
        raise ValueError(f"top-k must be an integer in [1, {MAX_TOP_K}], got {k!r}")
    return int(k)


def _recommend_materialised():
    """Tests: ncf_recommend through its materialised path whatever the shape."""
    return _forced_path("recommend")


def recommend_into(flat, lay, users_i32, k, seen, items_out, scores_out, ws):
    """One ncf_recommend call on the current stream into preallocated tensors
    (capturable: nothing is allocated or synchronised)."""
    dev = flat.device
    L.check(L.hip().ncf_recommend(L.ctypes.byref(lay), flat.data_ptr(), users_i32.data_ptr(), users_i32.numel(), k,
                                  None if seen is None else seen.ptr.data_ptr(),
                                  None if seen is None else seen.items.data_ptr(),
                                  items_out.data_ptr(), scores_out.data_ptr(), *_ws_args(ws), L.stream_ptr(dev)),
            "ncf_recommend")


def recommend_workspace(lay, n_users, k, owner, dev):
    return _serve_ws("recommend", "_ncf_rec_ws", lay, owner, dev, n_users, k)


def recommend(model, users, k, seen=None):
    """(items int32 [Q, k], scores float32 [Q, k]) of a HIP-resident model: the k best
    items of every queried user over the whole catalogue, score descending then item id
    ascending, `seen` (a SeenCSR on the device) left out, -1 / -inf in unfilled slots."""
    k = check_top_k(k)
    flat, lay = ensure_flat(model)
    dev = flat.device
    u = _as_i32(users, dev).view(-1)
    q = u.numel()
    items = torch.empty((q, k), dtype=torch.int32, device=dev)
    scores = torch.empty((q, k), dtype=torch.float32, device=dev)
    if q == 0:
        return items, scores
    check_id_range((u, model.user_num, "user"))
    ws = recommend_workspace(lay, q, k, model, dev)
    recommend_into(flat, lay, u, k, seen, items, scores, ws)
    return items, scores


# ---------------------------------------------------------------------------
# nearest neighbours over the embedding tables (ncf_neighbors; added within ABI 21)
SIDES = {"user": L.SIDE_USER, "item": L.SIDE_ITEM}
SPACES = {"gmf": L.SPACE_GMF, "mlp": L.SPACE_MLP, "concat": L.SPACE_CONCAT}
METRICS = {"cosine": L.SIM_COSINE, "dot": L.SIM_DOT}


def default_space(model_type):
    """The space a model of this type scores with: its own tables."""
    return {"GMF": "gmf", "MLP": "mlp"}.get(model_type, "concat")


def neighbor_codes(model_type, side, space, metric):
    """(side, space, metric) names -> the C ABI's codes; ValueError for an unknown one."""
    if space is None:
        space = default_space(model_type)
    for what, value, table in (("side", side, SIDES), ("space", space, SPACES), ("metric", metric, METRICS)):
        if not isinstance(value, str) or value not in table:
            raise ValueError(f"unknown {what} {value!r}: one of {sorted(table)}")
    return SIDES[side], SPACES[space], METRICS[metric]


def neighbors_workspace(lay, side, space, n_queries, k, owner, dev):
    return _serve_ws("neighbors", "_ncf_nb_ws", lay, owner, dev, side, space, n_queries, k)


def neighbors_into(flat, lay, side, space, metric, q_i32, k, exclude_self, ids_out, scores_out, ws):
    """One ncf_neighbors call on the current stream into preallocated tensors
    (capturable: nothing is allocated or synchronised)."""
    L.check(L.hip().ncf_neighbors(L.ctypes.byref(lay), flat.data_ptr(), int(side), int(space), int(metric),
                                  q_i32.data_ptr(), q_i32.numel(), int(k), 1 if exclude_self else 0,
                                  ids_out.data_ptr(), scores_out.data_ptr(), *_ws_args(ws),
                                  L.stream_ptr(flat.device)), "ncf_neighbors")


def neighbors(model, side, queries, k, space=None, metric="cosine", exclude_self=True):
    """(ids int32 [Q, k], scores float32 [Q, k]) of a HIP-resident model: the k rows of
    the `side` ("item" / "user") embedding table most similar to every queried row, score
    descending then id ascending, -1 / -inf in unfilled slots.  `space`: "gmf", "mlp" or
    "concat" (None: default_space(model.model_type)); `metric`: "cosine" or "dot"."""
    k = check_top_k(k)
    side_c, space_c, metric_c = neighbor_codes(model.model_type, side, space, metric)
    flat, lay = ensure_flat(model)
    dev = flat.device
    q = _as_i32(queries, dev).view(-1)
    n = q.numel()
    ids = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n == 0:
        return ids, scores
    check_id_range((q, model.item_num if side == "item" else model.user_num, side))
    ws = neighbors_workspace(lay, side_c, space_c, n, k, model, dev)
    neighbors_into(flat, lay, side_c, space_c, metric_c, q, k, exclude_self, ids, scores, ws)
    return ids, scores


# ---------------------------------------------------------------------------
# dynamic negative sampling: the hardest of m candidates per positive (ncf_select_negatives;
# added within ABI 21)
MAX_CANDIDATES = 64  # ncf_select_negatives' limit on m


class HardNegatives(collections.namedtuple("HardNegatives", "items slots scores")):
    """Result of NCF.hardest_negatives: per group the chosen item id, its slot j in the
    group and its logit."""
    __slots__ = ()


def check_candidates(m):
    if isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= MAX_CANDIDATES:
        raise ValueError(f"candidates per positive must be an integer in [1, {MAX_CANDIDATES}], got {m!r}")
    return int(m)


def _select_materialised():
    """Tests: ncf_select_negatives through its materialised path whatever the shape."""
    return _forced_path("select")


def select_negatives_workspace(lay, n, m, owner, dev):
    return _serve_ws("select_negatives", "_ncf_sel_ws", lay, owner, dev, n, m)


def select_negatives_into(flat, lay, users_i32, cand_i32, m, neg_out, slot_out, score_out, ws):
    """One ncf_select_negatives call on the current stream into preallocated tensors
    (capturable: nothing is allocated or synchronised).  users_i32 [n], cand_i32 [n * m]
    (group p = cand[p * m .. p * m + m)); slot_out / score_out may be None."""
    L.check(L.hip().ncf_select_negatives(L.ctypes.byref(lay), flat.data_ptr(), users_i32.data_ptr(),
                                         cand_i32.data_ptr(), users_i32.numel(), int(m), neg_out.data_ptr(),
                                         L.ptr(slot_out), L.ptr(score_out), *_ws_args(ws),
                                         L.stream_ptr(flat.device)), "ncf_select_negatives")


def check_candidate_shape(users, candidates):
    """(n, m) of users [n] and candidates [n, m]; ValueError for any other shape or a bad m."""
    if candidates.dim() != 2 or users.dim() != 1 or candidates.shape[0] != users.shape[0]:
        raise ValueError("hardest negatives: users [n] and candidates [n, m]")
    return int(users.shape[0]), check_candidates(int(candidates.shape[1]))


def select_negatives(model, users, candidates):
    """HardNegatives (items int32 [n], slots int32 [n], scores float32 [n]) of a HIP-resident
    model: per row the candidate with the highest eval-mode logit, equal scores to the
    lowest slot."""
    flat, lay = ensure_flat(model)
    dev = flat.device
    u = _as_i32(users, dev)
    c = _as_i32(candidates, dev)
    n, m = check_candidate_shape(u, c)
    items = torch.empty(n, dtype=torch.int32, device=dev)
    slots = torch.empty(n, dtype=torch.int32, device=dev)
    scores = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return HardNegatives(items, slots, scores)
    check_id_range((u, model.user_num, "user"), (c, model.item_num, "item"))
    ws = select_negatives_workspace(lay, n, m, model, dev)
    select_negatives_into(flat, lay, u, c.view(-1), m, items, slots, scores, ws)
    return HardNegatives(items, slots, scores)


# ---------------------------------------------------------------------------
# candidate ranking: top-K over caller-supplied item lists (ncf_rank_candidates; added within ABI 21)
class CandidateLists(collections.namedtuple("CandidateLists", "ptr items")):
    """Candidate lists of n queried users: ptr int64 [n + 1] (ascending, ptr[0] = 0,
    ptr[n] = len(items)), items int32; user q's list is items[ptr[q] .. ptr[q + 1]), and a
    candidate's slot is its position inside its own list."""
    __slots__ = ()


class Ranked(collections.namedtuple("Ranked", "items slots scores")):
    """Result of NCF.rank: per list the k best candidates' item ids, their slots in the list
    and their logits, [n, k] each; -1 / -1 / -inf beyond the list's length."""
    __slots__ = ()


def candidate_lists(lists, n_users=None, device=None):
    """CandidateLists from a CandidateLists (returned as it is), a sequence of per-user id
    sequences (ragged), a 2-D [n, m] array (one fixed-length list per row) or a 1-D array
    (one shared list for each of the `n_users` queried users).  ValueError for any other shape."""
    if isinstance(lists, CandidateLists):
        return lists
    dev = torch.device("cpu") if device is None else torch.device(device)
    if isinstance(lists, (list, tuple)) and any(np.ndim(x) > 0 or isinstance(x, (list, tuple)) for x in lists):
        rows = [np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x).reshape(-1) for x in lists]
        ptr = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rows], out=ptr[1:])
        flat = np.concatenate(rows) if rows else np.zeros(0)
        return CandidateLists(torch.from_numpy(ptr).to(dev), torch.from_numpy(flat.astype(np.int64)).to(dev))
    c = torch.as_tensor(lists)
    if c.dim() == 2:
        n, m = c.shape
        ptr = torch.arange(n + 1, dtype=torch.int64) * m
        return CandidateLists(ptr.to(dev), c.reshape(-1).to(dev))
    if c.dim() == 1:
        if n_users is None:
            raise ValueError("candidate_lists: a shared 1-D list needs n_users")
        n, m = int(n_users), c.numel()
        ptr = torch.arange(n + 1, dtype=torch.int64) * m
        return CandidateLists(ptr.to(dev), c.repeat(n).to(dev))
    raise ValueError("candidates: a CandidateLists, a sequence of lists, a 2-D [n, m] array or a 1-D shared list")


def check_rank_args(users, cands, user_num, item_num):
    """(n_lists, n_cand) of users [n] and a CandidateLists: ValueError for a bad shape or dtype, a
    non-monotone ptr or a users / ptr length mismatch, IndexError for an id outside the tables."""
    if users.dim() != 1:
        raise ValueError("rank: users [n]")
    n = int(users.numel())
    ptr, items = cands.ptr, cands.items
    if ptr.dim() != 1 or items.dim() != 1 or ptr.dtype != torch.int64 or items.dtype.is_floating_point:
        raise ValueError("rank: CandidateLists needs ptr int64 [n + 1] and integer items")
    if ptr.numel() != n + 1:
        raise ValueError(f"rank: {n} users but ptr has {ptr.numel()} entries (n + 1 expected)")
    check_csr_ptr(ptr, items.numel(), "rank: ptr must ascend from 0 to len(items)")
    check_id_range((users, user_num, "user"), (items, item_num, "item"))
    return n, int(items.numel())


def _rank_materialised():
    """Tests: ncf_rank_candidates through its materialised path whatever the shape."""
    return _forced_path("rank")


def rank_workspace(lay, n_lists, n_cand, k, owner, dev):
    return _serve_ws("rank_candidates", "_ncf_rank_ws", lay, owner, dev, n_lists, n_cand, k)


def rank_into(flat, lay, users_i32, ptr_i64, cand_i32, k, items_out, slots_out, scores_out, ws):
    """One ncf_rank_candidates call on the current stream into preallocated tensors
    (capturable: nothing is allocated or synchronised).  users_i32 [n], ptr_i64 [n + 1],
    cand_i32 [ptr[n]]; outputs [n, k]; slots_out may be None."""
    L.check(L.hip().ncf_rank_candidates(L.ctypes.byref(lay), flat.data_ptr(), users_i32.data_ptr(),
                                        ptr_i64.data_ptr(), cand_i32.data_ptr(), users_i32.numel(),
                                        cand_i32.numel(), int(k), items_out.data_ptr(), L.ptr(slots_out),
                                        scores_out.data_ptr(), *_ws_args(ws), L.stream_ptr(flat.device)),
            "ncf_rank_candidates")


def rank_candidates(model, users, cands, k):
    """Ranked (items int32 [n, k], slots int32 [n, k], scores float32 [n, k]) of a HIP-resident
    model: the k best candidates of every list, score descending then slot ascending."""
    k = check_top_k(k)
    flat, lay = ensure_flat(model)
    dev = flat.device
    u = _as_i32(users, dev)
    cands = candidate_lists(cands, n_users=u.numel(), device=dev)
    ptr = torch.as_tensor(cands.ptr, device=dev).contiguous()
    n, n_cand = check_rank_args(u, CandidateLists(ptr, cands.items), model.user_num, model.item_num)
    c = _as_i32(cands.items, dev)
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    slots = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n == 0:
        return Ranked(items, slots, scores)
    ws = rank_workspace(lay, n, n_cand, k, model, dev)
    rank_into(flat, lay, u, ptr, c, k, items, slots, scores, ws)
    return Ranked(items, slots, scores)


# ---------------------------------------------------------------------------
# target ranks: exact full-catalogue positions of given items (ncf_target_ranks; added within ABI 21)
class TargetRanks(collections.namedtuple("TargetRanks", "ranks scores ptr eligible")):
    """Result of NCF.target_ranks: per target its 0-based position in the user's full-catalogue
    order and its logit (flat, in the order of the targets, or shaped like an array input);
    ptr int64 [n + 1] cuts the flat order into the n lists; eligible int64 [n] is what each
    list's ranks are out of: item_num minus the user's seen items."""
    __slots__ = ()


def check_target_args(users, lists, user_num, item_num):
    """(n_lists, n_tgt) of users [n] and a CandidateLists of targets: check_rank_args' errors
    (two host reads)."""
    try:
        return check_rank_args(users, lists, user_num, item_num)
    except ValueError as e:
        raise ValueError(str(e).replace("rank:", "target_ranks:")) from None


def eligible_counts(users, seen, item_num):
    """int64 [n]: item_num - len(seen(users[q])), computed where `users` lives (no host read)."""
    u = users.to(torch.int64)
    if seen is None:
        return torch.full_like(u, int(item_num))
    return int(item_num) - (seen.ptr[u + 1] - seen.ptr[u])


def _target_materialised():
    """Tests: ncf_target_ranks through its materialised path whatever the shape."""
    return _forced_path("target")


def target_ranks_workspace(lay, n_lists, n_tgt, owner, dev):
    return _serve_ws("target_ranks", "_ncf_target_ws", lay, owner, dev, n_lists, n_tgt)


def target_ranks_into(flat, lay, users_i32, ptr_i64, tgt_i32, seen, ranks_out, scores_out, ws):
    """One ncf_target_ranks call on the current stream into preallocated tensors (capturable:
    nothing is allocated or synchronised).  users_i32 [n], ptr_i64 [n + 1], tgt_i32 [ptr[n]];
    ranks_out int32 and scores_out float32 [ptr[n]]; scores_out may be None."""
    L.check(L.hip().ncf_target_ranks(L.ctypes.byref(lay), flat.data_ptr(), users_i32.data_ptr(),
                                     ptr_i64.data_ptr(), tgt_i32.data_ptr(), users_i32.numel(), tgt_i32.numel(),
                                     None if seen is None else seen.ptr.data_ptr(),
                                     None if seen is None else seen.items.data_ptr(),
                                     ranks_out.data_ptr(), L.ptr(scores_out), *_ws_args(ws),
                                     L.stream_ptr(flat.device)),
            "ncf_target_ranks")


def target_ranks(model, users, targets, seen=None):
    """TargetRanks (ranks int32 [E], scores float32 [E], ptr, eligible) of a HIP-resident model:
    for every target of every list its position in the user's order over the whole catalogue
    (score descending, item id ascending), `seen` (a SeenCSR on the device) left out."""
    flat, lay = ensure_flat(model)
    dev = flat.device
    u = _as_i32(users, dev)
    lists = candidate_lists(targets, n_users=u.numel(), device=dev)
    ptr = torch.as_tensor(lists.ptr, device=dev).contiguous()
    n, n_tgt = check_target_args(u, CandidateLists(ptr, lists.items), model.user_num, model.item_num)
    t = _as_i32(lists.items, dev)
    ranks = torch.empty(n_tgt, dtype=torch.int32, device=dev)
    scores = torch.empty(n_tgt, dtype=torch.float32, device=dev)
    eligible = eligible_counts(u, seen, model.item_num)
    if n and n_tgt:
        ws = target_ranks_workspace(lay, n, n_tgt, model, dev)
        target_ranks_into(flat, lay, u, ptr, t, seen, ranks, scores, ws)
    return TargetRanks(ranks, scores, ptr, eligible)


# ---------------------------------------------------------------------------
# fold-in: vectors for unseen users from their interaction lists (ncf_fold_in; added within ABI 21)
class FoldExamples(collections.namedtuple("FoldExamples", "ptr items labels")):
    """Examples of Q folded users: ptr int64 [Q + 1], items int32 [E], labels float32 [E]
    in [0, 1]; user q owns the examples ptr[q] .. ptr[q + 1], in that order."""
    __slots__ = ()


class FoldState(collections.namedtuple("FoldState", "exp_avg exp_avg_sq step")):
    """Adam state of folded users: exp_avg / exp_avg_sq float32 [Q, f + dm] over (gmf | mlp),
    step = the optimizer steps taken so far."""
    __slots__ = ()


class FoldedUsers(collections.namedtuple("FoldedUsers", "gmf mlp loss state")):
    """Result of NCF.fold_in: gmf [Q, f], mlp [Q, dm], loss [Q, steps] (the loss at the
    vectors before each step's update) and the FoldState to continue from."""
    __slots__ = ()


def _np_i64(x):
    return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x).astype(np.int64).reshape(-1)


def _histories(histories):
    """list of item-id sequences / (users, items) pair / SeenCSR -> list of int64 arrays.
    A pair groups the items by user id 0 .. max(users), each user's in order of appearance."""
    if isinstance(histories, SeenCSR):
        ptr, items = _np_i64(histories.ptr), _np_i64(histories.items)
        return [items[ptr[q]:ptr[q + 1]] for q in range(len(ptr) - 1)]
    if isinstance(histories, tuple) and len(histories) == 2:
        u, i = _np_i64(histories[0]), _np_i64(histories[1])
        if u.size != i.size:
            raise ValueError("fold_examples: users and items must have equal length")
        if u.size and int(u.min()) < 0:
            raise IndexError("index out of range in self (user id)")
        q = int(u.max()) + 1 if u.size else 0
        order = np.argsort(u, kind="stable")
        cuts = np.cumsum(np.bincount(u, minlength=q))[:-1] if q else []
        return list(np.split(i[order], cuts)) if q else []
    return [_np_i64(h) for h in histories]


def fold_examples(histories, item_num, num_ng=4, generator=None):
    """FoldExamples (CPU tensors) of the users' interaction lists: per user the given items
    as positives (label 1), then num_ng * len negatives (label 0) drawn uniformly from the
    items not in that user's list with a CPU torch.Generator (None: the default one).
    `histories`: a list of item-id sequences, a (users, items) pair of arrays (user ids
    0 .. max) or a SeenCSR.  ValueError if a list covers the catalogue."""
    item_num, num_ng = int(item_num), int(num_ng)
    if num_ng < 0:
        raise ValueError("fold_examples: num_ng must be >= 0")
    ptr, items, labels = [0], [], []
    for h in _histories(histories):
        if h.size and (int(h.min()) < 0 or int(h.max()) >= item_num):
            raise IndexError("index out of range in self (item id)")
        members = np.unique(h)
        free = item_num - members.size
        if free <= 0:
            raise ValueError("fold_examples: an interaction list covers the whole catalogue")
        n_neg = num_ng * h.size
        r = torch.randint(0, free, (n_neg,), generator=generator, dtype=torch.int64).numpy()
        # the r-th item that is not a member: members m_j shift every rank >= m_j - j by one
        neg = r + np.searchsorted(members - np.arange(members.size), r, side="right")
        items += [h, neg]
        labels += [np.ones(h.size, np.float32), np.zeros(n_neg, np.float32)]
        ptr.append(ptr[-1] + h.size + n_neg)
    cat = np.concatenate(items).astype(np.int32) if items else np.zeros(0, np.int32)
    lab = np.concatenate(labels) if labels else np.zeros(0, np.float32)
    return FoldExamples(torch.from_numpy(np.asarray(ptr, dtype=np.int64)), torch.from_numpy(cat),
                        torch.from_numpy(lab))


def check_fold_examples(ex, item_num):
    """FoldExamples with the right dtypes and contents (ValueError / IndexError otherwise)."""
    ptr = torch.as_tensor(ex.ptr).to(torch.int64).view(-1)
    items = torch.as_tensor(ex.items).view(-1)
    labels = torch.as_tensor(ex.labels).to(torch.float32).view(-1)
    if ptr.numel() < 1 or items.numel() != labels.numel():
        raise ValueError("fold-in examples: ptr needs Q + 1 entries, items and labels equal length")
    check_csr_ptr(ptr, items.numel(), "fold-in examples: ptr must ascend from 0 to the number of examples")
    check_id_range((items, item_num, "item"))
    if items.numel() and (float(labels.min()) < 0.0 or float(labels.max()) > 1.0 or bool(torch.isnan(labels).any())):
        raise ValueError("fold-in examples: labels must lie in [0, 1]")
    return FoldExamples(ptr, items.to(torch.int32), labels)


def check_fold_steps(steps):
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
        raise ValueError(f"fold-in steps must be an integer >= 1, got {steps!r}")
    return int(steps)


def fold_opt(steps, lr, betas, eps, weight_decay, t0=0):
    return L.NcfFoldOpt(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(steps),
                        int(t0))


def _fold_generic():
    """Tests: ncf_fold_in through its generic path whatever the shape."""
    return _forced_path("fold")


def fold_in_workspace(lay, n_users, n_examples, steps, owner, dev):
    return _serve_ws("fold_in", "_ncf_fold_ws", lay, owner, dev, n_users, n_examples, steps)


def fold_in_into(flat, lay, ex, gmf, mlp, exp_avg, exp_avg_sq, opt, loss_out, grad_out, ws):
    """One ncf_fold_in call on the current stream, in place on gmf / mlp (and the Adam
    state, if given) with preallocated outputs (capturable: nothing is allocated or
    synchronised).  `ex`: FoldExamples on the device; `opt`: fold_opt(...)."""
    L.check(L.hip().ncf_fold_in(L.ctypes.byref(lay), flat.data_ptr(), ex.ptr.data_ptr(), L.ptr(ex.items) or None,
                                L.ptr(ex.labels) or None, ex.ptr.numel() - 1, ex.items.numel(),
                                gmf.data_ptr(), mlp.data_ptr(), L.ptr(exp_avg), L.ptr(exp_avg_sq),
                                L.ctypes.byref(opt), L.ptr(loss_out), L.ptr(grad_out), *_ws_args(ws),
                                L.stream_ptr(flat.device)), "ncf_fold_in")


def fold_in(model, ex, gmf0, mlp0, steps, lr, betas, eps, weight_decay, state=None, grad_out=None):
    """FoldedUsers of a HIP-resident model from checked examples and start vectors
    (copied, not modified)."""
    flat, lay = ensure_flat(model)
    dev = flat.device
    ex = FoldExamples(ex.ptr.to(dev).contiguous(), ex.items.to(dev).contiguous(), ex.labels.to(dev).contiguous())
    q = ex.ptr.numel() - 1
    gmf = gmf0.to(device=dev, dtype=torch.float32).clone().contiguous()
    mlp = mlp0.to(device=dev, dtype=torch.float32).clone().contiguous()
    width = gmf.shape[1] + mlp.shape[1]
    if state is None:
        m = torch.zeros((q, width), dtype=torch.float32, device=dev)
        v = torch.zeros((q, width), dtype=torch.float32, device=dev)
        t0 = 0
    else:
        m = state.exp_avg.to(device=dev, dtype=torch.float32).clone().contiguous()
        v = state.exp_avg_sq.to(device=dev, dtype=torch.float32).clone().contiguous()
        t0 = int(state.step)
        if m.shape != (q, width) or v.shape != (q, width) or t0 < 0:
            raise ValueError("fold-in state: exp_avg / exp_avg_sq must be [Q, f + dm] and step >= 0")
    loss = torch.zeros((q, steps), dtype=torch.float32, device=dev)
    if q:
        ws = fold_in_workspace(lay, q, ex.items.numel(), steps, model, dev)
        fold_in_into(flat, lay, ex, gmf, mlp, m, v, fold_opt(steps, lr, betas, eps, weight_decay, t0), loss, grad_out,
                     ws)
    return FoldedUsers(gmf, mlp, loss, FoldState(m, v, t0 + steps))
