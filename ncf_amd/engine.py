"""Device-resident NeuMF training engine (the fast path behind ``Trainer.fit``).

One optimizer step over one global batch is a few launches on the current stream, with no host
synchronisation and no per-step allocation, so steps are captured into hipGraphs and replayed
(``run``).  ``ncf_train_step`` is the fused gather / GMF / MFMA tower fwd / BCE / MFMA tower bwd /
embedding scatter-add (models.py:97-118, train_neumf.py:111-114; on the factored path it also
launches the expansion).  What follows it (launch tables: tests/test_gpu_engine_launch_order.py):

  single process with Adam -- the fused optimizer forms, in this file:
    dense     ncf_train_step, ncf_reduce_adam_step (slab reduction + dense Adam + grad zeroing +
              loss bookkeeping, train_neumf.py:90,115)
    deferred  ncf_train_step, ncf_lazy_adam_step; ncf_lazy_adam_flush when run() ends
    in-step   ncf_train_step_ais (the previous step's Adam inside it), ncf_ais_bump; a k-step graph
              is k launches and one bump; ncf_ais_begin before the first, ncf_ais_flush when run() ends
  otherwise -- exchange.py, one class per dp_mode: compute | exchange | optimize | finish
    single    ncf_train_step, ncf_reduce_slab | -- | ncf_adam_step or ncf_sgd_step | --
    allreduce as single | all-reduce of the flat gradient | as single | --
    zero1     as single | reduce-scatter | ncf_adam_step_fact, or ncf_zero_f32 + the dense optimizer,
              on this rank's shard | all-gather of the parameter shards
    touched   ncf_train_step, ncf_touched_pack | all-reduce of the packed rows + tower |
              ncf_lazy_adam_step_packed | --   (ncf_lazy_adam_flush when run() ends)
    owner     ncf_train_step, ncf_owner_pack (this rank's gradient rows bucketed by owner, the tower
              gradient in every bucket) | all-to-all | ncf_owner_adam (the owner sums the W
              contributions in rank order, dense Adam over its rows, tower Adam replicated, the rows
              each rank's next batch reads packed) | all-to-all, ncf_owner_unpack

With the collectives captured (always in a single process; NCF_CAPTURE_ALLREDUCE) one graph is a
whole step and a second one ``graph_steps`` steps; otherwise they are issued from the host
between the graphs of the pieces (exchange.StepGraphs).

Data parallelism: every rank holds the same epoch stream (same seeds, same sampler, same
permutation); rank r processes rows [r*ceil(gb/W), ...) of each global batch, with dlogit scaled by
1/global_batch, so the summed gradient is the single-device mean gradient of ``BCEWithLogitsLoss``.
"""
import ctypes
import os

import torch

from . import _lib as L
from . import distributed as D
from . import exchange as X
from . import ops


def _active_ranges(model, lay, extra=None):
    """Merged [begin, end) float ranges of the parameters that get gradients
    (``extra``: per-parameter mask OR-ed in, e.g. the embedding tables that the
    feature-distillation terms reach)."""
    segs = []
    sizes = [p.numel() for p in model.ordered_params()]
    offs = [lay.ug, lay.ig, lay.um, lay.im]
    for k in range(model.num_layers):
        offs += [lay.w[k], lay.b[k]]
    offs += [lay.wp, lay.bp]
    mask = ops.active_mask(model)
    if extra is not None:
        mask = [a or b for a, b in zip(mask, extra)]
    for off, n, act in zip(offs, sizes, mask):
        if act:
            segs.append([int(off), int(off + (n + 63) // 64 * 64)])
    merged = []
    for b, e in sorted(segs):
        if merged and merged[-1][1] == b:
            merged[-1][1] = e
        else:
            merged.append([b, e])
    return merged


def touched_segments(buf, nb):
    """Host view of an ncf_batch_touched buffer (int32 numpy copy): [b][k] id arrays,
    k = 2 * list + side (lists A, B, C; side 0 users, 1 items) -- include/ncf_hip.h."""
    import numpy as np
    seg = np.ascontiguousarray(buf[:2 * (6 * nb + 1)]).view(np.int64)
    ids = buf[2 * (6 * nb + 1):]
    return [[ids[seg[6 * b + k]:seg[6 * b + k + 1]] for k in range(6)] for b in range(nb)]


class TrainEngine:
    # world > 1 default exchange: one all-reduce + replicated Adam up to this many flat
    # floats, zero1 (reduce-scatter, shard Adam, all-gather: the same wire bytes) above.
    # Sharding saves 7/8 of a 32 B/param Adam pass at W = 8 (~5 ps/param at ~6 TB/s)
    # but costs two more launches and a collective (~16 us per step measured with a
    # one-rank RCCL group, scripts/dp_overhead.py): break-even near 3-4M floats
    # (C3 0.79M: allreduce; C4 13.2M: zero1).
    ALLREDUCE_MAX_FLOATS = 4 << 20

    # dp_mode "auto" (the world > 1 default where deferred Adam applies) resolves at the
    # first epoch stream: "touched" when the packed buffer of a global batch's rows is
    # at most this fraction of the flat gradient, else "allreduce".  Measured per rank
    # at N = 8 on one GPU (scripts/dp_modes.py): at C3 the packed buffer equals the flat
    # gradient (a 65,536-row batch touches every row) and the pack + deferred Adam cost
    # 55.1 us against 43.3 for all-reduce + dense Adam; at C4 it is 0.56 of it and saves
    # 23 MB of wire per step against ~33 us of local work.
    TOUCHED_MAX_FRACTION = 0.8

    @classmethod
    def default_dp_mode(cls, total_floats, touched_ok=False):
        """world > 1: "auto" (touched or allreduce by the global batch, see
        TOUCHED_MAX_FRACTION) where the model supports deferred Adam; else one
        all-reduce up to ALLREDUCE_MAX_FLOATS, zero1 above."""
        if touched_ok:
            return "auto"
        return "allreduce" if total_floats <= cls.ALLREDUCE_MAX_FLOATS else "zero1"

    # dp_mode "auto" picks the owner-sharded exchange from this many ranks up even where
    # a global batch touches every row (C3): two all-to-alls of the touched rows over the
    # point-to-point xGMI links against a ring all-reduce of the whole flat gradient
    # (the projection of DESIGN.md section 6, from per-rank costs measured at emulated
    # N = 2 / 4 / 8); at 2 ranks the all-reduce's one collective wins there
    OWNER_MIN_WORLD = 4

    @classmethod
    def auto_dp_mode(cls, lay, ranges, nranges, batch_size, world=2, owner_ok=False):
        """("owner" | "touched" | "allreduce" | "zero1", packed floats) for dp_mode "auto"
        at this global batch and world: owner (where it applies) when the batch touches
        a small part of the tables (packed buffer <= TOUCHED_MAX_FRACTION of the flat
        gradient, C4) or from OWNER_MIN_WORLD ranks up; else touched where the packed
        buffer is small enough; else the size rule of default_dp_mode (all-reduce up to
        ALLREDUCE_MAX_FLOATS, zero1 above: the optimizer state stays sharded)."""
        pf = int(L.hip().ncf_touched_packed_floats(ctypes.byref(lay), ranges, nranges, int(batch_size)))
        sparse = 0 < pf <= cls.TOUCHED_MAX_FRACTION * int(lay.total)
        if owner_ok and (sparse or int(world) >= cls.OWNER_MIN_WORLD):
            return "owner", pf
        if sparse:
            return "touched", pf
        return cls.default_dp_mode(int(lay.total), touched_ok=False), pf

    def _owner_ok(self):
        """dp_mode "owner" applies: Adam, no distillation, at most 16 ranks, rows of at
        most 1,024 floats (ncf_owner_plan_init) -- touched_ok's other limits."""
        if self.optimizer != "adam" or self.distill is not None or self.world_size > 16:
            return False
        P = L.NcfOwnerPlan()
        return L.hip().ncf_owner_plan_init(ctypes.byref(self.lay), self._ranges, self._nranges, 1, 1,
                                           self.world_size, self.rank, 0, 0, ctypes.byref(P)) == L.NCF_OK

    def _resolve_auto(self, batch_size):
        self.dp_mode, pf = self.auto_dp_mode(self.lay, self._ranges, self._nranges, batch_size, self.world_size,
                                             self._owner_ok())
        self.exchange = X.Touched(self, pf) if self.dp_mode == "touched" else X.MODES[self.dp_mode](self)
        if self.dp_mode == "zero1":
            # the flat buffers were padded to world x shard floats in __init__: keep this rank's moments
            if self.optimizer == "adam":
                r, S = self.rank, self.exchange.shard
                self.exp_avg = self.exp_avg[r * S:(r + 1) * S].clone()
                self.exp_avg_sq = self.exp_avg_sq[r * S:(r + 1) * S].clone()
            self.exchange.tune()
            self._drop_graphs()

    def __init__(self, model, lr=1e-3, optimizer="adam", betas=(0.9, 0.999), eps=1e-8,
                 world_size=1, rank=0, process_group=None, max_batches=1 << 16, dp_mode=None, distill=None,
                 loss="bce"):
        """distill: an ``ncf_amd.distill.DeviceDistillPlan`` -- the student step then
        runs ncf_train_step_kd (teacher logits of the epoch stream computed once per
        epoch by ncf_forward) plus ncf_kd_feature_step for the feature terms.
        loss: "bce" (the reference's BCEWithLogitsLoss, train_neumf.py:86) or "bpr" --
        the pairwise ranking loss over a pair stream (ops.build_pair_stream: rows 2k /
        2k + 1 are (u, i+) / (u, i-)); the step launches NCF_DZ_BPR, batch_size counts
        rows (two per triple).  Single process, no distillation."""
        if loss not in ("bce", "bpr"):
            raise ValueError(f"loss {loss!r}")
        if loss == "bpr" and int(world_size) > 1:
            raise ValueError("loss 'bpr' is single-process: a rank slice of a batch could split a pair")
        if loss == "bpr" and distill is not None:
            raise ValueError("loss 'bpr' does not combine with distillation")
        self.loss = loss
        self._dz = L.DZ_BPR if loss == "bpr" else L.DZ_BCE
        self.model = model
        self.distill = distill
        if process_group is None and int(world_size) > 1:
            # no group given: the collectives run over the default group, so the
            # owner all-gather and the stream agreement check must use it too
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                process_group = dist.group.WORLD
        self.world_size, self.rank, self.group = int(world_size), int(rank), process_group
        lay = L.layout(model.user_num, model.item_num, model.factor_num, model.num_layers, model.model_type)
        touched_ok = (optimizer == "adam" and model.factor_num % 4 == 0 and model.user_num <= (1 << 19)
                      and model.item_num <= (1 << 19))
        if dp_mode is None:
            dp_mode = os.environ.get("NCF_DP_MODE", self.default_dp_mode(int(lay.total), touched_ok)) \
                if self.world_size > 1 else "single"
        # an explicit exchange mode stands at world 1 (a one-rank group still runs the
        # real collectives: how the captured-collective graph is tested on one GPU)
        if dp_mode not in ("single", "zero1", "allreduce", "touched", "auto", "owner"):
            raise ValueError(f"dp_mode {dp_mode!r}")
        if dp_mode in ("touched", "auto", "owner") and not touched_ok:
            raise ValueError(f"dp_mode {dp_mode!r} needs Adam, factor_num % 4 == 0 and tables of <= 2^19 rows")
        if dp_mode == "owner" and (distill is not None or self.world_size > 16):
            raise ValueError("dp_mode 'owner': no distillation, at most 16 ranks")
        self.dp_mode = dp_mode
        # flat buffers padded to world x shard floats where the exchange shards them
        # (rank r owns [r*S, (r+1)*S)); "auto" pads too when its fallback would be zero1
        shards = dp_mode == "zero1" or (
            dp_mode == "auto" and self.default_dp_mode(int(lay.total)) == "zero1")
        n = int(lay.total)
        if shards:
            n = D.shard_floats(int(lay.total), self.world_size) * self.world_size
        self.flat, lay0 = ops.ensure_flat(model, n)
        # the engine's own copy: ncf_layout_tune shapes it for the batch size
        self.lay = type(lay0).from_buffer_copy(lay0)
        # nn.Dropout(p) before every tower Linear (models.py:23): training steps with
        # p > 0 run the layered path, keep masks hashed from (seed, step, layer, row,
        # column) -- include/ncf_hip.h ncf_dropout_hash
        ops.set_dropout(self.lay, model)
        dev = self.flat.device
        self.device = dev
        n = self.flat.numel()
        self.grads = torch.zeros(n, dtype=torch.float32, device=dev)
        self.optimizer = optimizer
        n_opt = D.shard_floats(int(lay.total), self.world_size) if dp_mode == "zero1" else n
        if optimizer == "adam":
            self.exp_avg = torch.zeros(n_opt, dtype=torch.float32, device=dev)
            self.exp_avg_sq = torch.zeros(n_opt, dtype=torch.float32, device=dev)
        elif optimizer != "sgd":
            raise ValueError(optimizer)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.ws = None  # ncf_train_step workspace, sized by set_epoch_stream
        self.ctl = ops.new_ctl(0, dev)
        self._ctl_n = None  # the stream length ctl holds
        rng = _active_ranges(model, self.lay, None if distill is None else distill.active_extra)
        self._ranges = (ctypes.c_int64 * (2 * len(rng)))(*[x for r in rng for x in r])
        self._nranges = len(rng)
        self._range_args = (self._ranges, self._nranges, self.ctl.data_ptr())  # as most launches take them
        self.loss_hist = torch.zeros(max_batches, dtype=torch.float32, device=dev)
        self.rows, self.n_total, self.batch_size = None, 0, None
        # the current stream buffer's exchange.StepGraphs, and those of every stream buffer
        # (the epoch pipeline alternates two): key (batch_size, n_total, rows pointer)
        self._plan = None
        self._graphs = {}
        # other epoch-stream buffers this engine will be handed (same layout as
        # the current one): captured together with it, so a buffer switch at an
        # epoch boundary replays graphs already built
        self.stream_buffers = []
        # ncf_user_order output per epoch-stream buffer (key: pointer, rows)
        self._orders = {}
        self._uses_order = False
        # deferred Adam (ncf_lazy_adam_step): per-row last step, step scalars ring,
        # ncf_batch_touched lists per epoch-stream buffer (key: pointer, rows, batch)
        self.lazy = False
        self._last = self._ring = None
        self._touched_lists = {}
        # in-step Adam: an update is pending (ncf_ais_begin .. ncf_ais_flush); NcfAisBufs, its tensors
        self._ais_live, self._ais_b, self._ais_t = False, None, None
        # stream agreement checks in flight; the first one was awaited
        self._stream_checks, self._stream_checked_once = [], False
        # the exchange mode's step, buffers and state ("auto": resolved at the first stream)
        self.exchange = X.MODES[dp_mode](self)

    # what callers outside name of the exchange (bound here: "auto" replaces the exchange object)
    _ow_plan = property(lambda self: self.exchange.plan)

    def owner_prebuild(self, rows, stream):  # EpochPipeline.on_built (Owner.prebuild; else nothing)
        self.exchange.prebuild(rows, stream)

    def owner_sync(self):  # dp_mode "owner": every owner's rows to every rank (Owner.sync), a collective
        self.exchange.sync()

    # ------------------------------------------------------------------ data
    def set_epoch_stream(self, rows, batch_size, checked=False):
        """Packed int64 rows (ops.pack_rows / ncf_prepare_epoch output) already in
        training order: batch b is rows[b*batch_size, ...).  Ids are range-checked
        once here (IndexError like nn.Embedding) unless the caller already did
        (`checked`, e.g. Trainer on the host arrays)."""
        if rows.dtype != torch.int64 or not rows.is_contiguous() or rows.device != self.device:
            raise ValueError("epoch stream: contiguous int64 packed rows on the engine's device")
        if self.loss == "bpr" and (int(batch_size) % 2 or rows.numel() % 2):
            raise ValueError("loss 'bpr': the stream and every batch hold whole pairs (even row counts)")
        if not checked:
            (ops.check_pair_rows if self.loss == "bpr" else ops.check_rows)(rows, self.model.user_num,
                                                                             self.model.item_num)
        n = rows.numel()
        self.rows = rows
        self.n_total = n
        if self.batch_size != batch_size or self.ws is None:
            self._drop_graphs()
            per = (int(batch_size) + self.world_size - 1) // self.world_size
            # launch shape for this batch size: workgroups = its 128-row tiles (64-row
            # tiles of 4-wave workgroups for small per-rank batches; up to one per CU),
            # per-row layer 0 for batches small against the tables.  NCF_WG_WAVES=4|8
            # forces the workgroup geometry (A/B measurements).
            wg = os.environ.get("NCF_WG_WAVES")
            if wg:
                L.check(L.hip().ncf_debug_set_geometry(int(wg)), "ncf_debug_set_geometry")
            # user store-and-sum (NCF_LAYOUT_USER_STORE, off by default): NCF_USER_STORE=1
            # forces it, =auto applies the per-rank batch rule (A/B)
            pr = os.environ.get("NCF_PER_ROW")  # 0|1: force the layer-0 form (A/B)
            if pr in ("0", "1"):
                L.check(L.hip().ncf_debug_set_per_row(int(pr)), "ncf_debug_set_per_row")
            us = os.environ.get("NCF_USER_STORE")
            if us in ("0", "1", "auto"):
                L.check(L.hip().ncf_debug_set_user_store(-1 if us == "auto" else int(us)), "ncf_debug_set_user_store")
            L.check(L.hip().ncf_layout_tune(ctypes.byref(self.lay), per), "ncf_layout_tune")
            if os.environ.get("NCF_FORCE_LAYERED", "0") == "1":  # A/B: the layered path for any shape
                self.lay.flags |= L.LAYOUT_LAYERED
            self.exchange.tune()
            self.ws = ops.new_workspace(self.lay, per, self.device)
        self.batch_size = int(batch_size)
        if self.num_batches > self.loss_hist.numel():
            # the optimizer launches write loss_hist[b % num_batches]: one slot per
            # batch of the epoch (a captured graph holds the old pointer: re-capture)
            self.loss_hist = torch.zeros(self.num_batches, dtype=torch.float32, device=self.device)
            self._drop_graphs()
        # device-side fills (an assignment from a host scalar is a pageable copy that
        # blocks the host until the stream drains, i.e. until the previous epoch ends)
        if n != self._ctl_n:
            self.ctl[0:4:3].zero_()
            self.ctl[2:3].fill_(n)
            self._ctl_n = n
        else:
            self.ctl[0:1].zero_()
        self._check_stream_agreement(rows)
        if self.dp_mode == "auto":
            self._resolve_auto(batch_size)
        self.exchange.prepare(rows)
        # deferred Adam: touched rows of every batch of this stream (once per epoch)
        lazy = self._lazy_wanted()
        if self.lazy and not lazy:
            self.flush()  # back to dense Adam: every row current first
        if lazy:
            if self._last is None:
                U, I = self.model.user_num, self.model.item_num
                self._last = torch.zeros(U + I, dtype=torch.int32, device=self.device)
                self._ring = torch.zeros(2 * self.LAZY_RING, dtype=torch.float32, device=self.device)
            if not self.lazy:  # rows are current as of the present step
                self.optimizer_state_set()
            L.check(L.hip().ncf_batch_touched(rows.data_ptr(), n, self.batch_size, self.model.user_num,
                                          self.model.item_num, self._touched_buf(rows).data_ptr(),
                                          L.stream_ptr(self.device)), "ncf_batch_touched")
        self.lazy = lazy
        # the rows of each rank slice by user, once per epoch (ncf_user_order): the layered
        # factored layer 0 sums user runs before its atomics; the fused step with
        # NCF_LAYOUT_USER_STORE sums its stored user-side rows over them
        self._uses_order = (os.environ.get("NCF_USER_ORDER", "1") == "1"
                            and bool(L.hip().ncf_uses_user_order(ctypes.byref(self.lay))))
        if self._uses_order:
            L.check(L.hip().ncf_user_order(rows.data_ptr(), n, self.batch_size, self.world_size,
                                           self.model.user_num, self._order_buf(rows).data_ptr(),
                                           L.stream_ptr(self.device)), "ncf_user_order")
        if self.distill is not None:
            # the frozen teacher's logit for every row of the epoch stream (one
            # forward launch per epoch instead of one no_grad forward per step); a new
            # logit buffer (another stream length) invalidates every captured step
            if self.distill.teacher_logits(rows):
                self._drop_graphs()

    def _check_stream_agreement(self, rows):
        """world > 1: every rank must train on the same epoch stream (same seeds, and
        the canonical grouping of ncf_prepare_epoch2): a device checksum of the stream,
        max and -min over the ranks in one all-reduce.  The first stream is checked at
        once; later ones asynchronously (flag copied to pinned memory, read at a later
        epoch boundary when done), so the host does not wait for the running epoch.
        Raises RuntimeError on a mismatch."""
        if self.world_size == 1 or self.group is None:
            return
        import torch.distributed as dist
        if dist.get_world_size(self.group) != self.world_size:
            return  # an emulated world (scripts/dp_modes.py)
        self._poll_stream_checks(block=False)
        c = ops.stream_checksum(rows)
        t = D._all_reduce(torch.stack([c, -c]), self.group, dist.ReduceOp.MAX)
        bad = (t[0] + t[1]) != 0
        flag = torch.empty(1, dtype=torch.bool, pin_memory=True)
        flag.copy_(bad.view(1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._stream_checks.append((flag, ev))
        if not self._stream_checked_once:
            self._stream_checked_once = True
            self._poll_stream_checks(block=True)

    def _poll_stream_checks(self, block):
        keep = []
        for flag, ev in self._stream_checks:
            if block:
                ev.synchronize()
            if not ev.query():
                keep.append((flag, ev))
                continue
            if bool(flag.item()):
                raise RuntimeError("data-parallel ranks hold different epoch streams: build them from the same "
                                   "seeds with the canonical grouping (ncf_prepare_epoch2 NCF_PREP_CANONICAL, "
                                   "ops.EpochPrep(canonical=True) / EpochPipeline(canonical=True))")
        self._stream_checks = keep

    # dp_mode "owner": list slots grow to OWNER_SLACK x the longest list seen (+16, multiples of 16):
    # the exchange chunks keep one size (and the captured graphs stay valid) across epochs
    OWNER_SLACK = 1.08

    def _side_buf(self, cache, rows, batch_keyed, numel, dtype, make=torch.empty, replaced=None):
        """The buffer in `cache` that goes with epoch-stream buffer `rows` (and the batch size),
        made with numel() elements on first use; with `replaced`, again when it is too small."""
        key = (rows.data_ptr(), rows.numel()) + ((self.batch_size,) if batch_keyed else ())
        buf = cache.get(key)
        if buf is None or (replaced is not None and buf.numel() < numel()):
            if buf is not None:
                replaced(buf)
            buf = cache[key] = make(numel(), dtype=dtype, device=self.device)
        return buf

    def _order_buf(self, rows):
        n = rows.numel()  # n int64 entries + n int32 inverse positions (ncf_user_order)
        return self._side_buf(self._orders, rows, False, lambda: n + (n + 1) // 2, torch.int64)

    # deferred Adam: steps a row may sit out are replayed from this ring of step
    # scalars (a row's gap is at most NCF_LAZY_SPAN steps; > 514 entries required)
    LAZY_RING = 1 << 12
    # on by default where it moves fewer bytes than dense Adam: tables with more rows
    # than LAZY_RATIO x the global batch (C2, C4, C5; not C3's ml-1m at 65,536)
    LAZY_RATIO = float(os.environ.get("NCF_LAZY_RATIO", "2"))

    def _lazy_wanted(self):
        """Deferred Adam for this stream (always with dp_mode "touched"): single-process Adam (the fused
        optimizer launch), factor_num % 4 == 0, tables <= 2^19 rows; NCF_LAZY_ADAM=1 turns it on for
        single-process training (auto: tables larger than LAZY_RATIO x the global batch), 0 (the default)
        keeps the dense launch, measured faster on MI355X at C2, C4 and C5."""
        if self.exchange.lazy:
            return True
        env = os.environ.get("NCF_LAZY_ADAM", "0")
        if env == "0" or not self._fused_optimizer:
            return False
        U, I = self.model.user_num, self.model.item_num
        if self.model.factor_num % 4 or U > (1 << 19) or I > (1 << 19):
            return False
        return env == "1" or (U + I) > self.LAZY_RATIO * self.batch_size

    def _touched_buf(self, rows):
        """The ncf_batch_touched lists that go with epoch-stream buffer `rows`."""
        return self._side_buf(self._touched_lists, rows, True, lambda: (int(L.hip().ncf_touched_bytes(
            rows.numel(), self.batch_size, self.model.user_num, self.model.item_num)) + 3) // 4, torch.int32)

    # argument runs the optimizer launches share: layout + parameters, gradients, moments; Adam's
    # scalars; the loss history (loss_hist[b % num_batches]); deferred Adam's lists, per-row last
    # step and ring of step scalars
    _state_args = property(lambda s: (ctypes.byref(s.lay), s.flat.data_ptr(), s.grads.data_ptr(),
                                      s.exp_avg.data_ptr(), s.exp_avg_sq.data_ptr()))
    _adam_args = property(lambda s: (s.lr, s.betas[0], s.betas[1], s.eps))
    _hist_args = property(lambda s: (s.loss_hist.data_ptr(), s.num_batches))
    _lazy_args = property(lambda s: (s._touched_buf(s.rows).data_ptr(), s.n_total, s.batch_size,
                                     s._last.data_ptr(), s._ring.data_ptr(), s.LAZY_RING))

    def flush(self):
        """Deferred Adam: every embedding row brought up to the current step (the parameters and
        moments are then the dense optimizer's).  In-step Adam: the pending update written
        (ncf_ais_flush).  dp_mode "owner": every replica brought up to date.  No-op otherwise."""
        self.exchange.sync()
        if self._ais_live:
            L.check(L.hip().ncf_ais_flush(*self._state_args, ctypes.byref(self._ais_bufs()), *self._range_args,
                                          *self._adam_args, *self._hist_args, L.stream_ptr(self.device)),
                    "ncf_ais_flush")
            self._ais_live = False
        if not self.lazy:
            return
        L.check(L.hip().ncf_lazy_adam_flush(*self._state_args, *self._range_args, *self._adam_args[1:],
                                            self._last.data_ptr(), self._ring.data_ptr(), self.LAZY_RING,
                                            L.stream_ptr(self.device)), "ncf_lazy_adam_flush")

    def optimizer_state_set(self):
        """Call after writing flat / exp_avg / exp_avg_sq / ctl from outside (e.g. a loaded or
        teacher-forced optimizer state): every row is current as of step ctl.adam_t."""
        if self._last is not None:
            self._last.copy_(self.ctl[1:2].to(torch.int32).expand_as(self._last))

    def user_order_ptr(self):
        """ncf_train_step's user_order argument for the current stream (None: unused)."""
        return self._order_buf(self.rows).data_ptr() if self._uses_order else None

    @property
    def num_batches(self):
        return (self.n_total + self.batch_size - 1) // self.batch_size

    # ------------------------------------------------------------------ step
    @property
    def _fused_optimizer(self):
        """Single process + Adam: slab reduction and Adam in one launch (ncf_reduce_adam_step)."""
        return self.exchange.single and self.optimizer == "adam" and os.environ.get("NCF_FUSED_ADAM", "1") == "1"

    # NCF_ADAM_IN_STEP: "auto" (default) -- the in-step optimizer where the step has at most
    # AIS_MAX_WG training workgroups (C5's 256-row batch: 11.7 against 12.0 us/step; at
    # C2's 16 workgroups the on-the-fly update quadruples each CU's gather loads and the
    # step takes 22.7 against 18.4 us, profiles/r05_evidence/ais_ab/); "1" wherever the
    # kernel exists, "0" never
    ADAM_IN_STEP = os.environ.get("NCF_ADAM_IN_STEP", "auto")
    AIS_MAX_WG = int(os.environ.get("NCF_AIS_MAX_WG", "4"))

    @property
    def _ais_active(self):
        """In-step Adam (ABI 18, ncf_train_step_ais): single process, dense Adam, the fused
        small-batch kernel with per-row layer 0; response distillation only (its logits
        ride in the launch, feature terms would add into the gradient separately)."""
        mode = {True: "1", False: "0"}.get(self.ADAM_IN_STEP, self.ADAM_IN_STEP)
        if mode == "0" or not self._fused_optimizer or self.lazy or self.loss == "bpr":
            return False  # (ncf_train_step_ais refuses the pairwise mode)
        if self.distill is not None and self.distill.keys:
            return False
        if not L.hip().ncf_ais_supported(ctypes.byref(self.lay)):
            return False
        if mode == "auto":
            wg = (int(self.lay.flags) >> L.LAYOUT_WG_SHIFT) & L.LAYOUT_WG_MASK
            return 0 < wg <= self.AIS_MAX_WG
        return True

    def _ais_bufs(self):
        if self._ais_b is None:
            n = int(self.lay.total)
            z = lambda: torch.zeros(n, dtype=torch.float32, device=self.device)  # noqa: E731
            self._ais_t = [z() for _ in range(5)] + [torch.zeros(4, dtype=torch.int64, device=self.device)]
            self._ais_b = L.NcfAisBufs(*[t.data_ptr() for t in self._ais_t])
        return self._ais_b

    def _ais_begin(self):
        if self._ais_live:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("in-step Adam: ncf_ais_begin must run before graph capture")
        L.check(L.hip().ncf_ais_begin(*self._state_args, ctypes.byref(self._ais_bufs()), *self._range_args,
                                      L.stream_ptr(self.device)), "ncf_ais_begin")
        self._ais_live = True

    def _ais_launch(self, step_i):
        if self.distill is not None:
            d = self.distill
            dl, dz, kd = d.tlog.data_ptr(), L.DZ_KD, (d.w_task, d.w_resp, d.temperature)
        else:
            dl, dz, kd = None, L.DZ_BCE, (0.0, 0.0, 0.0)
        L.check(L.hip().ncf_train_step_ais(*self._state_args, ctypes.byref(self._ais_bufs()), self._ranges,
                                           self._nranges, self.rows.data_ptr(), dl, self.ctl.data_ptr(),
                                           self.batch_size, dz, *kd, *self._adam_args, *self._hist_args, step_i,
                                           L.stream_ptr(self.device)), "ncf_train_step_ais")

    def _ais_bump(self, k):
        L.check(L.hip().ncf_ais_bump(self.ctl.data_ptr(), ctypes.byref(self._ais_bufs()), k,
                                     L.stream_ptr(self.device)), "ncf_ais_bump")

    def _grad_launch(self):
        """One step's gradients: the student's step (ncf_train_step_kd [+ feature terms]) or ncf_train_step."""
        st = L.stream_ptr(self.device)
        if self.distill is not None:
            self.distill.launch(self, st)
            return
        L.check(L.hip().ncf_train_step(ctypes.byref(self.lay), self.flat.data_ptr(), self.grads.data_ptr(),
                                       self.rows.data_ptr(), self.user_order_ptr(), None, self.ctl.data_ptr(),
                                       self.batch_size, self.world_size, self.rank, self._dz, self.ws.data_ptr(),
                                       self.ws.numel() * 4, None, st), "ncf_train_step")

    def _train_launch(self):
        if self._ais_active:  # one whole step: the previous step's Adam rides in this launch
            self._ais_begin()
            self._ais_launch(0)
            self._ais_bump(1)
            return
        self._grad_launch()

    def _reduce_slab(self):
        """Per-workgroup tower gradients -> flat gradient buffer (advances ctl)."""
        L.check(L.hip().ncf_reduce_slab(ctypes.byref(self.lay), self.ws.data_ptr(), self.grads.data_ptr(),
                                        self.ctl.data_ptr(), L.stream_ptr(self.device)), "ncf_reduce_slab")

    def _reduce_adam(self):
        st = L.stream_ptr(self.device)
        if self._ais_active:  # inside the next training launch (or ncf_ais_flush)
            return
        lay, *state = self._state_args
        name, more = ("ncf_lazy_adam_step", self._lazy_args) if self.lazy else ("ncf_reduce_adam_step", ())
        L.check(getattr(L.hip(), name)(lay, self.ws.data_ptr(), *state, *self._range_args, *self._adam_args,
                                       *self._hist_args, *more, st), name)

    def _step_body(self):
        if self._fused_optimizer:
            self._train_launch()
            self._reduce_adam()
            return
        x = self.exchange
        x.compute()
        x.exchange()
        x.optimize()
        x.finish()

    def time_kernels(self, n_steps):
        """Run n_steps eager steps with HIP events between the launches (on the
        stream they run on) and return mean milliseconds per launch group."""
        st = torch.cuda.current_stream(self.device)
        if self._ais_active:  # one launch per step: the previous step's Adam rides in it
            parts = [("ncf_train_step_ais", self._train_launch)]
        elif self._fused_optimizer:
            parts = [("ncf_train_step", self._train_launch),
                     ("ncf_lazy_adam_step" if self.lazy else "ncf_reduce_adam_step", self._reduce_adam)]
        else:
            parts = self.exchange.timed_parts()
        acc = {k: 0.0 for k, _ in parts}
        evs = []
        self.flush()  # timing starts from current rows (as a fresh epoch would)
        for _ in range(n_steps):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(len(parts) + 1)]
            e[0].record(st)
            for k, (_, fn) in enumerate(parts):
                fn()
                e[k + 1].record(st)
            evs.append(e)
        self.flush()
        torch.cuda.synchronize(self.device)
        for e in evs:
            for k, (name, _) in enumerate(parts):
                acc[name] += e[k].elapsed_time(e[k + 1])
        return {k: v / max(1, n_steps) for k, v in acc.items()}

    def time_train_kernel(self, reps):
        """Mean duration (ms) of the gradient-forming launches of one step -- the
        fused step kernel and, on the factored path, ncf_expand_grads: `reps`
        back-to-back launch groups on the current batch between one HIP event pair
        on the launch stream (per-launch event pairs add several microseconds each).
        The gradient buffer is zeroed afterwards (the launches accumulate into it)."""
        st = torch.cuda.current_stream(self.device)
        self._grad_launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            self._grad_launch()
        e1.record(st)
        torch.cuda.synchronize(self.device)
        self.grads.zero_()
        return e0.elapsed_time(e1) / reps

    def step(self):
        """One optimizer step on global batch ctl.batch (eager launches)."""
        self._step_body()
        if self._ais_live:
            self.flush()  # in-step Adam: the update written now, not in the next launch

    def _graph_of(self, fn):
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                fn()
        torch.cuda.current_stream(self.device).wait_stream(s)
        return g

    # steps unrolled into one graph when the collective is captured too (single
    # process): fewer graph launches, no host work between consecutive steps.
    # NCF_GRAPH_STEPS fixes it; by default the whole epoch for epochs of at most 128
    # steps (C3's 76: 56.6 -> 56.1 us/step against 8 -- no single-step remainder
    # replays), else 32 (C2 19.10 -> 18.42 us, C5 12.57 -> 12.18 us against 8; 128 no
    # better), profiles/r04_evidence/graph_steps_ab.log
    GRAPH_STEPS = int(os.environ.get("NCF_GRAPH_STEPS", "0"))

    @property
    def graph_steps(self):
        return self.GRAPH_STEPS if self.GRAPH_STEPS > 0 else self.num_batches if self.num_batches <= 128 else 32

    def capture(self):
        """Capture the step into hipGraph(s) (after at least one eager step).  dp_mode "owner": if
        capturing the all-to-alls raises, the collectives go eager between graphs from then on
        (Owner.capture_failed warns) instead of failing the run."""
        x, plan = self.exchange, None
        if x.captured:
            try:
                plan = self._capture_whole()
            except RuntimeError as err:
                if not x.capture_failed(err):
                    raise
                torch.cuda.synchronize(self.device)
        if plan is None:
            plan = x.capture_split()
        self._plan = self._graphs[(self.batch_size, self.n_total, self.rows.data_ptr())] = plan
        return plan

    def _capture_whole(self):
        whole, chunk, k = self._graph_of(self._step_body), None, self.graph_steps
        if k > 1:
            if self._ais_active:
                def body():  # k launches, one bump: each launch applies its predecessor's Adam
                    for j in range(k):
                        self._ais_launch(j)
                    self._ais_bump(k)
            else:
                def body():
                    for _ in range(k):
                        self._step_body()
            chunk = self._graph_of(body)
        return X.StepGraphs(whole, chunk, k)

    def _capture_buffers(self):
        """Capture for every registered stream buffer not captured yet (the rows pointer is read at replay)."""
        cur = (self.rows, self._plan)
        try:
            for buf in self.stream_buffers:
                key = (self.batch_size, self.n_total, buf.data_ptr())
                if (buf.numel() != self.n_total or buf.dtype != torch.int64 or buf.device != self.device
                        or key in self._graphs):
                    continue
                self.rows = buf
                # side buffers are allocated outside the capture (filled when the buffer is set)
                if self._uses_order:
                    self._order_buf(buf)
                if self.lazy:
                    self._touched_buf(buf)
                self.exchange.alloc_for(buf)
                self.capture()
        finally:
            self.rows, self._plan = cur

    def _drop_graphs(self):
        self._plan = None
        self._graphs = {}

    def run(self, n_steps, use_graph=True):
        """n_steps consecutive optimizer steps (batches advance on device).  With deferred Adam the
        embedding rows are brought up to the last step at the end (ncf_lazy_adam_flush: a pass over the
        per-row step counters; rows the last batch of an epoch already caught up cost nothing), so the
        parameters are the dense optimizer's whenever run() returns."""
        if self._ais_active:
            self._ais_begin()  # eager: the step graphs may replay without an eager step first
        self._run(n_steps, use_graph)
        self.flush()

    def _run(self, n_steps, use_graph=True):
        if not use_graph:
            for _ in range(n_steps):
                self._step_body()
            return
        left = n_steps
        self._plan = self._graphs.get((self.batch_size, self.n_total, self.rows.data_ptr()))
        if self._plan is None:
            # eager first step also sets kernel attributes outside the capture
            self._step_body()
            left -= 1
            if n_steps <= 1:
                return
            self.capture()  # captured launches are recorded, not executed
            self._capture_buffers()
        g = self._plan
        if g.whole is None:  # collectives from the host between the graphs
            self.exchange.replay(g, left)
            return
        if g.chunk is not None:
            for _ in range(left // g.k):
                g.chunk.replay()
            left %= g.k
        for _ in range(left):
            g.whole.replay()

    def epoch_losses(self):
        """Per-batch mean loss (BCE, or BPR per triple) of the last epoch (host copy); zero1: a collective."""
        return self.exchange.epoch_losses()

    def state_step(self):
        return int(self.ctl[1].item())
