"""Gradient-exchange modes of ``TrainEngine`` (``dp_mode``), one class each: the mode's buffers
and state, and its step ``compute(); exchange(); optimize(); finish()`` (the launches of each:
engine.py's docstring).  ``captured``: the collectives go inside the step graph; otherwise
``capture_split`` captures the pieces between them and ``replay`` runs n steps from those."""
import collections
import ctypes
import os
import weakref

import torch

from . import _lib as L
from . import distributed as D

# The captured graphs of one epoch-stream buffer.  Collectives captured: `whole` is one step,
# `chunk` is `k` steps.  Collectives from the host: `compute` and `optimize` are the halves of a
# step, `chained` what runs between two collectives across a step boundary (optimize + next
# compute; owner: unpack + next compute), `tail` the owner's last unpack.
StepGraphs = collections.namedtuple("StepGraphs", "whole chunk k compute optimize chained tail",
                                    defaults=(None, None, 0, None, None, None, None))


class Single:
    """No exchange: a single process without the fused optimizer (SGD, NCF_FUSED_ADAM=0)."""
    single = True        # the fused single-process optimizer forms may apply
    lazy = False         # deferred Adam, always
    chained = False      # eager collectives: optimize(t) + compute(t + 1) in one graph
    captured = True      # the collectives (none here) inside the step graph
    exchange_name = "allreduce"
    plan = None          # owner: the ncf_owner_plan of the current stream
    fact_shard = False   # zero1: the factored expansion sharded into the optimizer

    def __init__(self, e):
        # no reference cycle: the engine (its captured graphs with it) is freed when its last
        # reference goes, e.g. before the caller destroys the process group the graphs use
        self.e = weakref.proxy(e)
        self.loss_slot = int(e.lay.loss_slot)

    def _nothing(self, *args):
        pass
    # for a mode to fill in: prepare(rows) in set_epoch_stream; prebuild(rows, stream) from
    # EpochPipeline.on_built; alloc_for(rows) side buffers outside a capture; sync() in flush;
    # capture_failed(err): true to capture again, with the collectives from the host
    prepare = prebuild = alloc_for = sync = exchange = finish = capture_failed = _nothing

    def tune(self):
        """After ncf_layout_tune: the layout flags of this mode."""
        self.e.lay.flags &= ~L.LAYOUT_FACT_DEFER_DX

    def compute(self):
        self.e._train_launch()
        self.e._reduce_slab()

    def optimize(self):
        e = self.e
        self._dense(e.flat.data_ptr(), e.grads.data_ptr(), e._ranges, e._nranges, e.loss_hist.data_ptr())

    def _dense(self, p, g, ranges, nr, hist):
        """Dense Adam / SGD over `ranges` + grad zeroing + loss bookkeeping."""
        e, st = self.e, L.stream_ptr(self.e.device)
        if e.optimizer == "adam":
            L.check(L.hip().ncf_adam_step(p, g, e.exp_avg.data_ptr(), e.exp_avg_sq.data_ptr(), ranges, nr,
                                          e.ctl.data_ptr(), *e._adam_args, self.loss_slot, hist, e.num_batches, st),
                    "ncf_adam_step")
        else:
            L.check(L.hip().ncf_sgd_step(p, g, ranges, nr, e.ctl.data_ptr(), e.lr, self.loss_slot, hist,
                                         e.num_batches, st), "ncf_sgd_step")

    def timed_parts(self):
        """time_kernels: (key, launch) per launch group of a step."""
        return [("ncf_train_step", self.e._train_launch), ("ncf_reduce_slab", self.e._reduce_slab),
                (self.exchange_name, self.exchange), ("optimizer", self.optimize)]

    def capture_split(self):
        def opt_compute():
            self.optimize()
            self.compute()
        g = self.e._graph_of
        return StepGraphs(compute=g(self.compute), optimize=g(self.optimize),
                          chained=g(opt_compute) if self.chained else None)

    def replay(self, g, n):
        """n steps from capture_split's graphs, the collectives from the host."""
        if g.chained is not None and n >= 2:
            # compute(t0), [optimize(t), compute(t+1)] per step, the last optimize: one replay per step
            g.compute.replay()
            self.exchange()
            for _ in range(n - 1):
                g.chained.replay()
                self.exchange()
            g.optimize.replay()
            return
        for _ in range(n):
            g.compute.replay()
            self.exchange()
            g.optimize.replay()
            self.finish()

    def epoch_losses(self):
        return self.e.loss_hist[: self.e.num_batches].double().cpu().numpy()


class AllReduce(Single):
    """One all-reduce of the flat gradient, replicated optimizer ("auto" holds it until resolved)."""
    single = False
    chained = True

    def exchange(self):
        D.allreduce_flat_grads(self.e.grads, self.e.group)

    @property
    def captured(self):
        """Off by default: the collective between graphs needs only a plain all_reduce (any backend)."""
        return os.environ.get("NCF_CAPTURE_ALLREDUCE", "0") == "1"


class Zero1(AllReduce):
    """This rank's shard is [rank * shard, ...) of the flat buffers (padded to world x shard floats)."""
    chained = False
    exchange_name = "reduce_scatter"

    def __init__(self, e):
        """This rank's shard, its active ranges, the loss slot's owner and the optimizer's pointers."""
        super().__init__(e)
        S = self.shard = D.shard_floats(int(e.lay.total), e.world_size)
        r = e.rank
        assert e.flat.numel() >= S * e.world_size
        rng = [[e._ranges[2 * k], e._ranges[2 * k + 1]] for k in range(e._nranges)]
        self.gshard = torch.zeros(S, dtype=torch.float32, device=e.device)
        # an empty [0, 0) range when no active parameter falls in the shard: the
        # launch still records the loss if this rank owns the loss slot
        srng = D.shard_ranges(rng, e.world_size, r, S) or [[0, 0]]
        self._sranges = (ctypes.c_int64 * (2 * len(srng)))(*[x for q in srng for x in q])
        self._nsranges = len(srng)
        slot = int(e.lay.loss_slot)
        self.loss_owner = slot // S
        self.loss_slot = slot - r * S
        self.opt_ptrs = (e.flat.data_ptr() + 4 * r * S, self.gshard.data_ptr())
        self._ag_scratch = None

    def tune(self):
        """On the factored fused path (dm <= 64, Adam): the step forms only the dW0 partials
        (NCF_LAYOUT_FACT_DEFER_DX) and each rank expands the summed G rows of its own shard inside its
        Adam launch (ncf_adam_step_fact) -- the expansion and the optimizer sharded together, 1/W of each
        per rank.  NCF_FACT_SHARD=0 keeps the full expansion before the reduce-scatter (A/B)."""
        lay, m = self.e.lay, self.e.model
        self.fact_shard = bool(
            self.e.optimizer == "adam" and self.e.distill is None
            and os.environ.get("NCF_FACT_SHARD", "1") == "1"
            and not (lay.flags & L.LAYOUT_LAYERED) and lay.dropout == 0.0
            and L.supported(m.model_type, m.factor_num, m.num_layers) == L.PATH_FUSED
            and (m.factor_num << (m.num_layers - 1)) <= 64
            and L.hip().ncf_fact_mode(ctypes.byref(lay)) == 1)
        if self.fact_shard:
            lay.flags |= L.LAYOUT_FACT_DEFER_DX
        else:
            lay.flags &= ~L.LAYOUT_FACT_DEFER_DX

    def exchange(self):
        D.reduce_scatter_flat(self.gshard, self.e.grads, self.e.rank, self.e.group)

    def optimize(self):
        """The full local gradient buffer is zeroed too; only the loss slot's owner records the loss."""
        e, st = self.e, L.stream_ptr(self.e.device)
        hist = e.loss_hist.data_ptr() if e.rank == self.loss_owner else None
        p, g = self.opt_ptrs
        if not self.fact_shard:
            # the shard gradient is in gshard: clear the local bucket (the factored launch does it itself)
            L.check(L.hip().ncf_zero_f32(e.grads.data_ptr(), e.grads.numel(), st), "ncf_zero_f32")
            self._dense(p, g, self._sranges, self._nsranges, hist)
            return
        # the shard's G rows expanded inside the optimizer launch (+ the bucket cleared)
        L.check(L.hip().ncf_adam_step_fact(ctypes.byref(e.lay), e.ws.data_ptr(), p, g, e.exp_avg.data_ptr(),
                                           e.exp_avg_sq.data_ptr(), self._sranges, self._nsranges,
                                           e.rank * self.shard, e.grads.data_ptr(), e.grads.numel(),
                                           e.ctl.data_ptr(), *e._adam_args, self.loss_slot, hist, e.num_batches,
                                           st), "ncf_adam_step_fact")

    def finish(self):
        e = self.e
        if self._ag_scratch is None and not D._native_ok(e.flat, e.group):
            self._ag_scratch = torch.empty_like(e.flat)
        D.all_gather_flat(e.flat, e.rank, self.shard, e.group, self._ag_scratch)

    def timed_parts(self):
        return super().timed_parts() + [("all_gather", self.finish)]

    def epoch_losses(self):
        """The loss slot's owner recorded it and broadcasts it (a collective: every rank calls this)."""
        import torch.distributed as dist
        h = self.e.loss_hist[: self.e.num_batches].clone()
        if not D._native_ok(h, self.e.group):
            h = h.cpu()
        dist.broadcast(h, src=self.loss_owner, group=self.e.group)
        return h.double().cpu().numpy()


class Touched(AllReduce):
    """The rows a global batch touches + the tower: packed, all-reduced, replicated deferred Adam."""
    lazy = True

    def __init__(self, e, floats=None):
        super().__init__(e)
        self._packed = torch.zeros(self._floats(1) if floats is None else floats,  # resized in prepare
                                   dtype=torch.float32, device=e.device)

    def _floats(self, batch):
        e = self.e
        return int(L.hip().ncf_touched_packed_floats(ctypes.byref(e.lay), e._ranges, e._nranges, batch))

    def prepare(self, rows):
        pf = self._floats(self.e.batch_size)
        if self._packed.numel() != pf:
            self._packed = torch.zeros(pf, dtype=torch.float32, device=self.e.device)
            self.e._drop_graphs()

    def compute(self):
        e = self.e
        e._train_launch()  # (ctl advances in the optimizer)
        L.check(L.hip().ncf_touched_pack(ctypes.byref(e.lay), e.ws.data_ptr(), e.grads.data_ptr(), e._ranges,
                                         e._nranges, e._touched_buf(e.rows).data_ptr(), e.n_total, e.batch_size,
                                         e.ctl.data_ptr(), self._packed.data_ptr(), L.stream_ptr(e.device)),
                "ncf_touched_pack")

    def exchange(self):
        D.allreduce_flat_grads(self._packed, self.e.group)

    def optimize(self):
        e = self.e
        L.check(L.hip().ncf_lazy_adam_step_packed(ctypes.byref(e.lay), e.flat.data_ptr(), e.exp_avg.data_ptr(),
                                                  e.exp_avg_sq.data_ptr(), e._ranges, e._nranges, e.ctl.data_ptr(),
                                                  *e._adam_args, *e._hist_args, *e._lazy_args,
                                                  self._packed.data_ptr(), L.stream_ptr(e.device)),
                "ncf_lazy_adam_step_packed")

    def timed_parts(self):
        return [("ncf_train_step+ncf_touched_pack", self.compute), ("allreduce", self.exchange),
                ("ncf_lazy_adam_step_packed", self.optimize)]


class Owner(AllReduce):
    """Embedding row id is owned by rank id % W (ncf_owner_* in include/ncf_hip.h).  No host
    synchronisation: each step's bucket lists are built once per epoch from the stream all hold."""
    chained = False

    def __init__(self, e):
        super().__init__(e)
        self.slots = (0, 0)   # list slots high-water (max_u, max_i)
        self.lists = {}       # bucket lists per stream buffer
        self.bufs = None      # the four exchange buffers: send, recv, send2, recv2
        self.dmax = None      # the longest lists of the last build (device)
        self.pre = {}         # prebuild results per stream buffer
        self.old = []         # replaced list buffers (a side-stream prebuild may still write them)
        self.capture_error = False

    def _build(self, rows, mu, mi, dmax, stream, n=None):
        """A plan with list slots (mu, mi) and the bucket lists of `rows` under it (maxima to dmax)."""
        e, P = self.e, L.NcfOwnerPlan()
        L.check(L.hip().ncf_owner_plan_init(ctypes.byref(e.lay), e._ranges, e._nranges,
                                            e.n_total if n is None else int(n), e.batch_size, e.world_size,
                                            e.rank, int(mu), int(mi), ctypes.byref(P)), "ncf_owner_plan_init")
        L.check(L.hip().ncf_owner_lists(ctypes.byref(P), ctypes.byref(e.lay), rows.data_ptr(),
                                        self._lists_buf(rows, P).data_ptr(), dmax.data_ptr(), stream),
                "ncf_owner_lists")
        return P

    def prebuild(self, rows, stream):
        """The epoch's bucket lists built on the pipeline's side stream right after the stream
        itself, with the current list slots, and their maxima copied to pinned memory: at the
        epoch boundary prepare only reads two numbers of a build that finished long before (the
        host does not wait for the running epoch); lists longer than the slots are rebuilt there."""
        e = self.e
        if e.batch_size is None or self.plan is None:
            return
        mu, mi = self.slots
        dmax = torch.zeros(2, dtype=torch.int32, device=e.device)
        self._build(rows, mu, mi, dmax, stream.cuda_stream, n=rows.numel())
        host = torch.empty(2, dtype=torch.int32, pin_memory=True)
        host.copy_(dmax, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
        self.pre[(rows.data_ptr(), rows.numel(), e.batch_size)] = ((mu, mi), host, ev, dmax)

    def _lists_buf(self, rows=None, plan=None):
        """The bucket lists of stream buffer `rows` (default: the current one) under `plan`."""
        rows, plan = self.e.rows if rows is None else rows, self.plan if plan is None else plan
        ints = (int(plan.lists_bytes) + 3) // 4
        return self.e._side_buf(self.lists, rows, True, lambda: ints, torch.int32, torch.zeros, self._replaced)

    def _replaced(self, buf):  # work already queued may still use a list buffer that grew: kept until done
        ev = torch.cuda.Event()
        ev.record()  # the current stream (the side stream inside a prebuild)
        self.old.append((buf, [ev], False))

    alloc_for = _lists_buf

    def prepare(self, rows):
        """The epoch's bucket lists (ncf_owner_lists) for stream buffer `rows`; the list slots grow (the
        exchange buffers with them, graphs re-captured) when a list of this stream is longer than the
        slots -- the same decision on every rank.  One host read of the two maxima per epoch."""
        e = self.e
        self._retire()
        if self.dmax is None:
            self.dmax = torch.zeros(2, dtype=torch.int32, device=e.device)
        mu, mi = self.slots
        pre = self.pre.pop((rows.data_ptr(), rows.numel(), e.batch_size), None)
        if (pre is not None and pre[0] == (mu, mi) and self.plan is not None
                and int(self.plan.n_total) == rows.numel() and int(self.plan.batch_global) == e.batch_size):
            _, host, ev, _ = pre
            ev.synchronize()  # the side-stream build (a prefetched epoch: finished long before)
            need_u, need_i = (int(x) for x in host.tolist())
            if need_u <= mu and need_i <= mi:
                torch.cuda.current_stream(e.device).wait_event(ev)
                return
        while True:
            plan = self._build(rows, mu, mi, self.dmax, L.stream_ptr(e.device))
            need_u, need_i = (int(x) for x in self.dmax.cpu().tolist())
            if need_u <= mu and need_i <= mi:
                break
            # slots grow to OWNER_SLACK x the longest list seen (+16, multiples of 16)
            grow = lambda need, cur: max(cur, (int(need * e.OWNER_SLACK) + 16 + 15) // 16 * 16)  # noqa: E731
            mu, mi = grow(need_u, mu), grow(need_i, mi)
        old = self.plan
        self.plan, self.slots = plan, (mu, mi)
        same = old is not None and all(getattr(old, k) == getattr(plan, k) for k in ("max_u", "max_i", "n_total",
                                                                                      "batch_global", "send_floats"))
        if not same:
            mk = lambda n: torch.zeros(e.world_size * int(n), dtype=torch.float32, device=e.device)  # noqa: E731
            self.bufs = (mk(plan.send_floats), mk(plan.send_floats), mk(plan.param_floats), mk(plan.param_floats))
            e._drop_graphs()

    def _retire(self):
        """Free replaced list buffers once the work queued before their replacement is done: an event from
        the stream that replaced them, one from this (the step) stream at the next epoch boundary."""
        keep = []
        for buf, evs, main in self.old:
            if not main:
                ev = torch.cuda.Event()
                ev.record()
                evs = evs + [ev]
            if not all(x.query() for x in evs):
                keep.append((buf, evs, True))
        self.old = keep

    def compute(self):
        e = self.e
        e._train_launch()
        L.check(L.hip().ncf_owner_pack(ctypes.byref(self.plan), ctypes.byref(e.lay), e.ws.data_ptr(),
                                       e.grads.data_ptr(), self._lists_buf().data_ptr(), e.ctl.data_ptr(),
                                       self.bufs[0].data_ptr(), L.stream_ptr(e.device)), "ncf_owner_pack")

    def _a2a(self, k):
        """k = 0: gradient buckets to their owners; 1: updated rows to their readers."""
        out, inp = (self.bufs[1], self.bufs[0]) if k == 0 else (self.bufs[3], self.bufs[2])
        if self.e.world_size == 1 and self.e.group is None:
            out.copy_(inp)
            return
        D.all_to_all_equal(out, inp, self.e.group)

    def exchange(self):
        self._a2a(0)

    def optimize(self):
        e = self.e
        _, recv, send2, _ = self.bufs
        L.check(L.hip().ncf_owner_adam(ctypes.byref(self.plan), ctypes.byref(e.lay), e.flat.data_ptr(),
                                       e.exp_avg.data_ptr(), e.exp_avg_sq.data_ptr(), e._ranges, e._nranges,
                                       self._lists_buf().data_ptr(), e.ctl.data_ptr(), *e._adam_args, *e._hist_args,
                                       recv.data_ptr(), send2.data_ptr(), L.stream_ptr(e.device)), "ncf_owner_adam")

    def _unpack(self):
        e = self.e
        L.check(L.hip().ncf_owner_unpack(ctypes.byref(self.plan), ctypes.byref(e.lay), e.flat.data_ptr(),
                                         self._lists_buf().data_ptr(), e.ctl.data_ptr(), self.bufs[3].data_ptr(),
                                         L.stream_ptr(e.device)), "ncf_owner_unpack")

    def finish(self):
        self._a2a(1)
        self._unpack()

    def timed_parts(self):
        return [("ncf_train_step+ncf_owner_pack", self.compute), ("all_to_all_grads", self.exchange),
                ("ncf_owner_adam", self.optimize), ("all_to_all_params", lambda: self._a2a(1)),
                ("ncf_owner_unpack", self._unpack)]

    @property
    def captured(self):
        """RCCL: both all-to-alls inside the step graph unless turned off."""
        if self.capture_error:
            return False
        default = "1" if D.capturable(self.e.grads, self.e.group) else "0"
        return os.environ.get("NCF_CAPTURE_ALLREDUCE", default) == "1"

    def capture_failed(self, err):
        """Capturing the all-to-alls raised: eager collectives from then on instead of failing the run."""
        import warnings
        warnings.warn(f"owner exchange: capturing the all-to-alls failed ({err}); eager collectives")
        self.capture_error = True
        return True

    def capture_split(self):
        def unpack_compute():
            self._unpack()
            self.compute()
        g = self.e._graph_of
        return StepGraphs(compute=g(self.compute), optimize=g(self.optimize), chained=g(unpack_compute),
                          tail=g(self._unpack))

    def replay(self, g, n):
        """compute(t0), per step a2a, optimize, a2a, [unpack(t) + compute(t + 1)], the last unpack."""
        if n <= 0:
            return
        g.compute.replay()
        for s in range(n):
            self._a2a(0)
            g.optimize.replay()
            self._a2a(1)
            (g.chained if s + 1 < n else g.tail).replay()

    def sync(self):
        """Every owner's rows to every rank (a replica is current only on the rows it reads).  A collective."""
        e, m, P = self.e, self.e.model, self.plan
        if P is None or e.world_size == 1:
            return
        import torch.distributed as dist
        if e.group is None or dist.get_world_size(e.group) != e.world_size:
            return  # an emulated world on a smaller group (scripts/dp_modes.py): timing only
        f, dm = m.factor_num, m.factor_num << (m.num_layers - 1)
        tables = [(int(P.off[k]), w, n) for k, (w, n) in enumerate(((f, m.user_num), (f, m.item_num),
                                                                     (dm, m.user_num), (dm, m.item_num)))
                  if int(P.off[k]) >= 0]
        D.owner_gather_rows(e.flat, tables, e.world_size, e.rank, e.group)


MODES = {"single": Single, "allreduce": AllReduce, "auto": AllReduce, "zero1": Zero1, "touched": Touched,
         "owner": Owner}
