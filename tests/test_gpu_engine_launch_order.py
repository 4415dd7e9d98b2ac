"""What a TrainEngine step consists of, per exchange mode and optimizer form: every C
entry point, collective, graph capture and graph replay the engine issues, in order,
against the literal tables below.

The recorder hooks only names that exist whatever the engine's inner structure is:
``ncf_amd._lib.hip`` (a forwarding proxy: each C entry point called through it emits
its name), the collectives of ``ncf_amd.distributed`` (``coll:<name>``),
``torch.cuda.graph.__enter__`` / ``__exit__`` (``capture{`` / ``}``; launches issued
from Python while capturing still pass the proxy, so captured bodies are listed) and
``torch.cuda.CUDAGraph.replay`` (``replay#k``, k the graph's index in capture order).

Each case builds an engine, then runs ``set_epoch_stream`` + ``run`` and a second
``set_epoch_stream`` on the same buffer + a shorter ``run`` (graphs already captured:
single-step replays, the end-of-run flush).  ``# ...`` lines mark those calls.
Repeats are folded: ``3x[a b]`` is a b a b a b.

The tables were recorded on an MI355X from the commit before the exchange modes moved
into ncf_amd/exchange.py and are the contract for that restructuring: do not edit them
to follow the code."""
import contextlib
import os
import socket
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

U, I, T = 300, 400, 12
COLLECTIVES = ("allreduce_flat_grads", "reduce_scatter_flat", "all_gather_flat", "all_to_all_equal",
               "owner_gather_rows")
MODES = ("allreduce", "zero1", "touched", "owner")

# in-process cases: engine keywords, environment, the two runs (steps, use_graph)
GRAPH, EAGER = ((12, True), (5, True)), ((3, False), (2, False))
CASES = {
    "adam-graph": dict(runs=GRAPH),
    "adam-eager": dict(runs=EAGER),
    "sgd-graph": dict(runs=GRAPH, optimizer="sgd"),
    "sgd-eager": dict(runs=EAGER, optimizer="sgd"),
    "lazy-graph": dict(runs=GRAPH, env={"NCF_LAZY_ADAM": "1"}),
    "lazy-eager": dict(runs=EAGER, env={"NCF_LAZY_ADAM": "1"}),
    # 4 training workgroups: in-step Adam on by default; 3-step graph chunks
    "ais-graph": dict(runs=((7, True), (5, True)), f=8, B=256, graph_steps=3, ais=True),
}


class _Proxy:
    def __init__(self, lib, emit):
        self._lib, self._emit = lib, emit

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self._emit(name)
            return fn(*args)
        return call


@contextlib.contextmanager
def _recording():
    import ncf_amd._lib as L
    import ncf_amd.distributed as D
    events, graphs = [], []
    saved = [(L, "hip", L.hip)] + [(D, n, getattr(D, n)) for n in COLLECTIVES] + [
        (torch.cuda.graph, "__enter__", torch.cuda.graph.__enter__),
        (torch.cuda.graph, "__exit__", torch.cuda.graph.__exit__),
        (torch.cuda.CUDAGraph, "replay", torch.cuda.CUDAGraph.replay)]
    proxy = _Proxy(L.hip(), events.append)
    L.hip = lambda: proxy

    def coll(name, fn):
        def call(*a, **kw):
            events.append("coll:" + name)
            return fn(*a, **kw)
        return call
    for name in COLLECTIVES:
        setattr(D, name, coll(name, getattr(D, name)))
    enter, exit_, replay = saved[-3][2], saved[-2][2], saved[-1][2]

    def g_enter(self):
        graphs.append(self.cuda_graph)
        events.append("capture{")
        return enter(self)

    def g_exit(self, *exc):
        out = exit_(self, *exc)
        events.append("}")
        return out

    def g_replay(self):
        events.append("replay#%d" % next(k for k, g in enumerate(graphs) if g is self))
        return replay(self)
    torch.cuda.graph.__enter__, torch.cuda.graph.__exit__ = g_enter, g_exit
    torch.cuda.CUDAGraph.replay = g_replay
    try:
        yield events
    finally:
        for obj, name, val in saved:
            setattr(obj, name, val)


def _fold(ev):
    """Run-length form: at each position the repeating block that covers most events
    (the shortest such block), folded recursively."""
    out, i = [], 0
    while i < len(ev):
        p, r = 1, 1
        for q in range(1, min(96, (len(ev) - i) // 2) + 1):
            n = 1
            if "capture{" in ev[i:i + q] or "}" in ev[i:i + q]:
                continue  # a captured body is never folded together with what surrounds it
            while ev[i + q * n:i + q * (n + 1)] == ev[i:i + q]:
                n += 1
            if n > 1 and q * n > p * r:
                p, r = q, n
        if r == 1:
            out.append(ev[i])
        else:
            out.append("%dx[%s]" % (r, " ".join(_fold(ev[i:i + p]))))
        i += p * r
    return out


def _render(events):
    """One line per `# call` marker, the folded events of that call indented under it."""
    lines, cur = [], []
    for e in events + ["#"]:
        if e.startswith("#"):
            depth = 1
            for t in _fold(cur):
                depth -= t == "}"
                lines.append("  " * depth + t)
                depth += t == "capture{"
            cur = []
            if e != "#":
                lines.append(e)
        else:
            cur.append(e)
    return "\n".join(lines)


def _events(runs, f=16, B=1000, optimizer="adam", env=None, graph_steps=None, ais=False, setenv=None, **engine_kw):
    """Rendered event list of one case: NeuMF-end(f, 3) on U x I tables, T batches of B."""
    from ncf_amd import ops
    from ncf_amd.engine import TrainEngine
    from ncf_amd.models import NCF
    for k, v in (env or {}).items():
        setenv(k, v)
    rng = np.random.default_rng(5)
    u, i = rng.integers(0, U, T * B), rng.integers(0, I, T * B)
    y = (rng.random(T * B) < 0.2).astype(np.float32)
    torch.manual_seed(3)
    m = NCF(U, I, f, 3, 0.0, "NeuMF-end").to("cuda:0")
    rows = torch.as_tensor(ops.pack_rows_host(u, i, y), device="cuda:0")
    old = TrainEngine.GRAPH_STEPS
    if graph_steps is not None:
        TrainEngine.GRAPH_STEPS = graph_steps
    try:
        with _recording() as events:
            events.append("# TrainEngine()")
            eng = TrainEngine(m, lr=1e-3, optimizer=optimizer, **engine_kw)
            for n, graph in runs:
                events.append("# set_epoch_stream")
                eng.set_epoch_stream(rows, B)
                events.append("# run(%d%s)" % (n, "" if graph else ", use_graph=False"))
                eng.run(n, use_graph=graph)
            torch.cuda.synchronize()
        assert int(eng.ctl[0].item()) == runs[-1][0]  # the batch counter of the last run
    finally:
        TrainEngine.GRAPH_STEPS = old
    assert ("ncf_train_step_ais" in events) == ais
    return _render(events)


def _child(backend, port, q):
    """A one-rank group with an explicit dp_mode runs the real collectives: gloo with
    the collectives eager between graphs (and wholly eager), nccl (RCCL) with
    NCF_CAPTURE_ALLREDUCE=1, the collectives inside the step graph."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if backend == "nccl":
        os.environ["NCF_CAPTURE_ALLREDUCE"] = "1"
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=0, world_size=1)
    try:
        out = {}
        for mode in MODES:
            for name, runs in (("graph", GRAPH), ("eager", EAGER))[:2 if backend == "gloo" else 1]:
                out["%s-%s-%s" % (backend, mode, name)] = _events(runs, dp_mode=mode, world_size=1, rank=0,
                                                                  process_group=dist.group.WORLD)
        q.put(out)
    except Exception:
        q.put(traceback.format_exc())
    finally:
        dist.destroy_process_group()


def _child_tables(backend):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(backend, port, q))
    p.start()
    try:
        out = q.get(timeout=300)
    except Exception:
        p.kill()
        raise
    p.join(timeout=60)
    if p.exitcode is None:  # e.g. a graph with captured collectives outliving the process group
        p.kill()
        p.join()
        raise AssertionError("the %s child delivered its tables but did not exit" % backend)
    assert p.exitcode == 0
    assert isinstance(out, dict), out
    return out


@pytest.fixture(scope="module")
def gloo_tables():
    return _child_tables("gloo")


@pytest.fixture(scope="module")
def nccl_tables():
    return _child_tables("nccl")


def _same(got, want):
    assert got == want.strip("\n"), "launch order changed; recorded now:\n" + got


@pytest.mark.parametrize("case", sorted(CASES))
def test_single_process_launch_order(case, monkeypatch):
    _same(_events(setenv=monkeypatch.setenv, **CASES[case]), TABLES[case])


@pytest.mark.parametrize("form", ["graph", "eager"])
@pytest.mark.parametrize("mode", MODES)
def test_eager_collective_launch_order(mode, form, gloo_tables):
    case = "gloo-%s-%s" % (mode, form)
    _same(gloo_tables[case], TABLES[case])


@pytest.mark.parametrize("mode", MODES)
def test_captured_collective_launch_order(mode, nccl_tables):
    case = "nccl-%s-graph" % mode
    _same(nccl_tables[case], TABLES[case])


TABLES = {
    "adam-eager": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_uses_user_order
# run(3, use_graph=False)
  2x[ncf_ais_supported]
  2x[ncf_train_step ncf_ais_supported ncf_reduce_adam_step ncf_ais_supported]
  ncf_train_step
  ncf_ais_supported
  ncf_reduce_adam_step
# set_epoch_stream
  ncf_uses_user_order
# run(2, use_graph=False)
  2x[ncf_ais_supported]
  ncf_train_step
  ncf_ais_supported
  ncf_reduce_adam_step
  ncf_ais_supported
  ncf_train_step
  ncf_ais_supported
  ncf_reduce_adam_step
""",
    "adam-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_uses_user_order
# run(12)
  2x[ncf_ais_supported]
  ncf_train_step
  ncf_ais_supported
  ncf_reduce_adam_step
  capture{
    ncf_ais_supported
    ncf_train_step
    ncf_ais_supported
    ncf_reduce_adam_step
  }
  ncf_ais_supported
  capture{
    12x[ncf_ais_supported ncf_train_step ncf_ais_supported ncf_reduce_adam_step]
  }
  11x[replay#0]
# set_epoch_stream
  ncf_uses_user_order
# run(5)
  ncf_ais_supported
  5x[replay#0]
""",
    "ais-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_uses_user_order
# run(7)
  ncf_ais_supported
  ncf_ais_begin
  ncf_ais_supported
  ncf_train_step_ais
  ncf_ais_bump
  ncf_ais_supported
  capture{
    ncf_ais_supported
    ncf_train_step_ais
    ncf_ais_bump
    ncf_ais_supported
  }
  ncf_ais_supported
  capture{
    3x[ncf_train_step_ais]
    ncf_ais_bump
  }
  2x[replay#1]
  ncf_ais_flush
# set_epoch_stream
  ncf_uses_user_order
# run(5)
  ncf_ais_supported
  ncf_ais_begin
  replay#1
  2x[replay#0]
  ncf_ais_flush
""",
    "lazy-eager": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_touched_bytes
  ncf_batch_touched
  ncf_uses_user_order
# run(3, use_graph=False)
  3x[ncf_train_step ncf_lazy_adam_step]
  ncf_lazy_adam_flush
# set_epoch_stream
  ncf_batch_touched
  ncf_uses_user_order
# run(2, use_graph=False)
  2x[ncf_train_step ncf_lazy_adam_step]
  ncf_lazy_adam_flush
""",
    "lazy-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_touched_bytes
  ncf_batch_touched
  ncf_uses_user_order
# run(12)
  ncf_train_step
  ncf_lazy_adam_step
  capture{
    ncf_train_step
    ncf_lazy_adam_step
  }
  capture{
    12x[ncf_train_step ncf_lazy_adam_step]
  }
  11x[replay#0]
  ncf_lazy_adam_flush
# set_epoch_stream
  ncf_batch_touched
  ncf_uses_user_order
# run(5)
  5x[replay#0]
  ncf_lazy_adam_flush
""",
    "sgd-eager": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_uses_user_order
# run(3, use_graph=False)
  3x[ncf_train_step ncf_reduce_slab ncf_sgd_step]
# set_epoch_stream
  ncf_uses_user_order
# run(2, use_graph=False)
  2x[ncf_train_step ncf_reduce_slab ncf_sgd_step]
""",
    "sgd-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_uses_user_order
# run(12)
  ncf_train_step
  ncf_reduce_slab
  ncf_sgd_step
  capture{
    ncf_train_step
    ncf_reduce_slab
    ncf_sgd_step
  }
  capture{
    12x[ncf_train_step ncf_reduce_slab ncf_sgd_step]
  }
  11x[replay#0]
# set_epoch_stream
  ncf_uses_user_order
# run(5)
  5x[replay#0]
""",
    "gloo-allreduce-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_uses_user_order
# run(12)
  ncf_train_step
  ncf_reduce_slab
  coll:allreduce_flat_grads
  ncf_adam_step
  capture{
    ncf_train_step
    ncf_reduce_slab
  }
  capture{
    ncf_adam_step
  }
  capture{
    ncf_adam_step
    ncf_train_step
    ncf_reduce_slab
  }
  replay#0
  10x[coll:allreduce_flat_grads replay#2]
  coll:allreduce_flat_grads
  replay#1
# set_epoch_stream
  ncf_uses_user_order
# run(5)
  replay#0
  4x[coll:allreduce_flat_grads replay#2]
  coll:allreduce_flat_grads
  replay#1
""",
    "gloo-allreduce-eager": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_uses_user_order
# run(3, use_graph=False)
  3x[ncf_train_step ncf_reduce_slab coll:allreduce_flat_grads ncf_adam_step]
# set_epoch_stream
  ncf_uses_user_order
# run(2, use_graph=False)
  2x[ncf_train_step ncf_reduce_slab coll:allreduce_flat_grads ncf_adam_step]
""",
    "gloo-zero1-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_supported
  ncf_fact_mode
  ncf_workspace_bytes
  ncf_uses_user_order
# run(12)
  ncf_train_step
  ncf_reduce_slab
  coll:reduce_scatter_flat
  ncf_adam_step_fact
  coll:all_gather_flat
  capture{
    ncf_train_step
    ncf_reduce_slab
  }
  capture{
    ncf_adam_step_fact
  }
  11x[replay#0 coll:reduce_scatter_flat replay#1 coll:all_gather_flat]
# set_epoch_stream
  ncf_uses_user_order
# run(5)
  5x[replay#0 coll:reduce_scatter_flat replay#1 coll:all_gather_flat]
""",
    "gloo-zero1-eager": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_supported
  ncf_fact_mode
  ncf_workspace_bytes
  ncf_uses_user_order
# run(3, use_graph=False)
  3x[ncf_train_step ncf_reduce_slab coll:reduce_scatter_flat ncf_adam_step_fact coll:all_gather_flat]
# set_epoch_stream
  ncf_uses_user_order
# run(2, use_graph=False)
  2x[ncf_train_step ncf_reduce_slab coll:reduce_scatter_flat ncf_adam_step_fact coll:all_gather_flat]
""",
    "gloo-touched-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
  ncf_touched_packed_floats
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_touched_packed_floats
  ncf_touched_bytes
  ncf_batch_touched
  ncf_uses_user_order
# run(12)
  ncf_train_step
  ncf_touched_pack
  coll:allreduce_flat_grads
  ncf_lazy_adam_step_packed
  capture{
    ncf_train_step
    ncf_touched_pack
  }
  capture{
    ncf_lazy_adam_step_packed
  }
  capture{
    ncf_lazy_adam_step_packed
    ncf_train_step
    ncf_touched_pack
  }
  replay#0
  10x[coll:allreduce_flat_grads replay#2]
  coll:allreduce_flat_grads
  replay#1
  ncf_lazy_adam_flush
# set_epoch_stream
  ncf_touched_packed_floats
  ncf_batch_touched
  ncf_uses_user_order
# run(5)
  replay#0
  4x[coll:allreduce_flat_grads replay#2]
  coll:allreduce_flat_grads
  replay#1
  ncf_lazy_adam_flush
""",
    "gloo-touched-eager": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
  ncf_touched_packed_floats
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_touched_packed_floats
  ncf_touched_bytes
  ncf_batch_touched
  ncf_uses_user_order
# run(3, use_graph=False)
  3x[ncf_train_step ncf_touched_pack coll:allreduce_flat_grads ncf_lazy_adam_step_packed]
  ncf_lazy_adam_flush
# set_epoch_stream
  ncf_touched_packed_floats
  ncf_batch_touched
  ncf_uses_user_order
# run(2, use_graph=False)
  2x[ncf_train_step ncf_touched_pack coll:allreduce_flat_grads ncf_lazy_adam_step_packed]
  ncf_lazy_adam_flush
""",
    "gloo-owner-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  2x[ncf_owner_plan_init ncf_owner_lists]
  ncf_uses_user_order
# run(12)
  ncf_train_step
  ncf_owner_pack
  coll:all_to_all_equal
  ncf_owner_adam
  coll:all_to_all_equal
  ncf_owner_unpack
  capture{
    ncf_train_step
    ncf_owner_pack
  }
  capture{
    ncf_owner_adam
  }
  capture{
    ncf_owner_unpack
    ncf_train_step
    ncf_owner_pack
  }
  capture{
    ncf_owner_unpack
  }
  replay#0
  10x[coll:all_to_all_equal replay#1 coll:all_to_all_equal replay#2]
  coll:all_to_all_equal
  replay#1
  coll:all_to_all_equal
  replay#3
# set_epoch_stream
  ncf_owner_plan_init
  ncf_owner_lists
  ncf_uses_user_order
# run(5)
  replay#0
  4x[coll:all_to_all_equal replay#1 coll:all_to_all_equal replay#2]
  coll:all_to_all_equal
  replay#1
  coll:all_to_all_equal
  replay#3
""",
    "gloo-owner-eager": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  2x[ncf_owner_plan_init ncf_owner_lists]
  ncf_uses_user_order
# run(3, use_graph=False)
  3x[ncf_train_step ncf_owner_pack coll:all_to_all_equal ncf_owner_adam coll:all_to_all_equal ncf_owner_unpack]
# set_epoch_stream
  ncf_owner_plan_init
  ncf_owner_lists
  ncf_uses_user_order
# run(2, use_graph=False)
  2x[ncf_train_step ncf_owner_pack coll:all_to_all_equal ncf_owner_adam coll:all_to_all_equal ncf_owner_unpack]
""",
    "nccl-allreduce-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_uses_user_order
# run(12)
  ncf_train_step
  ncf_reduce_slab
  coll:allreduce_flat_grads
  ncf_adam_step
  capture{
    ncf_train_step
    ncf_reduce_slab
    coll:allreduce_flat_grads
    ncf_adam_step
  }
  capture{
    12x[ncf_train_step ncf_reduce_slab coll:allreduce_flat_grads ncf_adam_step]
  }
  11x[replay#0]
# set_epoch_stream
  ncf_uses_user_order
# run(5)
  5x[replay#0]
""",
    "nccl-zero1-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_supported
  ncf_fact_mode
  ncf_workspace_bytes
  ncf_uses_user_order
# run(12)
  ncf_train_step
  ncf_reduce_slab
  coll:reduce_scatter_flat
  ncf_adam_step_fact
  coll:all_gather_flat
  capture{
    ncf_train_step
    ncf_reduce_slab
    coll:reduce_scatter_flat
    ncf_adam_step_fact
    coll:all_gather_flat
  }
  capture{
    12x[ncf_train_step ncf_reduce_slab coll:reduce_scatter_flat ncf_adam_step_fact coll:all_gather_flat]
  }
  11x[replay#0]
# set_epoch_stream
  ncf_uses_user_order
# run(5)
  5x[replay#0]
""",
    "nccl-touched-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
  ncf_touched_packed_floats
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  ncf_touched_packed_floats
  ncf_touched_bytes
  ncf_batch_touched
  ncf_uses_user_order
# run(12)
  ncf_train_step
  ncf_touched_pack
  coll:allreduce_flat_grads
  ncf_lazy_adam_step_packed
  capture{
    ncf_train_step
    ncf_touched_pack
    coll:allreduce_flat_grads
    ncf_lazy_adam_step_packed
  }
  capture{
    12x[ncf_train_step ncf_touched_pack coll:allreduce_flat_grads ncf_lazy_adam_step_packed]
  }
  11x[replay#0]
  ncf_lazy_adam_flush
# set_epoch_stream
  ncf_touched_packed_floats
  ncf_batch_touched
  ncf_uses_user_order
# run(5)
  5x[replay#0]
  ncf_lazy_adam_flush
""",
    "nccl-owner-graph": """
# TrainEngine()
  2x[ncf_layout_init]
  ncf_supported
# set_epoch_stream
  ncf_layout_tune
  ncf_workspace_bytes
  2x[ncf_owner_plan_init ncf_owner_lists]
  ncf_uses_user_order
# run(12)
  ncf_train_step
  ncf_owner_pack
  coll:all_to_all_equal
  ncf_owner_adam
  coll:all_to_all_equal
  ncf_owner_unpack
  capture{
    ncf_train_step
    ncf_owner_pack
    coll:all_to_all_equal
    ncf_owner_adam
    coll:all_to_all_equal
    ncf_owner_unpack
  }
  capture{
    12x[ncf_train_step ncf_owner_pack coll:all_to_all_equal ncf_owner_adam coll:all_to_all_equal ncf_owner_unpack]
  }
  11x[replay#0]
# set_epoch_stream
  ncf_owner_plan_init
  ncf_owner_lists
  ncf_uses_user_order
# run(5)
  5x[replay#0]
""",
}
