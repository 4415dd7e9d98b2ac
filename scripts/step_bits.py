#!/usr/bin/env python3
"""sha256 of what one layered step computes, per shape -- run it under two library builds
(NCF_HIP_LIB=<variant>) to check that a kernel change that claims to keep the arithmetic
gives bitwise the same outputs.  Per shape: `fwd` hashes the ncf_forward logits, `step`
the logits and the reduced gradient buffer of one ncf_train_step + ncf_reduce_slab, and
`gemm` the same without the buffer's tail from the predict weights on (dwp, dbp, loss).

The inputs make the step run-to-run identical (a state hash over training steps is not:
the gradients pass through float atomics in arrival order): U = I = 512 and B = 256 rows
with all users distinct and all items distinct, so there is one row chunk and one dW0
chunk per table, and every atomic target of the GEMM epilogues receives one addend into
zeroed memory.  dwp, dbp and the loss are sums over the rows through LDS and slab atomics
in arrival order: `step` differs in their last bits between two runs of one library
(measured: at most 6e-8 on values up to 0.8), `gemm` and `fwd` do not.  For `step`,
compare element-wise: --cmp A A2 B prints, per shape, max |A - A2| (one library twice)
and max |B - A|, which may not exceed it.
Each shape runs in its own process (the library reads its environment switches once).
usage: step_bits.py [--save DIR]     (DIR: the hashed arrays as DIR/<shape>.npz)
       step_bits.py --cmp DIR_A DIR_A2 DIR_B"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = I = 512
B = 256
# name, model type, factor_num, layers, dropout, per-row layer 0, environment
SHAPES = [
    ("neumf_64_4", "NeuMF-end", 64, 4, 0.0, False, {}),  # x6b, x6<128>, x6<64>
    ("neumf_64_4_w0pre0", "NeuMF-end", 64, 4, 0.0, False, {"NCF_W0PRE": "0"}),
    ("neumf_64_4_tile64", "NeuMF-end", 64, 4, 0.0, False, {"NCF_GEMM_TILE": "64"}),
    ("neumf_32_3", "NeuMF-end", 32, 3, 0.0, False, {}),  # step chain, lyr_bwd_w_multi_kernel<64>
    ("neumf_32_3_per_row", "NeuMF-end", 32, 3, 0.0, True, {}),  # per-layer Vec4 kernels
    ("neumf_6_3", "NeuMF-end", 6, 3, 0.0, False, {}),  # scalar core
    ("mlp_11_2", "MLP", 11, 2, 0.0, False, {}),
    ("neumf_32_3_drop", "NeuMF-end", 32, 3, 0.1, False, {}),  # ScalarDrop
]


def child(idx, save):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import ncf_amd._lib as L
    from ncf_amd import ops
    from ncf_amd.models import NCF
    name, mt, f, layers, p, per_row, _ = SHAPES[idx]
    dev = "cuda:0"
    torch.manual_seed(11)
    m = NCF(U, I, f, layers, p, mt).to(dev)
    rng = np.random.default_rng(3)
    u = torch.as_tensor(rng.permutation(U)[:B], dtype=torch.int32, device=dev)
    it = torch.as_tensor(rng.permutation(I)[:B], dtype=torch.int32, device=dev)
    y = torch.as_tensor((rng.random(B) < 0.2), dtype=torch.float32, device=dev)
    flat, lay0 = ops.ensure_flat(m)
    rows = ops.pack_rows(u, it, y)
    fwd = ops.forward_logits(flat, lay0, rows).cpu().numpy()
    lay = type(lay0).from_buffer_copy(lay0)
    if per_row:
        lay.flags |= L.LAYOUT_PER_ROW_L0
    ops.set_dropout(lay, m)
    gflat = torch.zeros(int(lay.total), device=dev)
    ws = ops.new_workspace(lay, B, dev)
    ctl = ops.new_ctl(B, dev)
    logits = torch.empty(B, device=dev)
    st = L.stream_ptr()
    L.check(L.hip().ncf_train_step(L.ctypes.byref(lay), flat.data_ptr(), gflat.data_ptr(), rows.data_ptr(), None,
                                   None, ctl.data_ptr(), B, 1, 0, L.DZ_BCE, ws.data_ptr(), ws.numel() * 4,
                                   logits.data_ptr(), st), "train")
    L.check(L.hip().ncf_reduce_slab(L.ctypes.byref(lay), ws.data_ptr(), gflat.data_ptr(), ctl.data_ptr(), st),
            "reduce")
    torch.cuda.synchronize()
    lg, g = logits.cpu().numpy(), gflat.cpu().numpy()
    assert np.isfinite(fwd).all() and np.isfinite(lg).all() and np.isfinite(g).all() and g.any()
    if save:
        os.makedirs(save, exist_ok=True)
        np.savez(os.path.join(save, name + ".npz"), fwd=fwd, logits=lg, grads=g)
    sha = lambda *a: hashlib.sha256(b"".join(x.tobytes() for x in a)).hexdigest()[:16]
    print(f"BITS {name} lib={os.environ.get('NCF_HIP_LIB', '') or 'default'} fwd={sha(fwd)} step={sha(lg, g)} "
          f"gemm={sha(lg, g[:int(lay.wp)])}")


def cmp(da, da2, db):
    import numpy as np
    for name in (s[0] for s in SHAPES):
        a, a2, b = (np.load(os.path.join(d, name + ".npz")) for d in (da, da2, db))
        for k in ("fwd", "logits", "grads"):
            own, new = float(np.abs(a[k] - a2[k]).max()), float(np.abs(b[k] - a[k]).max())
            print(f"CMP {name} {k}: max|A-A2|={own:.3e} max|B-A|={new:.3e} {'ok' if new <= own else 'EXCEEDS'}")


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(int(args[1]), args[2] if len(args) > 2 else "")
    if args and args[0] == "--cmp":
        return cmp(*args[1:4])
    save = args[1] if len(args) > 1 and args[0] == "--save" else ""
    for idx, shape in enumerate(SHAPES):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(idx), save],
                             env=dict(os.environ, **shape[6]), capture_output=True, text=True, timeout=300)
        if out.returncode != 0:  # nothing more runs on the GPU after a failure
            print(out.stdout[-2000:], out.stderr[-3000:])
            sys.exit(out.returncode)
        print("\n".join(l for l in out.stdout.splitlines() if l.startswith("BITS")), flush=True)


if __name__ == "__main__":
    main()
