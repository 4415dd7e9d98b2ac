// Slab reduction and the dense optimizers: ncf_reduce_slab, Adam and SGD over the active
// ranges, the fused reduce + Adam launch, the step-scalar cache, ncf_zero_f32 -- and their
// C ABI (include/ncf_hip.h).  gfx950 only.
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <unordered_map>

#include "ncf_host.h"

namespace ncf {

// ---------------------------------------------------------------------------
// Slab reduction: grads[tb + j] = sum_w slab[w][j], fixed order (bitwise
// reproducible).  Block = 256 threads = 16 float4 columns x 16 row groups, each
// thread 16 independent 16-byte loads; the 16 row-group partials are combined
// in LDS in a fixed order.  Thread 0 of block 0 also advances the step control
// block (batch, adam_t): the fused step before it has read `batch`, the
// optimizer after it reads the advanced `adam_t` (kernel boundaries order it).
__global__ __launch_bounds__(256) void reduce_slab_kernel(const float* __restrict__ slab, float* __restrict__ out,
                                                          int lo, int stride, int rows, ncf_step_ctl* ctl, W0Part wp) {
    __shared__ f4 part[16][16];
    const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int j = lo + (blockIdx.x * 16 + c4) * 4;
    const f4 t = slab_column_total(slab, j, stride, rows, wp, rg, c4, part);
    if (rg == 0 && j < stride) *reinterpret_cast<f4*>(out + j) = t;
    if (ctl != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->batch = ctl->batch + 1;
        ctl->adam_t = ctl->adam_t + 1;
    }
}

void launch_reduce_slab(const ncf_layout* lay, const void* workspace, float* out, ncf_step_ctl* ctl, hipStream_t st) {
    const int stride = (int)ncf_slab_stride(lay);
    const int lo = slab_lo(lay);
    hipLaunchKernelGGL(reduce_slab_kernel, dim3((stride - lo + 63) / 64), dim3(256), 0, st,
                       static_cast<const float*>(workspace), out, lo, stride, reduce_rows(lay), ctl,
                       w0_part(lay, workspace));
}

__device__ ScCache g_sc_cache[SC_SLOTS][2];

// The step-scalar cache entry pair of a control block (see ScCache): one slot per
// (device, ctl pointer) seen, for the life of the process; null (always recompute)
// past SC_SLOTS control blocks on a device.  g_sc_cache has one copy per device, so
// its address is looked up per device -- the device of the launch's stream -- with
// that device current for the lookup.
ScCache* sc_cache_for(const void* ctl, void* stream) {
    struct DevSlots {
        ScCache* base = nullptr;
        bool failed = false;
        std::unordered_map<const void*, int> slots;
    };
    static std::mutex mu;
    static std::unordered_map<int, DevSlots> devs;
    int dev = -1;
    if (hipStreamGetDevice((hipStream_t)stream, &dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    DevSlots& d = devs[dev];
    if (d.failed) return nullptr;
    if (d.base == nullptr) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) return nullptr;
        if (cur != dev && hipSetDevice(dev) != hipSuccess) {
            d.failed = true;
            return nullptr;
        }
        const hipError_t e = hipGetSymbolAddress((void**)&d.base, HIP_SYMBOL(g_sc_cache));
        if (cur != dev) (void)hipSetDevice(cur);
        if (e != hipSuccess) {
            d.base = nullptr;
            d.failed = true;
            return nullptr;
        }
    }
    auto it = d.slots.find(ctl);
    if (it != d.slots.end()) return d.base + 2 * it->second;
    if ((int)d.slots.size() >= SC_SLOTS) return nullptr;
    const int k = (int)d.slots.size();
    d.slots.emplace(ctl, k);
    return d.base + 2 * k;
}

// ---------------------------------------------------------------------------
// Dense Adam (torch.optim.Adam, single-tensor path) + fused grad zeroing.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, Ranges R, const ncf_step_ctl* ctl, double lr,
                                                   double beta1, double beta2, float eps, int64_t loss_slot,
                                                   float* loss_hist, int64_t hist_len, ScCache* scc) {
#pragma clang fp contract(off)
    __shared__ float sc[2];
    const int64_t t_step = ctl->adam_t;  // advanced by ncf_reduce_slab
    step_scalars(scc, t_step, lr, beta1, beta2, sc);
    step_scalars_ahead(scc, t_step, lr, beta1, beta2);
    __syncthreads();
    const float neg_step = sc[0], bc2s = sc[1];
    const float w1 = (float)(1.0 - beta1);
    const float b2 = (float)beta2;
    const float omb2 = (float)(1.0 - beta2);
    const int64_t total = R.prefix[R.n];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q0 < total; q0 += 2 * stride) {
        const int64_t q1 = q0 + stride;
        const bool has1 = q1 < total;
        int which;
        const int64_t i0 = range_locate(R, q0, &which);
        const int64_t i1 = has1 ? range_locate(R, q1, &which) : i0;
        f4 g0 = *reinterpret_cast<const f4*>(g + i0), g1 = *reinterpret_cast<const f4*>(g + i1);
        f4 m0 = *reinterpret_cast<const f4*>(m + i0), m1 = *reinterpret_cast<const f4*>(m + i1);
        f4 v0 = *reinterpret_cast<const f4*>(v + i0), v1 = *reinterpret_cast<const f4*>(v + i1);
        f4 p0 = *reinterpret_cast<const f4*>(p + i0), p1 = *reinterpret_cast<const f4*>(p + i1);
        adam_f4(p0, m0, v0, g0, w1, b2, omb2, bc2s, eps, neg_step);
        *reinterpret_cast<f4*>(m + i0) = m0;
        *reinterpret_cast<f4*>(v + i0) = v0;
        *reinterpret_cast<f4*>(p + i0) = p0;
        *reinterpret_cast<f4*>(g + i0) = f4{0.f, 0.f, 0.f, 0.f};
        if (has1) {
            adam_f4(p1, m1, v1, g1, w1, b2, omb2, bc2s, eps, neg_step);
            *reinterpret_cast<f4*>(m + i1) = m1;
            *reinterpret_cast<f4*>(v + i1) = v1;
            *reinterpret_cast<f4*>(p + i1) = p1;
            *reinterpret_cast<f4*>(g + i1) = f4{0.f, 0.f, 0.f, 0.f};
        }
    }
    record_loss(ctl, g, loss_slot, loss_hist, hist_len);
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, float* __restrict__ g, Ranges R,
                                                  const ncf_step_ctl* ctl, float lr, int64_t loss_slot, float* loss_hist,
                                                  int64_t hist_len) {
#pragma clang fp contract(off)
    const int64_t total = R.prefix[R.n];
    const float nlr = -lr;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        int which;
        const int64_t i = range_locate(R, q, &which);
        f4 gg = *reinterpret_cast<const f4*>(g + i);
        f4 pp = *reinterpret_cast<const f4*>(p + i);
        pp.x = pp.x + nlr * gg.x;  // param.add_(grad, alpha=-lr)
        pp.y = pp.y + nlr * gg.y;
        pp.z = pp.z + nlr * gg.z;
        pp.w = pp.w + nlr * gg.w;
        *reinterpret_cast<f4*>(p + i) = pp;
        *reinterpret_cast<f4*>(g + i) = f4{0.f, 0.f, 0.f, 0.f};
    }
    record_loss(ctl, g, loss_slot, loss_hist, hist_len);
}

// Tower block for slabs of at most 16 rows and no dW0 partials (the layered path: 1-16
// rows; the fused small-batch steps: one row per workgroup): one float4 column per
// thread, its rows summed in order (the same additions as the 16-row-group form: rows 0,
// 1, ..., then the empty groups' zeros, folded into one + 0), then Adam -- every thread
// updates, where the 16 x 16 form reduced through LDS with one thread in 16 updating
// (a stress tower of 700K floats ran 11K such blocks).
__device__ __forceinline__ void tower_col_adam(const float* __restrict__ slab, int lo, int stride, int rows,
                                               int64_t tb, int64_t tower_len, float* __restrict__ p,
                                               float* __restrict__ m, float* __restrict__ v, const Ranges& R,
                                               int64_t t_step, int64_t b_step, double lr, double beta1,
                                               double beta2, float eps, float* loss_hist, int64_t hist_len, float* sc,
                                               const ScCache* scc) {
#pragma clang fp contract(off)
    const ScCache sce = sc_peek(scc, t_step);
    const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
    const int j = lo + ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    const int64_t i = tb + j;
    const bool upd = j < tower_len && in_ranges(R, i);
    f4 pp, mm, vv;
    if (upd) {
        pp = *reinterpret_cast<const f4*>(p + i);
        mm = *reinterpret_cast<const f4*>(m + i);
        vv = *reinterpret_cast<const f4*>(v + i);
    }
    f4 x[16];
#pragma unroll
    for (int r = 0; r < 16; ++r)
        x[r] = (r < rows && j < stride) ? *reinterpret_cast<const f4*>(slab + (int64_t)r * stride + j)
                                        : f4{0.f, 0.f, 0.f, 0.f};
    f4 gs = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (r < rows) { gs.x += x[r].x; gs.y += x[r].y; gs.z += x[r].z; gs.w += x[r].w; }
    if (rows < 16) { gs.x += 0.f; gs.y += 0.f; gs.z += 0.f; gs.w += 0.f; }
    sc_resolve(sce, t_step, lr, beta1, beta2, sc);
    __syncthreads();
    if (j == tower_len) {
        if (loss_hist != nullptr && hist_len > 0) loss_hist[((b_step % hist_len) + hist_len) % hist_len] = gs.x;
    } else if (upd) {
        adam_f4(pp, mm, vv, gs, w1, b2, omb2, sc[1], eps, sc[0]);
        *reinterpret_cast<f4*>(m + i) = mm;
        *reinterpret_cast<f4*>(v + i) = vv;
        *reinterpret_cast<f4*>(p + i) = pp;
    }
}

// ---------------------------------------------------------------------------
// ncf_reduce_adam_step: blocks [0, nA) each reduce 64 slab columns (the order of
// reduce_slab_kernel) and apply Adam to the active ones in place; blocks
// [nA, grid) run the plain Adam over the embedding ranges RE.  t and the batch
// come from the snapshot the train step wrote; block 0 commits them.
// (tower_reduce_adam_block, shared with lazy_adam_kernel: ncf_adam.h)
__global__ __launch_bounds__(256) void reduce_adam_kernel(const float* __restrict__ slab, int lo, int stride, int rows,
                                                          int nA, int64_t tb, int64_t tower_len, float* __restrict__ p,
                                                          float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, Ranges R, Ranges RE,
                                                          ncf_step_ctl* ctl, double lr, double beta1, double beta2,
                                                          float eps, float* loss_hist, int64_t hist_len, W0Part wp,
                                                          ScCache* scc, int colmode) {
#pragma clang fp contract(off)
    __shared__ float sc[2];
    __shared__ f4 part[16][16];
    const int64_t t_step = ctl->snap_t;
    const int64_t b_step = ctl->snap_batch;
    step_scalars_ahead(scc, t_step, lr, beta1, beta2);
    if ((int)blockIdx.x < nA && colmode) {
        tower_col_adam(slab, lo, stride, rows, tb, tower_len, p, m, v, R, t_step, b_step, lr, beta1, beta2, eps,
                       loss_hist, hist_len, sc, scc);
    } else if ((int)blockIdx.x < nA) {
        tower_reduce_adam_block(slab, lo, stride, rows, tb, tower_len, p, m, v, R, t_step, b_step, lr, beta1, beta2,
                                eps, loss_hist, hist_len, wp, sc, part, scc);
    } else {
        const float w1 = (float)(1.0 - beta1);
        const float b2 = (float)beta2;
        const float omb2 = (float)(1.0 - beta2);
        const int64_t total = RE.prefix[RE.n];
        const int64_t nthr = (int64_t)(gridDim.x - nA) * blockDim.x;
        int64_t q = (int64_t)(blockIdx.x - nA) * blockDim.x + threadIdx.x;
        int64_t i = 0;
        f4 gg, mm, vv, pp;
        auto load = [&]() {
            int which;
            i = range_locate(RE, q, &which);
            gg = *reinterpret_cast<const f4*>(g + i);
            mm = *reinterpret_cast<const f4*>(m + i);
            vv = *reinterpret_cast<const f4*>(v + i);
            pp = *reinterpret_cast<const f4*>(p + i);
        };
        const ScCache sce = sc_peek(scc, t_step);
        if (q < total) load();  // the first element's loads fly while thread 0 resolves the scalars
        sc_resolve(sce, t_step, lr, beta1, beta2, sc);
        __syncthreads();
        const float neg_step = sc[0], bc2s = sc[1];
        while (q < total) {
            adam_f4(pp, mm, vv, gg, w1, b2, omb2, bc2s, eps, neg_step);
            *reinterpret_cast<f4*>(m + i) = mm;
            *reinterpret_cast<f4*>(v + i) = vv;
            *reinterpret_cast<f4*>(p + i) = pp;
            *reinterpret_cast<f4*>(g + i) = f4{0.f, 0.f, 0.f, 0.f};
            q += nthr;
            if (q < total) load();
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // no other block of this launch reads these two
        ctl->adam_t = t_step;
        ctl->batch = b_step + 1;
    }
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zero_f32_kernel(f4* __restrict__ p, int64_t n4) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (int64_t)gridDim.x * blockDim.x)
        p[q] = f4{0.f, 0.f, 0.f, 0.f};
}

int launch_zero_f32(float* p, int64_t n, hipStream_t st) {
    if (!p || n < 0 || (n & 3) || (reinterpret_cast<uintptr_t>(p) & 15)) return NCF_E_ARG;
    if (n == 0) return NCF_OK;
    int64_t grid = (n / 4 + 255) / 256;
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(zero_f32_kernel, dim3((int)grid), dim3(256), 0, st, reinterpret_cast<f4*>(p), n / 4);
    return hipGetLastError() == hipSuccess ? NCF_OK : NCF_E_LAUNCH;
}

}  // namespace ncf

using namespace ncf;

extern "C" {

int ncf_reduce_slab(const ncf_layout* lay, const void* workspace, float* grads, ncf_step_ctl* ctl, void* stream) {
    if (!lay || !workspace || !grads) return NCF_E_ARG;
    launch_reduce_slab(lay, workspace, grads + lay->tower_begin, ctl, (hipStream_t)stream);
    return launch_status();
}

int ncf_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int64_t* ranges,
                  int nranges, ncf_step_ctl* ctl, double lr, double beta1, double beta2, double eps,
                  int64_t loss_slot, float* loss_hist, int64_t hist_len, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !ranges || !ctl) return NCF_E_ARG;
    int err = 0;
    Ranges R = make_ranges(ranges, nranges, &err);
    if (err) return NCF_E_ARG;
    const int64_t total = R.prefix[R.n];
    int64_t grid = (total + 511) / 512;  // two float4 per thread
    if (grid > 4096) grid = 4096;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(adam_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg,
                       exp_avg_sq, R, ctl, lr, beta1, beta2, (float)eps, loss_slot, loss_hist, hist_len,
                       sc_cache_for(ctl, stream));
    return launch_status();
}

int ncf_reduce_adam_step(const ncf_layout* lay, const void* workspace, float* params, float* grads, float* exp_avg,
                         float* exp_avg_sq, const int64_t* ranges, int nranges, ncf_step_ctl* ctl, double lr,
                         double beta1, double beta2, double eps, float* loss_hist, int64_t hist_len, void* stream) {
    if (!lay || !workspace || !params || !grads || !exp_avg || !exp_avg_sq || !ranges || !ctl) return NCF_E_ARG;
    if (lay->flags & NCF_LAYOUT_RETIRED_0X20) return NCF_E_UNSUPPORTED;
    int err = 0;
    Ranges R = make_ranges(ranges, nranges, &err);
    if (err) return NCF_E_ARG;
    // plain-Adam part of the active ranges: [begin, min(end, tower_begin)), the
    // embedding tables (their gradient is in grads)
    const int64_t plain_end = lay->tower_begin;
    int64_t er[16];
    int ne = 0;
    for (int i = 0; i < nranges; ++i) {
        const int64_t b = ranges[2 * i];
        const int64_t e = ranges[2 * i + 1] < plain_end ? ranges[2 * i + 1] : plain_end;
        if (e > b) {
            er[2 * ne] = b;
            er[2 * ne + 1] = e;
            ++ne;
        }
    }
    Ranges RE;
    memset(&RE, 0, sizeof(RE));
    if (ne > 0) {
        RE = make_ranges(er, ne, &err);
        if (err) return NCF_E_ARG;
    }
    const int stride = (int)ncf_slab_stride(lay);
    const int lo = slab_lo(lay);
    const int rows = reduce_rows(lay);
    const W0Part wp = w0_part(lay, workspace);
    // tower blocks: one float4 column per thread on the layered path (slab of <= 16 rows,
    // no dW0 partials): stress 857 -> 841 us/step; CLI unchanged; on the fused
    // small-batch step (C2: 16 rows, a 6K-float tower, 6 such blocks) the 16 x 16 form
    // stays, 18.6 against 19.7 us (profiles/r06_evidence/tower_col_ab/).  NCF_TOWER_COL=0:
    // the 16 x 16 form everywhere (A/B)
    static const bool col_ok = [] {
        const char* e = getenv("NCF_TOWER_COL");
        return !(e != nullptr && e[0] == '0');
    }();
    const int colmode = col_ok && rows <= 16 && wp.p == nullptr && train_fused(lay) == nullptr ? 1 : 0;
    const int nA = colmode ? ((stride - lo) / 4 + 1 + 255) / 256 : (stride - lo + 63) / 64;
    const int64_t etotal = RE.prefix[RE.n];
    int64_t nB = (etotal + 255) / 256;
    // embedding-Adam blocks at most: one float4 per thread up to 2M float4 (C4's 3.3M
    // float4: 8192 against 2048 blocks took the step 132.4 -> 129.8 us; 16384 / 65536 the
    // same as 8192; profiles/r06_evidence/adam_blocks_ab/).  NCF_ADAM_MAXB: A/B
    static const int64_t max_b = [] {
        const char* e = getenv("NCF_ADAM_MAXB");
        const long v = e ? atol(e) : 0;
        return (int64_t)(v > 0 ? v : 8192);
    }();
    if (nB > max_b) nB = max_b;
    hipLaunchKernelGGL(reduce_adam_kernel, dim3((unsigned)(nA + nB)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const float*>(workspace), lo, stride, rows, nA, lay->tower_begin, lay->tower_len,
                       params, grads, exp_avg, exp_avg_sq, R, RE, ctl, lr, beta1, beta2, (float)eps, loss_hist,
                       hist_len, wp, sc_cache_for(ctl, stream), colmode);
    return launch_status();
}

int ncf_sgd_step(float* params, float* grads, const int64_t* ranges, int nranges, ncf_step_ctl* ctl, double lr,
                 int64_t loss_slot, float* loss_hist, int64_t hist_len, void* stream) {
    if (!params || !grads || !ranges || !ctl) return NCF_E_ARG;
    int err = 0;
    Ranges R = make_ranges(ranges, nranges, &err);
    if (err) return NCF_E_ARG;
    const int64_t total = R.prefix[R.n];
    int64_t grid = (total + 255) / 256;
    if (grid > 2048) grid = 2048;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(sgd_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, params, grads, R, ctl, (float)lr,
                       loss_slot, loss_hist, hist_len);
    return launch_status();
}

int ncf_zero_f32(float* p, int64_t n, void* stream) { return launch_zero_f32(p, n, (hipStream_t)stream); }

}  // extern "C"
