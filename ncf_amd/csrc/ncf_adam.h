// Dense Adam pieces shared by the optimizer launches (ncf_optim.hip, ncf_fact.hip,
// ncf_sparse.hip) and the fused step's in-step optimizer (ncf_train.hip,
// NCF_LAYOUT_ADAM_IN_STEP): the float4 active ranges, torch.optim.Adam's per-element
// update, the step-scalar cache entries, the tower slab's column sums and their Adam block.
#pragma once
#include "ncf_common.h"

namespace ncf {

struct Ranges {
    int64_t begin[8];
    int64_t prefix[9];  // prefix sums of float4 counts
    int n;
};

__device__ __forceinline__ int64_t range_locate(const Ranges& R, int64_t q, int* which) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < 8; ++i)
        if (i < R.n && q >= R.prefix[i]) k = i;
    *which = k;
    return R.begin[k] + (q - R.prefix[k]) * 4;
}

__device__ __forceinline__ bool in_ranges(const Ranges& R, int64_t i) {
    for (int k = 0; k < R.n; ++k)
        if (i >= R.begin[k] && i < R.begin[k] + (R.prefix[k + 1] - R.prefix[k]) * 4) return true;
    return false;
}

__device__ __forceinline__ void adam_f4(f4& p, f4& m, f4& v, const f4& g, float w1, float b2, float omb2,
                                        float bc2s, float eps, float neg_step) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float gr = lane_get(g, r);
        float mr = lane_get(m, r), vr = lane_get(v, r), pr = lane_get(p, r);
        mr = fmaf(w1, gr - mr, mr);          // exp_avg.lerp_(grad, 1 - beta1)   (fmadd form)
        vr = vr * b2 + omb2 * gr * gr;       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        const float den = sqrtf(vr) / bc2s + eps;  // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
        pr = pr + neg_step * mr / den;       // param.addcdiv_(exp_avg, denom, value=-step_size)
        if (r == 0) { m.x = mr; v.x = vr; p.x = pr; }
        else if (r == 1) { m.y = mr; v.y = vr; p.y = pr; }
        else if (r == 2) { m.z = mr; v.z = vr; p.z = pr; }
        else { m.w = mr; v.w = vr; p.w = pr; }
    }
}

// Step-t scalars in double like torch's Python scalars, by thread 0 of the block:
// sc[0] = -(lr / (1 - beta1^t)), sc[1] = sqrt(1 - beta2^t) (torch _single_tensor_adam).
// The two double pows take ~2.5 us on one lane -- longer than the launch's loads --
// so each optimizer launch also computes step t + 1's pair (one lane of block 0,
// beside its other work) into a per-control-block cache entry, and step t + 1's
// launch reads it instead: entry [t & 1] is only written by the launch of step t - 1
// (a finished kernel), never by the launch that reads it.  The entry holds its
// inputs (t, lr, beta1, beta2); any mismatch -- first step, a reloaded or
// teacher-forced state, another optimizer on the same control block -- computes
// the pair again, so the cached value is always the one pow gives.
struct ScCache {
    int64_t t;
    double lr, beta1, beta2;
    float sc0, sc1;
    int64_t pad;
};
constexpr int SC_SLOTS = 1024;

__device__ __forceinline__ void step_pair(int64_t t_step, double lr, double beta1, double beta2, float* a, float* b) {
    const double t = (double)t_step;
    *a = (float)(-(lr / (1.0 - pow(beta1, t))));
    *b = (float)sqrt(1.0 - pow(beta2, t));
}

// thread 0: the cache entry of step t, requested (issue early, resolve late)
__device__ __forceinline__ ScCache sc_peek(const ScCache* cache, int64_t t_step) {
    ScCache e;
    e.t = -1;
    if (threadIdx.x == 0 && cache != nullptr) e = cache[t_step & 1];
    return e;
}

__device__ __forceinline__ void sc_resolve(const ScCache& e, int64_t t_step, double lr, double beta1, double beta2,
                                           float* sc) {
    if (threadIdx.x == 0) {
        if (e.t == t_step && e.lr == lr && e.beta1 == beta1 && e.beta2 == beta2) {
            sc[0] = e.sc0;
            sc[1] = e.sc1;
        } else {
            step_pair(t_step, lr, beta1, beta2, &sc[0], &sc[1]);
        }
    }
}

__device__ __forceinline__ void step_scalars(const ScCache* cache, int64_t t_step, double lr, double beta1,
                                             double beta2, float* sc) {
    sc_resolve(sc_peek(cache, t_step), t_step, lr, beta1, beta2, sc);
}

// step t + 1's entry, by lane 0 of wave 1 of this block (vector stores)
__device__ __forceinline__ void step_scalars_ahead_lane(ScCache* cache, int64_t t_step, double lr, double beta1,
                                                        double beta2) {
    if (cache == nullptr || threadIdx.x != 64) return;
    ScCache e;
    e.t = t_step + 1;
    e.lr = lr;
    e.beta1 = beta1;
    e.beta2 = beta2;
    e.pad = 0;
    step_pair(t_step + 1, lr, beta1, beta2, &e.sc0, &e.sc1);
    cache[(t_step + 1) & 1] = e;
}
// ... by block 0
__device__ __forceinline__ void step_scalars_ahead(ScCache* cache, int64_t t_step, double lr, double beta1,
                                                   double beta2) {
    if (blockIdx.x == 0) step_scalars_ahead_lane(cache, t_step, lr, beta1, beta2);
}

// Scalar form of adam_f4 (the same operations per element, so the same bits).
__device__ __forceinline__ float adam_1(float p, float& m, float& v, float g, float w1, float b2, float omb2, float bc2s,
                                        float eps, float neg_step) {
#pragma clang fp contract(off)
    m = fmaf(w1, g - m, m);
    v = v * b2 + omb2 * g * g;
    const float den = sqrtf(v) / bc2s + eps;
    return p + neg_step * m / den;
}

// One float4 column j of the tower slab's total, summed by one thread in the order of
// slab_column_total (below): row group rg of 16 sums rows rg, rg + 16, ... (and
// the remainder row), then the 16 group sums in order -- the same bits.
__device__ __forceinline__ f4 slab_column_serial(const float* __restrict__ slab, int64_t j, int stride, int rows) {
    const int per = rows / 16;
    f4 t = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
        f4 s = f4{0.f, 0.f, 0.f, 0.f};
        const float* q = slab + (int64_t)rg * stride + j;
        for (int r = 0; r < per; ++r) {
            const f4 x = *reinterpret_cast<const f4*>(q + (int64_t)r * 16 * stride);
            s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
        }
        if (rg < rows - 16 * per) {
            const f4 x = *reinterpret_cast<const f4*>(q + (int64_t)per * 16 * stride);
            s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
        }
        if (rg == 0) {
            t = s;
        } else {
            t.x += s.x; t.y += s.y; t.z += s.z; t.w += s.w;
        }
    }
    return t;
}

// W0's columns on the factored path: the gradient is the sum of the per-block
// partials of ncf_expand_grads (fact_expand_kernel), [nblk][dm][dm], user blocks
// [0, nbu) for W0[:, :dm], item blocks [nbu, nblk) for W0[:, dm:].  cols = 0: none.
struct W0Part {
    const float* p;
    int nbu, nblk, dm, cols;
};

// This thread's share (row group rg of 16) of the W0 gradient at tower column j.
__device__ __forceinline__ f4 w0_part_sum(const W0Part& P, int j, int rg) {
    f4 s = f4{0.f, 0.f, 0.f, 0.f};
    const int row = j / (2 * P.dm), col = j - row * 2 * P.dm;
    if (row >= P.dm) return s;  // alignment padding of the W0 segment
    const bool item = col >= P.dm;
    const int64_t off = (int64_t)row * P.dm + (item ? col - P.dm : col);
    const int b1 = item ? P.nblk : P.nbu;
    const int64_t bstride = (int64_t)P.dm * P.dm;
#pragma unroll 8
    for (int b = (item ? P.nbu : 0) + rg; b < b1; b += 16) {
        const f4 v = *reinterpret_cast<const f4*>(P.p + (int64_t)b * bstride + off);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    return s;
}

// One float4 column j of the slab reduction by the 16 row groups of a 256-thread
// block (thread = column c4 of 16, row group rg): the total, for the rg == 0 threads
// (j < stride); every thread of the block must call it (one barrier).
__device__ __forceinline__ f4 slab_column_total(const float* __restrict__ slab, int j, int stride, int rows,
                                                const W0Part& wp, int rg, int c4, f4 (*part)[16]) {
    f4 s = f4{0.f, 0.f, 0.f, 0.f};
    if (j < wp.cols) {
        s = w0_part_sum(wp, j, rg);
    } else if (j < stride) {
        const float* p = slab + (int64_t)rg * stride + j;
        const int per = rows / 16;
#pragma unroll 16
        for (int r = 0; r < per; ++r) {
            const f4 v = *reinterpret_cast<const f4*>(p + (int64_t)r * 16 * stride);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        if (rg < rows - 16 * per) {  // rows not a multiple of 16 (the layered path's single row)
            const f4 v = *reinterpret_cast<const f4*>(p + (int64_t)per * 16 * stride);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    part[rg][c4] = s;
    __syncthreads();
    f4 t = part[0][c4];
    if (rg == 0 && j < stride) {
#pragma unroll
        for (int q = 1; q < 16; ++q) {
            const f4 v = part[q][c4];
            t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
        }
    }
    return t;
}

// Loss bookkeeping of the step: done by one thread, no cross-block protocol.
__device__ __forceinline__ void record_loss(const ncf_step_ctl* ctl, const float* grads, int64_t loss_slot,
                                            float* loss_hist, int64_t hist_len) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && loss_hist != nullptr && loss_slot >= 0 && hist_len > 0) {
        const int64_t b = ctl->batch - 1;  // ncf_reduce_slab advanced it
        loss_hist[((b % hist_len) + hist_len) % hist_len] = grads[loss_slot];
    }
}

// reduce_adam_kernel (ncf_optim.hip) and lazy_adam_kernel (ncf_sparse.hip):
// Block of the tower part (blockIdx.x < nA): reduce 64 slab columns (W0's from the
// expansion's partials), apply Adam to the active ones in place; the loss column
// goes to the history.  sc[0..1] = (-step size, sqrt(bias correction 2)) of step t,
// computed by thread 0 of the block after its loads are in flight.
__device__ __forceinline__ void tower_reduce_adam_block(const float* __restrict__ slab, int lo, int stride, int rows,
                                                        int64_t tb, int64_t tower_len, float* __restrict__ p,
                                                        float* __restrict__ m, float* __restrict__ v, const Ranges& R,
                                                        int64_t t_step, int64_t b_step, double lr, double beta1,
                                                        double beta2, float eps, float* loss_hist, int64_t hist_len,
                                                        const W0Part& wp, float* sc, f4 (*part)[16],
                                                        const ScCache* scc, const float* __restrict__ pre = nullptr) {
#pragma clang fp contract(off)
    const ScCache sce = sc_peek(scc, t_step);  // arrives with the first slab loads
    const float w1 = (float)(1.0 - beta1);
    const float b2 = (float)beta2;
    const float omb2 = (float)(1.0 - beta2);
    const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int j = lo + (blockIdx.x * 16 + c4) * 4;
    // the updating threads' optimizer state, requested ahead of the slab reads
    const int64_t i = tb + j;
    const bool upd = rg == 0 && j < tower_len && in_ranges(R, i);
    f4 pp, mm, vv;
    if (upd) {
        pp = *reinterpret_cast<const f4*>(p + i);
        mm = *reinterpret_cast<const f4*>(m + i);
        vv = *reinterpret_cast<const f4*>(v + i);
    }
    f4 s = f4{0.f, 0.f, 0.f, 0.f};
    if (pre != nullptr) {  // the summed (all-reduced) tower gradient: tail of the packed buffer
        if (rg == 0 && j < stride) s = *reinterpret_cast<const f4*>(pre + j);
    } else if (j < wp.cols) {
        s = w0_part_sum(wp, j, rg);
    } else if (j < stride) {
        const float* q = slab + (int64_t)rg * stride + j;
        const int per = rows / 16;
#pragma unroll 16
        for (int r = 0; r < per; ++r) {
            const f4 x = *reinterpret_cast<const f4*>(q + (int64_t)r * 16 * stride);
            s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
        }
        if (rg < rows - 16 * per) {
            const f4 x = *reinterpret_cast<const f4*>(q + (int64_t)per * 16 * stride);
            s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
        }
    }
    part[rg][c4] = s;
    sc_resolve(sce, t_step, lr, beta1, beta2, sc);
    __syncthreads();
    const float neg_step = sc[0], bc2s = sc[1];
    if (rg == 0 && j < stride) {
        f4 gs = part[0][c4];
        if (pre == nullptr) {
#pragma unroll
            for (int q = 1; q < 16; ++q) {
                const f4 x = part[q][c4];
                gs.x += x.x; gs.y += x.y; gs.z += x.z; gs.w += x.w;
            }
        }
        if (j == tower_len) {
            if (loss_hist != nullptr && hist_len > 0) loss_hist[((b_step % hist_len) + hist_len) % hist_len] = gs.x;
        } else if (upd) {
            adam_f4(pp, mm, vv, gs, w1, b2, omb2, bc2s, eps, neg_step);
            *reinterpret_cast<f4*>(m + i) = mm;
            *reinterpret_cast<f4*>(v + i) = vv;
            *reinterpret_cast<f4*>(p + i) = pp;
        }
    }
}

}  // namespace ncf
