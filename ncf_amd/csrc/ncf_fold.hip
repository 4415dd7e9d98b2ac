// Fold-in (ncf_fold_in, include/ncf_hip.h; added within ABI 21): fit the two vectors of
// users that were not in the training set to their interaction lists, with the item
// tables, the tower and the predict layer frozen.  Per folded user q, `steps` full-batch
// torch.optim.Adam steps on (ug | um) of
//   loss_q = mean_e BCEWithLogits(logit(ug, um, items[e]), labels[e]),  e in [ptr[q], ptr[q+1]).
// The whole optimisation of a user runs inside one launch: one workgroup per user.
//
// Prologue (both paths, one launch): Pi = Im W0[:, dm:]^T + b0 over the catalogue, tile_pi
// per element (ncf_tower_tile.h: the bits of ncf_recommend's Pi); the step scalars
// (-lr / (1 - beta1^t), sqrt(1 - beta2^t)) of t = t0 + 1 .. t0 + steps, once, by
// step_pair (ncf_adam.h): the two double pows are not evaluated inside the step loop; and,
// for calls of at most FD_ORDER_MAX users, the users ordered longest list first (workgroup b
// takes user order[b]: a user's step is a dependent chain, so the long lists set the tail
// and start first -- 41.1 -> 27.0 ms at the benchmark shape then).  A user's
// result does not depend on its position, so the order changes no bit.
//
// Fused path (NCF_FUSED_SHAPES, dm <= 64).  A workgroup of 4 waves stages in LDS the tower
// weights W_1 .. W_{L-1} in the layout rc_layer reads and, in the same pass, a transposed
// image of each for the data-gradient pass (its own loop, not tile_stage: fold_kernel is
// compiled to a register budget and keeps the code it was tuned with), the biases, the
// predict weights and W0[:, :dm] (row stride dm + 1).  Per step:
//   1. Pu = W0u um (thread c: the fmaf chain over k), Ag = wp_g * ug.
//   2. Wave w walks the 16-example tiles w, w + 4, ...: lane (g, it) gathers its columns of
//      the Pi row and the embed_item_GMF row of example `it` by item id (L2-resident
//      tables; streamed every step), h0 = relu(Pu + Pi) (tile_h0), layers 1.. on
//      v_mfma_f32_16x16x4_f32 (rc_layer), the logit (tile_gmf_dot, tile_logit),
//      dz = (sigmoid(z) - y) / n (0 past the user's last example), back through the tower
//      on the same MFMA with the transposed images and the ReLU masks of the activations
//      still in registers, and per lane, in tile order, acc += dpre0 ([dm]) and
//      acc += dz * ig ([f]).
//   3. Reduction in a fixed order: butterfly over the 16 item lanes (xor 1, 2, 4, 8), then
//      waves 0, 1, 2, 3 summed left to right from LDS.
//   4. dum = W0u^T S (thread k: the fmaf chain over c), dug = wp_g * Sg.
//   5. g = d + weight_decay * p, adam_1 on f + dm lanes (parameters and moments stay in
//      registers across steps).
//   6. thread 0 stores loss_out[q][t], the loss at the vectors before the update.
// Nothing else is written to global memory inside the step loop.  Every sum has a fixed
// order that depends on the user's examples alone, so a user's result does not depend on
// the other users of the call or on its position.
//
// Generic path (every other shape ncf_supported accepts, and every shape under
// ncf_debug_set_fold_path(NCF_PATH_LAYERED)): the same contract in plain fp32 fmaf loops,
// one workgroup per user, one example at a time, weights read from global memory, no
// MFMA.  It exists for correctness and coverage -- a second implementation of the same
// numbers -- not for speed.
#include <string.h>

#include "ncf_host.h"
#include "ncf_tower_tile.h"

namespace ncf {

static int g_fold_path = 0;  // ncf_debug_set_fold_path

constexpr int FD_THREADS = RC_WAVES * 64;
constexpr int FD_ORDER_MAX = 16384;  // users: the rank pass is quadratic; beyond, the tail is a small share

struct FoldArgs {
    ncf_layout lay;
    const float* params;
    const int64_t* ptr;
    const int32_t* items;
    const float* labels;
    int64_t nq;
    float* ug;
    float* um;
    float* m;  // [nq][f + dm] or NULL (with v): start from zero, discard
    float* v;
    float* loss_out;  // [nq][steps] or NULL
    float* grad_out;  // [nq][f + dm] or NULL
    const float* Pi;  // [item_num][kpi]
    const float* sc;  // [steps][2]
    const int32_t* order;  // [nq]: workgroup -> user, or NULL (identity)
    int kpi;
    int steps;
    float eps, wd, w1, b2, omb2;
};

// Prologue: Pi (b0 folded in; zero padded to kpi columns), the step scalars and, in the
// blocks from pro_blocks on, the users' order: order[rank(q)] = q with rank(q) = the users
// with a longer list, or an equal one and a lower index (a permutation; no atomics).
__global__ __launch_bounds__(256) void fold_pro_kernel(ncf_layout lay, const float* __restrict__ prm, int kpi,
                                                       float* __restrict__ Pi, float* __restrict__ sc, int steps,
                                                       int64_t t0, double lr, double beta1, double beta2,
                                                       unsigned pro_blocks, const int64_t* __restrict__ ptr, int nq,
                                                       int32_t* __restrict__ order) {
    if (blockIdx.x >= pro_blocks) {  // block-uniform
        __shared__ int64_t len[256];
        const int q = (int)(blockIdx.x - pro_blocks) * 256 + threadIdx.x;
        const int64_t mine = q < nq ? ptr[q + 1] - ptr[q] : 0;
        int rank = 0;
        for (int b = 0; b < nq; b += 256) {
            __syncthreads();
            const int o = b + threadIdx.x;
            len[threadIdx.x] = o < nq ? ptr[o + 1] - ptr[o] : -1;
            __syncthreads();
            const int cnt = nq - b < 256 ? nq - b : 256;
            for (int j = 0; j < cnt; ++j) rank += (len[j] > mine) || (len[j] == mine && b + j < q);
        }
        if (q < nq) order[rank] = q;
        return;
    }
    const int DM = lay.factor_num << (lay.num_layers - 1);
    const int64_t n_pi = (int64_t)lay.item_num * kpi;
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n_pi) {
        const int64_t row = idx / kpi;
        Pi[idx] = tile_pi(lay, prm, row, (int)(idx - row * kpi), DM);
        return;
    }
    idx -= n_pi;
    if (idx < steps) step_pair(t0 + 1 + idx, lr, beta1, beta2, &sc[2 * idx], &sc[2 * idx + 1]);
}

// Data-gradient step of one tower layer on the transposed image WT[c][o] (row stride
// 16 TIN + 4): out[o'] (columns of the layer's input) = sum_o W[o][c] in[o], the A operand
// being WT[16 o' + it][16 t + 4 g + r] -- rc_layer without bias and ReLU.
template <int TIN, int TOUT>
__device__ __forceinline__ void fold_layer_t(const f4 (&in)[TIN], f4 (&out)[TOUT], const float* WT, int it, int g) {
    constexpr int ST = 16 * TIN + 4;
#pragma unroll
    for (int o = 0; o < TOUT; ++o) {
        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < TIN; ++t) {
            const f4 w = *reinterpret_cast<const f4*>(WT + (16 * o + it) * ST + 16 * t + 4 * g);
            acc = MFMA4(w.x, in[t].x, acc);
            acc = MFMA4(w.y, in[t].y, acc);
            acc = MFMA4(w.z, in[t].z, acc);
            acc = MFMA4(w.w, in[t].w, acc);
        }
        out[o] = acc;
    }
}

// d = (h > 0) ? d : 0 (ReLU backward from the activation)
template <int TN>
__device__ __forceinline__ void fold_mask(f4 (&d)[TN], const f4 (&h)[TN]) {
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        d[t].x = h[t].x > 0.f ? d[t].x : 0.f;
        d[t].y = h[t].y > 0.f ? d[t].y : 0.f;
        d[t].z = h[t].z > 0.f ? d[t].z : 0.f;
        d[t].w = h[t].w > 0.f ? d[t].w : 0.f;
    }
}

// d = (h > 0) ? dz * wp : 0: the predict layer's data gradient at the tower output
template <int TN>
__device__ __forceinline__ void fold_top(f4 (&d)[TN], const f4 (&h)[TN], const float* wp, float dz, int g) {
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        const f4 w = *reinterpret_cast<const f4*>(wp + 16 * t + 4 * g);
        d[t].x = h[t].x > 0.f ? dz * w.x : 0.f;
        d[t].y = h[t].y > 0.f ? dz * w.y : 0.f;
        d[t].z = h[t].z > 0.f ? dz * w.z : 0.f;
        d[t].w = h[t].w > 0.f ? dz * w.w : 0.f;
    }
}

__device__ __forceinline__ float fold_lanes16(float v) {
    v += shfl_xor(v, 1);
    v += shfl_xor(v, 2);
    v += shfl_xor(v, 4);
    v += shfl_xor(v, 8);
    return v;
}

// LDS floats of the fused kernel
template <int F, int L, int MODE>
struct FoldShape : RcShape<F, L, MODE> {
    using C = RcShape<F, L, MODE>;
    // transposed image of W_k: KP(k - 1) rows (input columns) of KP(k) + 4 floats
    __host__ __device__ static constexpr int ST(int k) { return C::KP(k) + 4; }
    __host__ __device__ static constexpr int wtsize(int k) { return (C::MLP && k >= 1 && k <= C::NL) ? C::KP(k - 1) * ST(k) : 0; }
    __host__ __device__ static constexpr int wtoff(int k) { return k <= 1 ? 0 : wtoff(k - 1) + wtsize(k - 1); }
    static constexpr int WT_TOTAL = wtoff(C::NL + 1);
    static constexpr int S0 = C::DM + 1;                     // row stride of the staged W0[:, :dm]
    static constexpr int W0U4 = C::MLP ? (C::DM * S0 + 3) & ~3 : 0;
    static constexpr int RS = C::KP0 + C::FP + 4;            // reduction row: dpre0 sums, dz ig sums, loss (+ pad)
    static constexpr int TOTAL = C::W_TOTAL + WT_TOTAL + C::B_TOTAL + C::WP + W0U4 + 2 * (C::KP0 + C::FP) /* p, (Pu | Ag) */ +
                                 (RC_WAVES + 1) * RS;
};

// Compiled for two waves per SIMD (two workgroups per CU).  Left alone the compiler keeps
// the tower weights of the tile loop in registers (245 VGPRs + 28 AGPRs at NeuMF(16,3): one
// wave per SIMD); with the budget of 256 it spills 4 VGPRs (20 bytes of scratch) and the
// benchmark call takes 19.4 ms instead of 27.0.  Three waves spill 95.
template <int F, int L, int MODE>
__global__ __launch_bounds__(FD_THREADS, 2) void fold_kernel(FoldArgs a) {
#pragma clang fp contract(off)
    using C = RcShape<F, L, MODE>;
    using S = FoldShape<F, L, MODE>;
    __shared__ f4 smem4[S::TOTAL / 4];
    static_assert(S::TOTAL % 4 == 0 && S::TOTAL * 4 <= 64 * 1024, "fold_kernel LDS");
    float* const Wl = reinterpret_cast<float*>(smem4);
    float* const WTl = Wl + C::W_TOTAL;
    float* const Bl = WTl + S::WT_TOTAL;
    float* const WPl = Bl + C::B_TOTAL;
    float* const W0l = WPl + C::WP;
    float* const umL = W0l + S::W0U4;    // [KP0]
    float* const ugL = umL + C::KP0;     // [FP]
    float* const PuL = ugL + C::FP;      // [KP0]
    float* const AgL = PuL + C::KP0;     // [FP]
    float* const red = AgL + C::FP;      // [RC_WAVES][RS]
    float* const Sl = red + RC_WAVES * S::RS;  // [RS]
    constexpr int LOSS = C::KP0 + C::FP;
    constexpr int DM = C::DM;
    constexpr int T0 = C::MLP ? C::T(0) : 1, T1 = C::T(1), T2 = C::T(2), T3 = C::T(3), TG = C::GMF ? C::TG : 1;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, it = lane & 15;
    const float* __restrict__ prm = a.params;
    const int64_t q = a.order != nullptr ? a.order[blockIdx.x] : blockIdx.x;
    const int64_t e0 = a.ptr[q];
    const int64_t n = a.ptr[q + 1] - e0;
    const float nf = (float)n;
    const int64_t ntiles = (n + 15) >> 4;
    const int DMS = F << (a.lay.num_layers - 1);  // the table's row (GMF type: not C::DM)
    const int W = F + DMS;                        // floats per user of the state and the gradient

    if constexpr (C::MLP) {
#pragma unroll
        for (int k = 1; k <= C::NL; ++k) {
            const int rows = C::KP(k), cols = C::KP(k - 1), sw = C::SW(k), st = S::ST(k);
            const int out = DM >> k, in = DM >> (k - 1);
            const float* w = prm + a.lay.w[k];
            for (int idx = tid; idx < rows * cols; idx += FD_THREADS) {
                const int r = idx / cols, c = idx - r * cols;
                const float x = (r < out && c < in) ? w[r * in + c] : 0.f;
                Wl[C::woff(k) + r * sw + c] = x;
                WTl[S::wtoff(k) + c * st + r] = x;
            }
            for (int idx = tid; idx < rows; idx += FD_THREADS)
                Bl[C::boff(k) + idx] = idx < out ? prm[a.lay.b[k] + idx] : 0.f;
        }
        for (int idx = tid; idx < C::WP; idx += FD_THREADS) WPl[idx] = idx < F ? prm[a.lay.wp + C::POFF + idx] : 0.f;
        for (int idx = tid; idx < DM * DM; idx += FD_THREADS) {
            const int r = idx / DM, c = idx - r * DM;
            W0l[r * S::S0 + c] = prm[a.lay.w[0] + (int64_t)r * 2 * DM + c];
        }
        for (int idx = tid; idx < C::KP0; idx += FD_THREADS) {
            umL[idx] = idx < DM ? a.um[q * DM + idx] : 0.f;
            PuL[idx] = 0.f;
        }
    }
    if constexpr (C::GMF) {
        for (int idx = tid; idx < C::FP; idx += FD_THREADS) {
            ugL[idx] = idx < F ? a.ug[q * F + idx] : 0.f;
            AgL[idx] = 0.f;
        }
    }
    const float bp = prm[a.lay.bp];

    // this thread's optimizer element: wave 0 the MLP vector, wave 1 the GMF vector
    const bool own_m = C::MLP && tid < DM;
    const bool own_g = C::GMF && tid >= 64 && tid < 64 + F;
    const int own_col = own_m ? F + tid : tid - 64;  // column of (ug | um)
    float p = 0.f, mo = 0.f, vo = 0.f, gr = 0.f, wpg = 0.f;
    if (own_m) p = a.um[q * DM + tid];
    if (own_g) {
        p = a.ug[q * F + (tid - 64)];
        wpg = prm[a.lay.wp + (tid - 64)];
    }
    if ((own_m || own_g) && a.m != nullptr) {
        mo = a.m[q * W + own_col];
        vo = a.v[q * W + own_col];
    }
    __syncthreads();

    for (int s = 0; s < a.steps; ++s) {
        // 1. Pu, Ag at the current vectors
        if (own_m) {
            float acc = 0.f;
            for (int k = 0; k < DM; ++k) acc = fmaf(umL[k], W0l[tid * S::S0 + k], acc);
            PuL[tid] = acc;
        }
        if (own_g) AgL[tid - 64] = wpg * p;
        __syncthreads();

        // 2. the user's examples, 16 per tile
        f4 pu[T0], ag[TG], accP[T0], accG[TG];
        float lacc = 0.f;
#pragma unroll
        for (int t = 0; t < T0; ++t) {
            accP[t] = f4{0.f, 0.f, 0.f, 0.f};
            if constexpr (C::MLP) pu[t] = *reinterpret_cast<const f4*>(PuL + 16 * t + 4 * g);
        }
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            accG[t] = f4{0.f, 0.f, 0.f, 0.f};
            if constexpr (C::GMF) ag[t] = *reinterpret_cast<const f4*>(AgL + 16 * t + 4 * g);
        }
#pragma unroll 1
        for (int64_t tile = wave; tile < ntiles; tile += RC_WAVES) {
            const int64_t e = tile * 16 + it;
            const bool valid = e < n;
            const int item = valid ? a.items[e0 + e] : 0;
            const float y = valid ? a.labels[e0 + e] : 0.f;
            f4 h0[T0], h1[T1], h2[T2], h3[T3], ig[TG];
            float part = 0.f;
            if constexpr (C::MLP) {
#pragma unroll
                for (int t = 0; t < T0; ++t)
                    h0[t] = tile_h0(pu[t],
                                    *reinterpret_cast<const f4*>(a.Pi + (int64_t)item * C::KP0 + 16 * t + 4 * g));
                if constexpr (C::NL >= 1) rc_layer(h0, h1, Wl + C::woff(1), Bl + C::boff(1), it, g);
                if constexpr (C::NL >= 2) rc_layer(h1, h2, Wl + C::woff(2), Bl + C::boff(2), it, g);
                if constexpr (C::NL >= 3) rc_layer(h2, h3, Wl + C::woff(3), Bl + C::boff(3), it, g);
                if constexpr (C::NL == 0) part = rc_dot(h0, WPl, g);
                if constexpr (C::NL == 1) part = rc_dot(h1, WPl, g);
                if constexpr (C::NL == 2) part = rc_dot(h2, WPl, g);
                if constexpr (C::NL == 3) part = rc_dot(h3, WPl, g);
            }
            if constexpr (C::GMF) part += tile_gmf_dot<C>(ag, ig, prm + a.lay.ig + (int64_t)item * F, g);
            const float z = tile_logit(part, bp);  // the same bits in the four lanes of an example
            const float dz = valid ? (sigmoidf_(z) - y) / nf : 0.f;
            if (valid && g == 0) lacc += bce_loss(z, y);

            if constexpr (C::MLP) {
                f4 d0[T0];
                if constexpr (C::NL == 0) {
                    fold_top(d0, h0, WPl, dz, g);
                } else if constexpr (C::NL == 1) {
                    f4 d1[T1];
                    fold_top(d1, h1, WPl, dz, g);
                    fold_layer_t(d1, d0, WTl + S::wtoff(1), it, g);
                    fold_mask(d0, h0);
                } else if constexpr (C::NL == 2) {
                    f4 d1[T1], d2[T2];
                    fold_top(d2, h2, WPl, dz, g);
                    fold_layer_t(d2, d1, WTl + S::wtoff(2), it, g);
                    fold_mask(d1, h1);
                    fold_layer_t(d1, d0, WTl + S::wtoff(1), it, g);
                    fold_mask(d0, h0);
                } else {
                    f4 d1[T1], d2[T2], d3[T3];
                    fold_top(d3, h3, WPl, dz, g);
                    fold_layer_t(d3, d2, WTl + S::wtoff(3), it, g);
                    fold_mask(d2, h2);
                    fold_layer_t(d2, d1, WTl + S::wtoff(2), it, g);
                    fold_mask(d1, h1);
                    fold_layer_t(d1, d0, WTl + S::wtoff(1), it, g);
                    fold_mask(d0, h0);
                }
#pragma unroll
                for (int t = 0; t < T0; ++t) {
                    accP[t].x += d0[t].x;
                    accP[t].y += d0[t].y;
                    accP[t].z += d0[t].z;
                    accP[t].w += d0[t].w;
                }
            }
            if constexpr (C::GMF) {
#pragma unroll
                for (int t = 0; t < TG; ++t) {
                    accG[t].x = fmaf(dz, ig[t].x, accG[t].x);
                    accG[t].y = fmaf(dz, ig[t].y, accG[t].y);
                    accG[t].z = fmaf(dz, ig[t].z, accG[t].z);
                    accG[t].w = fmaf(dz, ig[t].w, accG[t].w);
                }
            }
        }

        // 3. the 16 item lanes, then the 4 waves, in a fixed order
        float* const rw = red + wave * S::RS;
        if constexpr (C::MLP) {
#pragma unroll
            for (int t = 0; t < T0; ++t) {
                f4 x;
                x.x = fold_lanes16(accP[t].x);
                x.y = fold_lanes16(accP[t].y);
                x.z = fold_lanes16(accP[t].z);
                x.w = fold_lanes16(accP[t].w);
                if (it == 0) *reinterpret_cast<f4*>(rw + 16 * t + 4 * g) = x;
            }
        }
        if constexpr (C::GMF) {
#pragma unroll
            for (int t = 0; t < TG; ++t) {
                f4 x;
                x.x = fold_lanes16(accG[t].x);
                x.y = fold_lanes16(accG[t].y);
                x.z = fold_lanes16(accG[t].z);
                x.w = fold_lanes16(accG[t].w);
                if (it == 0) *reinterpret_cast<f4*>(rw + C::KP0 + 16 * t + 4 * g) = x;
            }
        }
        lacc = fold_lanes16(lacc);
        if (lane == 0) rw[LOSS] = lacc;
        __syncthreads();
        if (tid <= LOSS) Sl[tid] = ((red[tid] + red[S::RS + tid]) + red[2 * S::RS + tid]) + red[3 * S::RS + tid];
        __syncthreads();

        // 4.-6. gradient, Adam, loss
        const bool last = s == a.steps - 1;
        if (own_m) {
            float acc = 0.f;
            for (int c = 0; c < DM; ++c) acc = fmaf(W0l[c * S::S0 + tid], Sl[c], acc);
            gr = fmaf(a.wd, p, acc);
        }
        if (own_g) gr = fmaf(a.wd, p, wpg * Sl[C::KP0 + (tid - 64)]);
        if (own_m || own_g) {
            const float neg_step = a.sc[2 * s], bc2s = a.sc[2 * s + 1];
            p = adam_1(p, mo, vo, gr, a.w1, a.b2, a.omb2, bc2s, a.eps, neg_step);
            if (own_m) umL[tid] = p;
        }
        if (tid == 0 && a.loss_out != nullptr) a.loss_out[q * a.steps + s] = n > 0 ? Sl[LOSS] / nf : 0.f;
        if (!last) __syncthreads();
    }

    if (own_m) a.um[q * DM + tid] = p;
    if (own_g) a.ug[q * F + (tid - 64)] = p;
    if (own_m || own_g) {
        if (a.m != nullptr) {
            a.m[q * W + own_col] = mo;
            a.v[q * W + own_col] = vo;
        }
        if (a.grad_out != nullptr) a.grad_out[q * W + own_col] = gr;
    }
    if (a.grad_out != nullptr) {
        // the half this model type does not train: gradient 0
        if (!C::MLP)
            for (int k = tid; k < DMS; k += FD_THREADS) a.grad_out[q * W + F + k] = 0.f;
        if (!C::GMF && tid >= 64 && tid < 64 + F) a.grad_out[q * W + (tid - 64)] = 0.f;
    }
}

// ---------------------------------------------------------------------------
// Generic path.  LDS (floats): um [DM], Pu [DM], S [DM], h [2 DM] (the activations of
// layers 0 .. NL back to back), d [2 DM] (their gradients, same offsets), ug [F], Ag [F],
// Sg [F], ig [F], m / v [2 (F + DM)], scalars [4].
struct FgShape {
    int um, pu, s, h, d, ug, ag, sg, ig, m, v, misc, total;
};
static FgShape fg_shape(int F, int DM) {
    FgShape o;
    int x = 0;
    o.um = x; x += DM;
    o.pu = x; x += DM;
    o.s = x; x += DM;
    o.h = x; x += 2 * DM;
    o.d = x; x += 2 * DM;
    o.ug = x; x += F;
    o.ag = x; x += F;
    o.sg = x; x += F;
    o.ig = x; x += F;
    o.m = x; x += F + DM;
    o.v = x; x += F + DM;
    o.misc = x; x += 4;
    o.total = x;
    return o;
}

__global__ __launch_bounds__(FD_THREADS) void fold_generic_kernel(FoldArgs a, FgShape sh) {
#pragma clang fp contract(off)
    extern __shared__ f4 fold_smem4[];
    float* const smem = reinterpret_cast<float*>(fold_smem4);
    const int F = a.lay.factor_num, Lk = a.lay.num_layers, MODE = a.lay.model_type;
    const bool GMF = MODE != NCF_MODEL_MLP, MLP = MODE != NCF_MODEL_GMF;
    const int DM = F << (Lk - 1), NL = Lk - 1, W = F + DM;
    const int POFF = MODE == NCF_MODEL_NEUMF ? F : 0;
    float* const umL = smem + sh.um;
    float* const PuL = smem + sh.pu;
    float* const Sl = smem + sh.s;
    float* const hL = smem + sh.h;
    float* const dL = smem + sh.d;
    float* const ugL = smem + sh.ug;
    float* const AgL = smem + sh.ag;
    float* const SgL = smem + sh.sg;
    float* const igL = smem + sh.ig;
    float* const mL = smem + sh.m;
    float* const vL = smem + sh.v;
    const int tid = threadIdx.x;
    const float* __restrict__ prm = a.params;
    const int64_t q = a.order != nullptr ? a.order[blockIdx.x] : blockIdx.x;
    const int64_t e0 = a.ptr[q];
    const int64_t n = a.ptr[q + 1] - e0;
    const float nf = (float)n;
    const float bp = prm[a.lay.bp];
    const float* const wpt = prm + a.lay.wp + POFF;  // predict weights of the tower output
    const float* const wpg = prm + a.lay.wp;         // ... of the GMF product

    for (int c = tid; c < DM; c += FD_THREADS) umL[c] = a.um[q * DM + c];
    for (int f = tid; f < F; f += FD_THREADS) ugL[f] = a.ug[q * F + f];
    for (int j = tid; j < W; j += FD_THREADS) {
        mL[j] = a.m != nullptr ? a.m[q * W + j] : 0.f;
        vL[j] = a.m != nullptr ? a.v[q * W + j] : 0.f;
    }
    __syncthreads();

    for (int s = 0; s < a.steps; ++s) {
        if (MLP) {
            for (int c = tid; c < DM; c += FD_THREADS) {
                const float* w = prm + a.lay.w[0] + (int64_t)c * 2 * DM;
                float acc = 0.f;
                for (int k = 0; k < DM; ++k) acc = fmaf(umL[k], w[k], acc);
                PuL[c] = acc;
                Sl[c] = 0.f;
            }
        }
        if (GMF) {
            for (int f = tid; f < F; f += FD_THREADS) {
                AgL[f] = wpg[f] * ugL[f];
                SgL[f] = 0.f;
            }
        }
        float lacc = 0.f;  // thread 0's
        __syncthreads();

        for (int64_t e = 0; e < n; ++e) {
            const int item = a.items[e0 + e];
            const float y = a.labels[e0 + e];
            if (MLP) {
                const float* pi = a.Pi + (int64_t)item * a.kpi;
                for (int c = tid; c < DM; c += FD_THREADS) hL[c] = fmaxf(PuL[c] + pi[c], 0.f);
            }
            if (GMF) {
                for (int f = tid; f < F; f += FD_THREADS) igL[f] = prm[a.lay.ig + (int64_t)item * F + f];
            }
            __syncthreads();
            int hoff = 0;  // offset of layer k - 1's activation
            if (MLP) {
                for (int k = 1; k <= NL; ++k) {
                    const int in = DM >> (k - 1), out = DM >> k;
                    const float* w = prm + a.lay.w[k];
                    const float* b = prm + a.lay.b[k];
                    const float* hin = hL + hoff;
                    float* hout = hL + hoff + in;
                    for (int o = tid; o < out; o += FD_THREADS) {
                        float acc = b[o];
                        for (int c = 0; c < in; ++c) acc = fmaf(w[(int64_t)o * in + c], hin[c], acc);
                        hout[o] = fmaxf(acc, 0.f);
                    }
                    hoff += in;
                    __syncthreads();
                }
            }
            // the logit, by every thread (the same chain, the same bits)
            float z = 0.f;
            if (MLP) {
                const float* htop = hL + hoff;
                for (int o = 0; o < F; ++o) z = fmaf(htop[o], wpt[o], z);
            }
            if (GMF) {
                float sg = 0.f;
                for (int f = 0; f < F; ++f) sg = fmaf(AgL[f], igL[f], sg);
                z += sg;
            }
            z += bp;
            const float dz = (sigmoidf_(z) - y) / nf;
            if (tid == 0) lacc += bce_loss(z, y);
            if (GMF) {
                for (int f = tid; f < F; f += FD_THREADS) SgL[f] = fmaf(dz, igL[f], SgL[f]);
            }
            if (MLP) {
                // top: d_NL = (h_NL > 0) dz wp; NL == 0: straight into S
                const float* htop = hL + hoff;
                if (NL == 0) {
                    for (int c = tid; c < DM; c += FD_THREADS) Sl[c] += htop[c] > 0.f ? dz * wpt[c] : 0.f;
                } else {
                    for (int o = tid; o < F; o += FD_THREADS) dL[hoff + o] = htop[o] > 0.f ? dz * wpt[o] : 0.f;
                    __syncthreads();
                    for (int k = NL; k >= 1; --k) {
                        const int in = DM >> (k - 1), out = DM >> k;
                        const float* w = prm + a.lay.w[k];
                        const float* dout = dL + hoff;
                        hoff -= in;
                        const float* hin = hL + hoff;
                        for (int c = tid; c < in; c += FD_THREADS) {
                            float acc = 0.f;
                            for (int o = 0; o < out; ++o) acc = fmaf(w[(int64_t)o * in + c], dout[o], acc);
                            acc = hin[c] > 0.f ? acc : 0.f;
                            if (k == 1) Sl[c] += acc; else dL[hoff + c] = acc;
                        }
                        __syncthreads();
                    }
                }
            }
            // (the next example's first barrier orders its h / ig writes after this one's reads
            // of other layers; h0 / ig / S / Sg elements are touched by their owner thread alone)
            if (MLP && NL == 0) __syncthreads();
            if (!MLP) __syncthreads();
        }
        __syncthreads();

        const float neg_step = a.sc[2 * s], bc2s = a.sc[2 * s + 1];
        const bool last = s == a.steps - 1;
        if (MLP) {
            for (int k = tid; k < DM; k += FD_THREADS) {
                const float* w = prm + a.lay.w[0] + k;
                float acc = 0.f;
                for (int c = 0; c < DM; ++c) acc = fmaf(w[(int64_t)c * 2 * DM], Sl[c], acc);
                const float p = umL[k];
                const float gr = fmaf(a.wd, p, acc);
                float mo = mL[F + k], vo = vL[F + k];
                const float pn = adam_1(p, mo, vo, gr, a.w1, a.b2, a.omb2, bc2s, a.eps, neg_step);
                mL[F + k] = mo;
                vL[F + k] = vo;
                umL[k] = pn;
                if (last && a.grad_out != nullptr) a.grad_out[q * W + F + k] = gr;
            }
        } else if (last && a.grad_out != nullptr) {
            for (int k = tid; k < DM; k += FD_THREADS) a.grad_out[q * W + F + k] = 0.f;
        }
        if (GMF) {
            for (int f = tid; f < F; f += FD_THREADS) {
                const float p = ugL[f];
                const float gr = fmaf(a.wd, p, wpg[f] * SgL[f]);
                float mo = mL[f], vo = vL[f];
                ugL[f] = adam_1(p, mo, vo, gr, a.w1, a.b2, a.omb2, bc2s, a.eps, neg_step);
                mL[f] = mo;
                vL[f] = vo;
                if (last && a.grad_out != nullptr) a.grad_out[q * W + f] = gr;
            }
        } else if (last && a.grad_out != nullptr) {
            for (int f = tid; f < F; f += FD_THREADS) a.grad_out[q * W + f] = 0.f;
        }
        if (tid == 0 && a.loss_out != nullptr) a.loss_out[q * a.steps + s] = n > 0 ? lacc / nf : 0.f;
        __syncthreads();
    }

    if (MLP) {
        for (int c = tid; c < DM; c += FD_THREADS) a.um[q * DM + c] = umL[c];
    }
    if (GMF) {
        for (int f = tid; f < F; f += FD_THREADS) a.ug[q * F + f] = ugL[f];
    }
    if (a.m != nullptr) {
        for (int j = tid; j < W; j += FD_THREADS) {
            const bool active = j < F ? GMF : MLP;
            if (active) {
                a.m[q * W + j] = mL[j];
                a.v[q * W + j] = vL[j];
            }
        }
    }
}

template <int F, int L, int MODE>
struct FoldKernel {
    static constexpr auto kernel = &fold_kernel<F, L, MODE>;
};
static const TileEntry* fold_fused(const ncf_layout* lay) { return tile_fused<FoldKernel>(lay, g_fold_path); }

// Pi columns per item: the fused kernel's padded width, dm on the generic path, 0 for GMF.
static int fold_kpi(const ncf_layout* lay) {
    if (lay->model_type == NCF_MODEL_GMF) return 0;
    const TileEntry* e = fold_fused(lay);
    return e ? e->kp0 : lay->factor_num << (lay->num_layers - 1);
}

}  // namespace ncf

using namespace ncf;

extern "C" {

int ncf_debug_set_fold_path(int path) { return set_debug_path(&g_fold_path, path); }

int64_t ncf_fold_in_workspace_bytes(const ncf_layout* lay, int64_t n_users, int64_t n_examples, int steps) {
    if (!lay || n_users < 0 || n_examples < 0 || steps < 1 || lay->item_num <= 0) return -1;
    if (!ncf_supported(lay->model_type, lay->factor_num, lay->num_layers)) return -1;
    if (n_users == 0) return 0;
    return ws_align((int64_t)lay->item_num * fold_kpi(lay) * 4) + ws_align((int64_t)steps * 8) +
           (n_users <= FD_ORDER_MAX ? ws_align(n_users * 4) : 0);
}

int ncf_fold_in(const ncf_layout* lay, const float* params, const int64_t* ex_ptr, const int32_t* ex_items,
                const float* ex_labels, int64_t n_users, int64_t n_examples, float* ug, float* um, float* exp_avg,
                float* exp_avg_sq, const ncf_fold_opt* opt, float* loss_out, float* grad_out, void* workspace,
                int64_t workspace_bytes, void* stream) {
    if (!lay || !opt || n_users < 0 || n_examples < 0) return NCF_E_ARG;
    if (opt->steps < 1 || opt->t0 < 0) return NCF_E_ARG;
    if ((exp_avg == nullptr) != (exp_avg_sq == nullptr)) return NCF_E_ARG;
    if (n_users == 0) return NCF_OK;
    if (!params || !ex_ptr || !ug || !um || !workspace) return NCF_E_ARG;
    if (n_examples > 0 && (!ex_items || !ex_labels)) return NCF_E_ARG;
    if (!ncf_supported(lay->model_type, lay->factor_num, lay->num_layers)) return NCF_E_UNSUPPORTED;
    if (n_users > 0x7fffffff) return NCF_E_ARG;
    const int64_t need = ncf_fold_in_workspace_bytes(lay, n_users, n_examples, opt->steps);
    if (need < 0 || workspace_bytes < need) return NCF_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const int kpi = fold_kpi(lay);
    const int64_t n_pi = (int64_t)lay->item_num * kpi;

    FoldArgs a;
    memset(&a, 0, sizeof(a));
    a.lay = *lay;
    a.params = params;
    a.ptr = ex_ptr;
    a.items = ex_items;
    a.labels = ex_labels;
    a.nq = n_users;
    a.ug = ug;
    a.um = um;
    a.m = exp_avg;
    a.v = exp_avg_sq;
    a.loss_out = loss_out;
    a.grad_out = grad_out;
    a.Pi = reinterpret_cast<const float*>(ws);
    a.sc = reinterpret_cast<const float*>(ws + ws_align(n_pi * 4));
    const bool ordered = n_users <= FD_ORDER_MAX;
    if (ordered) a.order = reinterpret_cast<const int32_t*>(ws + ws_align(n_pi * 4) + ws_align((int64_t)opt->steps * 8));
    a.kpi = kpi;
    a.steps = opt->steps;
    a.eps = opt->eps;
    a.wd = opt->weight_decay;
    a.w1 = (float)(1.0 - opt->beta1);
    a.b2 = (float)opt->beta2;
    a.omb2 = (float)(1.0 - opt->beta2);

    const TileEntry* e = fold_fused(lay);
    const FgShape sh = fg_shape(lay->factor_num, lay->factor_num << (lay->num_layers - 1));
    const int64_t lds = ((int64_t)sh.total * 4 + 15) & ~(int64_t)15;
    if (!e) {
        if (lds > LDS_LIMIT_BYTES) return NCF_E_UNSUPPORTED;
        if (lds > 64 * 1024 && ensure_lds(reinterpret_cast<const void*>(&fold_generic_kernel), lds) != NCF_OK)
            return NCF_E_LAUNCH;
    }
    const int64_t npro = n_pi + opt->steps;
    const unsigned pro_blocks = (unsigned)((npro + 255) / 256);
    const unsigned order_blocks = ordered ? (unsigned)((n_users + 255) / 256) : 0;
    hipLaunchKernelGGL(fold_pro_kernel, dim3(pro_blocks + order_blocks), dim3(256), 0, st, *lay, params, kpi,
                       const_cast<float*>(a.Pi), const_cast<float*>(a.sc), a.steps, opt->t0, opt->lr, opt->beta1,
                       opt->beta2, pro_blocks, ex_ptr, (int)n_users, const_cast<int32_t*>(a.order));
    if (e) {
        void* args[] = {&a};
        if (hipLaunchKernel(e->fn, dim3((unsigned)n_users), dim3(FD_THREADS), args, 0, st) != hipSuccess)
            return NCF_E_LAUNCH;
    } else {
        hipLaunchKernelGGL(fold_generic_kernel, dim3((unsigned)n_users), dim3(FD_THREADS), (size_t)lds, st, a, sh);
    }
    return launch_status();
}

}  // extern "C"
