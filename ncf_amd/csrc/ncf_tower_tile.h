// The in-register MFMA tower tile shared by ncf_recommend.hip (full-catalogue top-K) and
// ncf_fold.hip (fold-in of unseen users): the padded shape constants, the layer step, the
// predict dot and the layer-0 projection chain.
//
// Register layout of a 16-item tile of one user (one wave): lane l = (g = l >> 4,
// it = l & 15) holds, for item `it`, the activations of columns 16 t + 4 g + r
// (t = 16-column tile, r = 0..3) as f4 h[t].  That is the B operand of MFMA4 for K-step
// (t, r) (B[k = g][j = it]); the A operand is W[16 o + it][16 t + 4 g + r], one 16-byte
// LDS read per four MFMAs, and the result D[i = 4 g + r'][j = it] is output column
// 16 o + 4 g + r' of item `it` -- the same layout again, so the tower runs in registers
// with no transposes.  Widths below 16 are zero padded (weights, biases, Pi, Pu).
#pragma once
#include "ncf_common.h"

namespace ncf {

constexpr int RC_CH = 64;  // items per LDS chunk of ncf_recommend (one seen-mask bit per lane)
// materialised paths (ncf_recommend, ncf_select_negatives): (user, item) pairs per chunk
constexpr int64_t RC_MAT_PAIRS = 1 << 17;

__host__ __device__ constexpr int rc_max(int a, int b) { return a > b ? a : b; }

template <int F_, int L_, int MODE_>
struct RcShape {
    static constexpr int F = F_, MODE = MODE_;
    static constexpr bool GMF = MODE != NCF_MODEL_MLP;
    static constexpr bool MLP = MODE != NCF_MODEL_GMF;
    static constexpr int L = MLP ? L_ : 1;
    static constexpr int DM = F << (L - 1);
    static constexpr int NL = MLP ? L - 1 : 0;  // tower layers after layer 0
    // padded width of layer k's output (k = 0: the layer-0 activation h1)
    __host__ __device__ static constexpr int KP(int k) { return rc_max(16, DM >> k); }
    __host__ __device__ static constexpr int T(int k) { return KP(k) / 16; }
    __host__ __device__ static constexpr int SW(int k) { return KP(k - 1) + 4; }  // LDS row stride of W_k
    __host__ __device__ static constexpr int wsize(int k) { return (MLP && k >= 1 && k <= NL) ? KP(k) * SW(k) : 0; }
    __host__ __device__ static constexpr int woff(int k) { return k <= 1 ? 0 : woff(k - 1) + wsize(k - 1); }
    __host__ __device__ static constexpr int boff(int k) { return k <= 1 ? 0 : boff(k - 1) + KP(k - 1); }
    static constexpr int W_TOTAL = woff(NL + 1);
    static constexpr int B_TOTAL = MLP ? boff(NL + 1) : 0;
    static constexpr int WP = MLP ? KP(NL) : 0;  // padded predict weights of the tower output
    static constexpr int KP0 = MLP ? KP(0) : 0;
    static constexpr int SP = MLP ? KP0 + 4 : 0;  // LDS row stride of the staged Pi chunk
    static constexpr int FP = GMF ? rc_max(16, F) : 0;
    static constexpr int TG = FP / 16;
    static constexpr int SG = GMF ? FP + 4 : 0;   // LDS row stride of the staged Ig chunk
    static constexpr int POFF = MODE == NCF_MODEL_NEUMF ? F : 0;
    static constexpr int FIXED = W_TOTAL + B_TOTAL + WP + RC_CH * (SP + SG);  // floats, all % 4 == 0
};

template <int TIN, int TOUT>
__device__ __forceinline__ void rc_layer(const f4 (&in)[TIN], f4 (&out)[TOUT], const float* W, const float* bias,
                                         int it, int g) {
    constexpr int SW = 16 * TIN + 4;
#pragma unroll
    for (int o = 0; o < TOUT; ++o) {
        f4 acc = *reinterpret_cast<const f4*>(bias + 16 * o + 4 * g);
#pragma unroll
        for (int t = 0; t < TIN; ++t) {
            const f4 w = *reinterpret_cast<const f4*>(W + (16 * o + it) * SW + 16 * t + 4 * g);
            acc = MFMA4(w.x, in[t].x, acc);
            acc = MFMA4(w.y, in[t].y, acc);
            acc = MFMA4(w.z, in[t].z, acc);
            acc = MFMA4(w.w, in[t].w, acc);
        }
        out[o].x = fmaxf(acc.x, 0.f);
        out[o].y = fmaxf(acc.y, 0.f);
        out[o].z = fmaxf(acc.z, 0.f);
        out[o].w = fmaxf(acc.w, 0.f);
    }
}

template <int TN>
__device__ __forceinline__ float rc_dot(const f4 (&h)[TN], const float* w, int g) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        const f4 v = *reinterpret_cast<const f4*>(w + 16 * t + 4 * g);
        s = fmaf(h[t].x, v.x, s);
        s = fmaf(h[t].y, v.y, s);
        s = fmaf(h[t].z, v.z, s);
        s = fmaf(h[t].w, v.w, s);
    }
    return s;
}

// One element of a layer-0 projection: the fmaf chain of x[0 .. n) against w[0 .. n), in
// column order from zero (Pi, Pu of ncf_recommend; Pi of ncf_fold_in: the same bits).
__device__ __forceinline__ float rc_proj_chain(const float* __restrict__ x, const float* __restrict__ w, int n) {
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc = fmaf(x[k], w[k], acc);
    return acc;
}

}  // namespace ncf
