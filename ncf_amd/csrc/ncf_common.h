// Shared definitions for the NeuMF HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ncf_hip.h"

typedef float f4 __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x4_f32: exact f32 FMA chain, 32-cycle issue per SIMD.
//   A operand: lane l holds A[i = l&15][k = l>>4]
//   B operand: lane l holds B[k = l>>4][j = l&15]
//   C/D      : lane l, reg r holds C[i = 4*(l>>4) + r][j = l&15]
#define MFMA4(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

static constexpr int WAVE = 64;

__device__ __forceinline__ float lane_get(const f4& v, int r) {
    return r == 0 ? v.x : (r == 1 ? v.y : (r == 2 ? v.z : v.w));
}

__device__ __forceinline__ float shfl_xor(float v, int m) { return __shfl_xor(v, m, 64); }

// Exact reference-order BCE-with-logits pieces (torch binary_cross_entropy_with_logits):
//   loss = (1 - y) * x + m + log(exp(-m) + exp(-x - m)),  m = max(-x, 0)
__device__ __forceinline__ float bce_loss(float x, float y) {
    float m = fmaxf(-x, 0.0f);
    return (1.0f - y) * x + m + logf(expf(-m) + expf(-x - m));
}
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// Dropout keep hash (include/ncf_hip.h ncf_dropout_hash): splitmix64 finalizer of
// the mixed (seed, step, layer, row, column), upper 32 bits.
__host__ __device__ __forceinline__ uint32_t dropout_hash(uint32_t seed, uint32_t t, uint32_t layer, int64_t row,
                                                          uint32_t col) {
    uint64_t x = ((uint64_t)seed << 32) ^ ((uint64_t)t * 0x9E3779B97F4A7C15ull) ^
                 ((uint64_t)row * 0xBF58476D1CE4E5B9ull) ^ ((uint64_t)((layer << 16) | col) * 0x94D049BB133111EBull);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)(x >> 32);
}

// ---------------------------------------------------------------------------
// Running top-K lists shared by ncf_recommend and ncf_neighbors: K entries sorted by
// score descending, then id ascending (a total order), one wave per list.
namespace ncf {

// Workspace layouts: every piece starts on a 256-byte boundary
inline int64_t ws_align(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

constexpr int RC_WAVES = 4;
constexpr int RC_MAXK = 128;
constexpr int RC_IDMAX = 0x7fffffff;  // id of an empty list slot (sorts last)

__device__ __forceinline__ bool rc_better(float s, int id, float ts, int ti) {
    return s > ts || (s == ts && id < ti);
}

// Wave-wide insert of the candidates lanes 0..15 hold (ascending ids) into the sorted
// list ls / li of K entries.  The common case is the one compare against entry K - 1.
__device__ __forceinline__ void rc_feed(volatile float* ls, volatile int* li, int K, float s, int id, bool valid,
                                        int lane) {
    float ts = ls[K - 1];
    int ti = li[K - 1];
    unsigned long long m = __ballot(valid && rc_better(s, id, ts, ti));
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        const float cs = __shfl(s, src, 64);
        const int ci = __shfl(id, src, 64);
        const int j0 = lane, j1 = lane + 64;
        float e0s = 0.f, e1s = 0.f;
        int e0i = 0, e1i = 0;
        if (j0 < K) { e0s = ls[j0]; e0i = li[j0]; }
        if (j1 < K) { e1s = ls[j1]; e1i = li[j1]; }
        const bool b0 = j0 < K && rc_better(e0s, e0i, cs, ci);
        const bool b1 = j1 < K && rc_better(e1s, e1i, cs, ci);
        const int pos = __popcll(__ballot(b0)) + __popcll(__ballot(b1));  // entries ahead of the candidate
        if (j0 < K && !b0 && j0 + 1 < K) { ls[j0 + 1] = e0s; li[j0 + 1] = e0i; }
        if (j1 < K && !b1 && j1 + 1 < K) { ls[j1 + 1] = e1s; li[j1 + 1] = e1i; }
        if (lane == 0) { ls[pos] = cs; li[pos] = ci; }
        ts = ls[K - 1];
        ti = li[K - 1];
        m &= m - 1;
        m &= __ballot(valid && rc_better(s, id, ts, ti));
    }
}

__device__ __forceinline__ void rc_list_init(volatile float* ls, volatile int* li, int K, int lane) {
    for (int j = lane; j < K; j += 64) {
        ls[j] = -INFINITY;
        li[j] = RC_IDMAX;
    }
}

// One wave per query: the nsplit sorted partial lists into the final K (empty slots:
// id -1, score -inf).  Dynamic LDS: RC_WAVES * 2 * K * 4 bytes.  A template so that the
// translation units that launch it share one definition.
template <int NW = RC_WAVES>
__global__ __launch_bounds__(NW * 64) void rc_merge_kernel(const float* __restrict__ part_s,
                                                           const int32_t* __restrict__ part_i, int64_t nq, int nsplit,
                                                           int K, int32_t* __restrict__ items_out,
                                                           float* __restrict__ scores_out) {
    extern __shared__ f4 rc_smem4[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* const lsf = reinterpret_cast<float*>(rc_smem4) + wave * 2 * K;
    int* const lif = reinterpret_cast<int*>(lsf + K);
    const int64_t q = (int64_t)blockIdx.x * NW + wave;
    if (q >= nq) return;
    volatile float* ls = lsf;
    volatile int* li = lif;
    rc_list_init(ls, li, K, lane);
    for (int s = 0; s < nsplit; ++s) {
        const int64_t o = (q * nsplit + s) * K;
        for (int j0 = 0; j0 < K; j0 += 16) {
            const int j = j0 + lane;
            float sc = 0.f;
            int id = RC_IDMAX;
            if (lane < 16 && j < K) { sc = part_s[o + j]; id = part_i[o + j]; }
            rc_feed(ls, li, K, sc, id, id != RC_IDMAX, lane);
        }
    }
    for (int j = lane; j < K; j += 64) {
        const int id = li[j];
        items_out[q * K + j] = id == RC_IDMAX ? -1 : id;
        scores_out[q * K + j] = ls[j];
    }
}

// rc_merge_kernel over nq queries on stream st (launch only: the caller checks launch_status).
// A template for the reason rc_merge_kernel is one.
template <int NW = RC_WAVES>
void launch_merge(const float* part_s, const int32_t* part_i, int64_t nq, int nsplit, int K, int32_t* ids_out,
                  float* scores_out, hipStream_t st) {
    hipLaunchKernelGGL(rc_merge_kernel<NW>, dim3((unsigned)((nq + NW - 1) / NW)), dim3(NW * 64),
                       (size_t)NW * 2 * K * 4, st, part_s, part_i, nq, nsplit, K, ids_out, scores_out);
}

}  // namespace ncf

// Distillation response term of one row (src/distillation/base.py:27-34 with T > 0,
// response.py:28-32 with T <= 0): *r = its per-row loss, returns d r / d z.
__device__ __forceinline__ float kd_response(float z, float t, float T, float* r) {
    if (T > 0.f) {
        const float ss = sigmoidf_(z / T), st = sigmoidf_(t / T);
        const float d = ss - st;
        *r = d * d * (T * T);
        return 2.f * T * d * (ss * (1.f - ss));
    }
    const float d = z - t;
    *r = d * d;
    return 2.f * d;
}
