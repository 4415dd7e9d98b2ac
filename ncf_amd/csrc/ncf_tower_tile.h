// The in-register MFMA tower tile shared by the serving entry points -- ncf_recommend.hip
// (full-catalogue top-K), ncf_select.hip (hardest negatives), ncf_rank.hip (candidate
// ranking), ncf_target.hip (target ranks) and ncf_fold.hip (fold-in of unseen users): the
// list of fused shapes and the table built from it, the padded shape
// constants, the layer-0 projection prologue (its kernel, its place in a workspace and its
// launch: rc_proj_kernel, proj_ws, launch_proj), the staging of the tower into LDS, and the
// pair score (h0, the layer ladder, the predict and GMF dots, the logit).  ncf_train.hip
// builds kernel_table from the same shape list.
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

// Every shape with a fused kernel (ncf_supported == NCF_PATH_FUSED), as X(F, L, MODE): the
// one list behind kernel_table / kernel_table_bpr (ncf_train.hip) and the three serving
// tables (tile_fused below).
#define NCF_FUSED_TOWER(X, F, L) X(F, L, NCF_MODEL_MLP) X(F, L, NCF_MODEL_NEUMF)
#define NCF_FUSED_SHAPES(X)                                                                                       \
    X(8, 1, NCF_MODEL_GMF) X(16, 1, NCF_MODEL_GMF) X(32, 1, NCF_MODEL_GMF) X(64, 1, NCF_MODEL_GMF)                \
    NCF_FUSED_TOWER(X, 8, 1) NCF_FUSED_TOWER(X, 8, 2) NCF_FUSED_TOWER(X, 8, 3) NCF_FUSED_TOWER(X, 8, 4)           \
    NCF_FUSED_TOWER(X, 16, 1) NCF_FUSED_TOWER(X, 16, 2) NCF_FUSED_TOWER(X, 16, 3) NCF_FUSED_TOWER(X, 32, 1)       \
    NCF_FUSED_TOWER(X, 32, 2) NCF_FUSED_TOWER(X, 64, 1)

namespace ncf {

constexpr int RC_CH = 64;  // items per LDS chunk of ncf_recommend (one seen-mask bit per lane)
// materialised paths (ncf_recommend, ncf_select_negatives, ncf_rank_candidates): (user, item) pairs per chunk
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

// ---------------------------------------------------------------------------
// The layer-0 projection prologue: pre0(u, i) = Pu[u] + Pi[i].  One element each, the fmaf
// chain of rc_proj_chain and, for Pi, b0 added after it; columns from DM on are zero padding.
__device__ __forceinline__ float tile_pi(const ncf_layout& lay, const float* prm, int64_t item, int c, int DM) {
    if (c >= DM) return 0.f;
    float acc = rc_proj_chain(prm + lay.im + item * DM, prm + lay.w[0] + (int64_t)c * 2 * DM + DM, DM);
    acc += prm[lay.b[0] + c];
    return acc;
}
__device__ __forceinline__ float tile_pu(const ncf_layout& lay, const float* prm, int64_t user, int c, int DM) {
    return c < DM ? rc_proj_chain(prm + lay.um + user * DM, prm + lay.w[0] + (int64_t)c * 2 * DM, DM) : 0.f;
}
// Ag = wp[:F] * Ug[u]: the GMF user side pre-scaled by the predict weights
__device__ __forceinline__ float tile_ag(const ncf_layout& lay, const float* prm, int64_t user, int f) {
    return f < lay.factor_num ? prm[lay.wp + f] * prm[lay.ug + user * lay.factor_num + f] : 0.f;
}

// Pi [item_num][KP0] over the catalogue, Pu [nr][KP0] and Ag [nr][FP] over the user rows:
// users[0 .. nr), or the user table (row = user id) with users == NULL.  A template so that
// the translation units that launch it share one definition.
template <int NT = 256>
__global__ __launch_bounds__(NT) void rc_proj_kernel(ncf_layout lay, const float* __restrict__ prm,
                                                     const int32_t* __restrict__ users, int64_t nr, int KP0, int FP,
                                                     float* __restrict__ Pi, float* __restrict__ Pu,
                                                     float* __restrict__ Ag) {
    const int DM = lay.factor_num << (lay.num_layers - 1);
    const int64_t n_pi = (int64_t)lay.item_num * KP0, n_pu = nr * KP0, n_ag = nr * FP;
    int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx < n_pi) {
        const int64_t row = idx / KP0;
        Pi[idx] = tile_pi(lay, prm, row, (int)(idx - row * KP0), DM);
        return;
    }
    idx -= n_pi;
    const bool mlp = idx < n_pu;
    if (!mlp) idx -= n_pu;
    if (!mlp && idx >= n_ag) return;
    const int64_t row = idx / (mlp ? KP0 : FP);
    const int c = (int)(idx - row * (mlp ? KP0 : FP));
    const int64_t u = users != nullptr ? (int64_t)users[row] : row;
    if (mlp) Pu[idx] = tile_pu(lay, prm, u, c, DM);
    else Ag[idx] = tile_ag(lay, prm, u, c);
}

// Where the projections lie in a workspace: Pi [item_num][kp0], Pu [user_rows][kp0] and
// Ag [user_rows][fp]; total = the first byte after them.
struct ProjWs {
    int64_t pi, pu, ag, total;
};
inline ProjWs proj_ws(const ncf_layout* lay, int64_t user_rows, int kp0, int fp) {
    ProjWs w;
    w.pi = 0;
    w.pu = ws_align((int64_t)lay->item_num * kp0 * 4);
    w.ag = w.pu + ws_align(user_rows * kp0 * 4);
    w.total = w.ag + ws_align(user_rows * fp * 4);
    return w;
}

// ---------------------------------------------------------------------------
// Tower weights W_1 .. W_NL zero padded in the layout rc_layer reads, the biases and the
// predict weights of the tower output into LDS, by the NT threads of a workgroup.  No
// barrier: the caller's first one covers it.
template <class C, int NT>
__device__ __forceinline__ void tile_stage(const ncf_layout& lay, const float* prm, float* Wl, float* Bl, float* WPl,
                                           int tid) {
    if constexpr (C::MLP) {
#pragma unroll
        for (int k = 1; k <= C::NL; ++k) {
            const int rows = C::KP(k), cols = C::KP(k - 1), sw = C::SW(k);
            const int out = C::DM >> k, in = C::DM >> (k - 1);
            const float* w = prm + lay.w[k];
            for (int idx = tid; idx < rows * cols; idx += NT) {
                const int r = idx / cols, c = idx - r * cols;
                Wl[C::woff(k) + r * sw + c] = (r < out && c < in) ? w[r * in + c] : 0.f;
            }
            for (int idx = tid; idx < rows; idx += NT) Bl[C::boff(k) + idx] = idx < out ? prm[lay.b[k] + idx] : 0.f;
        }
        for (int idx = tid; idx < C::WP; idx += NT) WPl[idx] = idx < C::F ? prm[lay.wp + C::POFF + idx] : 0.f;
    }
}

// h0 = relu(Pu + Pi), four columns
__device__ __forceinline__ f4 tile_h0(const f4 pu, const f4 pi) {
    f4 h;
    h.x = fmaxf(pu.x + pi.x, 0.f);
    h.y = fmaxf(pu.y + pi.y, 0.f);
    h.z = fmaxf(pu.z + pi.z, 0.f);
    h.w = fmaxf(pu.w + pi.w, 0.f);
    return h;
}

// Layers 1 .. NL on h0 and the predict dot of the tower output: this lane's partial of the logit.
template <class C>
__device__ __forceinline__ float tile_tower(const f4 (&h0)[C::T(0)], const float* Wl, const float* Bl,
                                            const float* WPl, int it, int g) {
    if constexpr (C::NL == 0) {
        return rc_dot(h0, WPl, g);
    } else {
        f4 h1[C::T(1)];
        rc_layer(h0, h1, Wl + C::woff(1), Bl + C::boff(1), it, g);
        if constexpr (C::NL == 1) {
            return rc_dot(h1, WPl, g);
        } else {
            f4 h2[C::T(2)];
            rc_layer(h1, h2, Wl + C::woff(2), Bl + C::boff(2), it, g);
            if constexpr (C::NL == 2) {
                return rc_dot(h2, WPl, g);
            } else {
                f4 h3[C::T(3)];
                rc_layer(h2, h3, Wl + C::woff(3), Bl + C::boff(3), it, g);
                return rc_dot(h3, WPl, g);
            }
        }
    }
}

// rc_dot(ag, item row) with the embed_item_GMF row read from global memory into ig (zero
// from column F on; F % 8 == 0 on the fused path: whole float4s).
template <class C>
__device__ __forceinline__ float tile_gmf_dot(const f4 (&ag)[C::TG], f4 (&ig)[C::TG], const float* row, int g) {
    float sg = 0.f;
#pragma unroll
    for (int t = 0; t < C::TG; ++t) {
        ig[t] = f4{0.f, 0.f, 0.f, 0.f};
        if (16 * t + 4 * g < C::F) ig[t] = *reinterpret_cast<const f4*>(row + 16 * t + 4 * g);
        sg = fmaf(ag[t].x, ig[t].x, sg);
        sg = fmaf(ag[t].y, ig[t].y, sg);
        sg = fmaf(ag[t].z, ig[t].z, sg);
        sg = fmaf(ag[t].w, ig[t].w, sg);
    }
    return sg;
}

// The four column groups' partials summed across the wave, + bp: the same bits in the four
// lanes of an item.
__device__ __forceinline__ float tile_logit(float part, float bp) {
    part += shfl_xor(part, 16);
    part += shfl_xor(part, 32);
    return part + bp;
}

// ---------------------------------------------------------------------------
// The catalogue sweep of ncf_recommend and ncf_target_ranks: the seen mask of a 64-item chunk
// and the launch shape.
// First position p in [lo, hi) with seen_items[p] >= item (wave-uniform).
__device__ __forceinline__ int64_t rc_lower_bound(const int32_t* __restrict__ seen_items, int64_t lo, int64_t hi,
                                                  int item) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (seen_items[mid] < item) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Seen mask of the 64 items [c0, c0 + 64) of a user whose cursor *cur points at the first
// list entry >= c0: bit j = item c0 + j is in the list.  The list is ascending and unique,
// so at most 64 entries fall in the chunk and one load per lane covers them; every access
// is bounded by hi = seen_ptr[u + 1].  scr: 64 ints of per-wave LDS.
__device__ __forceinline__ unsigned long long rc_seen_mask(const int32_t* __restrict__ seen_items, int64_t* cur,
                                                           int64_t hi, int c0, volatile int* scr, int lane) {
    const int64_t p = *cur + lane;
    const int v = p < hi ? seen_items[p] : RC_IDMAX;
    const bool below = p < hi && v < c0 + RC_CH;
    scr[lane] = 0;
    if (below && v >= c0) scr[v - c0] = 1;
    const unsigned long long mask = __ballot(scr[lane] != 0);
    *cur += __popcll(__ballot(below));
    return mask;
}

// Launch shape of the fused kernel from the query size and the catalogue: 16-user tiles
// from 256 queried users up (4-user tiles below), and as many item splits as bring the
// grid to about four workgroups per compute unit.
struct RcGeo {
    int upw, nsplit, cps;
    int64_t tiles;
};
inline RcGeo rc_geometry(int64_t nq, int I) {
    RcGeo G;
    G.upw = nq >= 256 ? 4 : 1;
    const int UT = RC_WAVES * G.upw;
    G.tiles = (nq + UT - 1) / UT;
    const int64_t nchunks = ((int64_t)I + RC_CH - 1) / RC_CH;
    int64_t want = (1024 + G.tiles - 1) / G.tiles;
    if (want > nchunks) want = nchunks;
    if (want > 1024) want = 1024;
    if (want < 1) want = 1;
    G.cps = (int)((nchunks + want - 1) / want);
    G.nsplit = (int)((nchunks + G.cps - 1) / G.cps);
    return G;
}

// ---------------------------------------------------------------------------
// One table per serving kernel template, over NCF_FUSED_SHAPES.  K<F, L, MODE>::kernel is
// the kernel's address (function templates cannot be template arguments themselves).
struct TileEntry {
    int mode, F, L;
    const void* fn;
    int fixed, kp0, fp;  // ncf_recommend's LDS floats before the lists; padded Pi / Pu and Ag widths
};

// The fused kernel of a serving entry point for this layout, or null: its debug switch
// (ncf_debug_set_*_path), then ncf_supported, then the table.
template <template <int, int, int> class K>
const TileEntry* tile_fused(const ncf_layout* lay, int debug_path) {
#define NCF_TILE_ENTRY(F, L, MODE)                                                                          \
    TileEntry{MODE, F, L, reinterpret_cast<const void*>(K<F, L, MODE>::kernel), RcShape<F, L, MODE>::FIXED, \
              RcShape<F, L, MODE>::KP0, RcShape<F, L, MODE>::FP},
    static const TileEntry table[] = {NCF_FUSED_SHAPES(NCF_TILE_ENTRY)};
#undef NCF_TILE_ENTRY
    if (debug_path == NCF_PATH_LAYERED) return nullptr;
    if (ncf_supported(lay->model_type, lay->factor_num, lay->num_layers) != NCF_PATH_FUSED) return nullptr;
    const int Lk = lay->model_type == NCF_MODEL_GMF ? 1 : lay->num_layers;
    for (const TileEntry& e : table)
        if (e.mode == lay->model_type && e.F == lay->factor_num && e.L == Lk) return &e;
    return nullptr;
}

// rc_proj_kernel into the head of workspace ws (proj_ws) over R user rows: users[0 .. R), or
// the user table with users == NULL; *Pi, *Pu, *Ag = where they lie.  Launch only: the caller
// checks launch_status.  A template for the reason rc_proj_kernel is one.
template <int NT = 256>
void launch_proj(const ncf_layout* lay, const float* params, const int32_t* users, int64_t R, const TileEntry* e,
                 char* ws, hipStream_t st, const float** Pi, const float** Pu, const float** Ag) {
    const ProjWs W = proj_ws(lay, R, e->kp0, e->fp);
    float *pi = reinterpret_cast<float*>(ws + W.pi), *pu = reinterpret_cast<float*>(ws + W.pu),
          *ag = reinterpret_cast<float*>(ws + W.ag);
    const int64_t nproj = ((int64_t)lay->item_num + R) * e->kp0 + R * e->fp;
    hipLaunchKernelGGL(rc_proj_kernel<NT>, dim3((unsigned)((nproj + NT - 1) / NT)), dim3(NT), 0, st, *lay, params,
                       users, R, e->kp0, e->fp, pi, pu, ag);
    *Pi = pi, *Pu = pu, *Ag = ag;
}

}  // namespace ncf
