// Dynamic negative sampling for pairwise (BPR) training (ncf_select_negatives,
// include/ncf_hip.h; added within ABI 21): for each of n positives with m sampled
// candidates, score the n x m (user, candidate) pairs with the current parameters and keep
// the hardest one -- the argmax of the eval-mode logit, equal scores to the lowest slot --
// without materialising rows or logits.
//
// Fused path (the shapes of ncf_recommend's fused path, dm <= 64).  The prologue is
// ncf_recommend's (the same expressions, the same bits): Pi = Im W0[:, dm:]^T + b0 over the
// catalogue, Pu = Um W0[:, :dm]^T and Ag = wp * Ug over the n rows' users, or over the
// whole user table when n >= user_num (row q = user id q then).  The main kernel runs
// workgroups of RC_WAVES waves with the tower weights, biases and predict weights staged in
// LDS in the layout rc_layer reads.  A 16-column tile (ncf_tower_tile.h) holds 16 pairs:
// lane (g, it) gathers its columns of Pu[user of it's group], Pi[cand], Ag and the
// embed_item_GMF row from global memory (L2-resident tables, as ncf_fold.hip gathers),
// h0 = relu(Pu + Pi), layers 1.. through rc_layer, rc_dot, the GMF dot, the two
// shfl_xor(16 / 32) sums and + bp: the arithmetic sequence of rc_kernel, so a pair's score
// has the bits ncf_recommend gives it.
//
// Lanes of a tile.  m <= 16: a tile holds G = floor(16 / m) whole groups, group gi in
// lanes it = gi m .. gi m + m - 1 (slot j = it - gi m); the lanes from G m on idle.  A
// wave's work unit is one tile (G groups).  m > 16: a group takes ceil(m / 16) consecutive
// tiles of one wave (slot j = 16 tile + it), the running best carried in registers; the
// unit is one group.  Units are walked grid-stride, so a group never straddles two waves.
//
// Argmax: a segmented suffix maximum over the tile's 16 item lanes on (score, slot, id) --
// at distance d = 1, 2, 4, 8 lane it takes lane it + d's triple when that lane is in the
// same group and its score is strictly greater (the lanes it covers so far all hold lower
// slots, so equal scores keep the lowest slot).  No LDS, no atomics.  The group's first
// lane (g = 0) stores neg_out[p] and, when given, slot_out[p] and score_out[p]; nothing
// else is written.  Every result is a function of its own group alone.
//
// Materialised path (every other accepted shape, and every shape under
// ncf_debug_set_select_path(NCF_PATH_LAYERED)): chunks of whole groups of at most
// RC_MAT_PAIRS pairs -- rows kernel, ncf_forward, a select kernel with the same rule (one
// thread per group).  A second implementation for coverage, not for speed.
#include <string.h>

#include "ncf_common.h"
#include "ncf_tower_tile.h"

namespace ncf {

static int g_sel_path = 0;  // ncf_debug_set_select_path

constexpr int SEL_MAXM = 64;
constexpr int SEL_MAX_WG = 512;  // workgroups of the fused kernel (two per compute unit); beyond, grid-stride

struct SelArgs {
    ncf_layout lay;
    const float* params;
    const int32_t* users;
    const int32_t* cand;
    int64_t n;
    int m;
    int by_row;       // Pu / Ag rows: 1 = the call's row p, 0 = the user id
    const float* Pi;  // [I][KP0]
    const float* Pu;  // [R][KP0]
    const float* Ag;  // [R][FP]
    int32_t* neg_out;
    int32_t* slot_out;
    float* score_out;
};

// Prologue: rc_proj_kernel's Pi, Pu and Ag (ncf_recommend.hip) with the user rows either
// users[0 .. nr) (users != NULL) or the whole table (row = user id).
__global__ __launch_bounds__(256) void sel_proj_kernel(ncf_layout lay, const float* __restrict__ prm,
                                                       const int32_t* __restrict__ users, int64_t nr, int KP0, int FP,
                                                       float* __restrict__ Pi, float* __restrict__ Pu,
                                                       float* __restrict__ Ag) {
    const int DM = lay.factor_num << (lay.num_layers - 1);
    const int F = lay.factor_num;
    const int64_t n_pi = (int64_t)lay.item_num * KP0, n_pu = nr * KP0, n_ag = nr * FP;
    int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n_pi + n_pu) {
        const bool item = idx < n_pi;
        if (!item) idx -= n_pi;
        const int64_t row = idx / KP0;
        const int c = (int)(idx - row * KP0);
        float acc = 0.f;
        if (c < DM) {
            const float* w = prm + lay.w[0] + (int64_t)c * 2 * DM + (item ? DM : 0);
            const int64_t u = item ? row : (users != nullptr ? (int64_t)users[row] : row);
            const float* x = item ? prm + lay.im + row * DM : prm + lay.um + u * DM;
            acc = rc_proj_chain(x, w, DM);
            if (item) acc += prm[lay.b[0] + c];
        }
        (item ? Pi : Pu)[idx] = acc;
        return;
    }
    idx -= n_pi + n_pu;
    if (idx < n_ag) {
        const int64_t q = idx / FP;
        const int f = (int)(idx - q * FP);
        const int64_t u = users != nullptr ? (int64_t)users[q] : q;
        Ag[idx] = f < F ? prm[lay.wp + f] * prm[lay.ug + u * F + f] : 0.f;
    }
}

template <int F, int L, int MODE>
__global__ __launch_bounds__(RC_WAVES * 64) void sel_kernel(SelArgs a) {
    using C = RcShape<F, L, MODE>;
    constexpr int LDSF = C::W_TOTAL + C::B_TOTAL + C::WP;
    __shared__ f4 smem4[(LDSF > 0 ? LDSF : 4) / 4];
    static_assert(LDSF % 4 == 0 && LDSF * 4 <= 64 * 1024, "sel_kernel LDS");
    float* const Wl = reinterpret_cast<float*>(smem4);
    float* const Bl = Wl + C::W_TOTAL;
    float* const WPl = Bl + C::B_TOTAL;
    constexpr int T0 = C::MLP ? C::T(0) : 1, TG = C::GMF ? C::TG : 1;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, it = lane & 15;
    const float* __restrict__ prm = a.params;

    // tower weights (zero padded), biases, predict weights: rc_kernel's staging
    if constexpr (C::MLP) {
#pragma unroll
        for (int k = 1; k <= C::NL; ++k) {
            const int rows = C::KP(k), cols = C::KP(k - 1), sw = C::SW(k);
            const int out = C::DM >> k, in = C::DM >> (k - 1);
            const float* w = prm + a.lay.w[k];
            for (int idx = tid; idx < rows * cols; idx += RC_WAVES * 64) {
                const int r = idx / cols, c = idx - r * cols;
                Wl[C::woff(k) + r * sw + c] = (r < out && c < in) ? w[r * in + c] : 0.f;
            }
            for (int idx = tid; idx < rows; idx += RC_WAVES * 64)
                Bl[C::boff(k) + idx] = idx < out ? prm[a.lay.b[k] + idx] : 0.f;
        }
        for (int idx = tid; idx < C::WP; idx += RC_WAVES * 64)
            WPl[idx] = idx < F ? prm[a.lay.wp + C::POFF + idx] : 0.f;
    }
    const float bp = prm[a.lay.bp];
    __syncthreads();  // the only workgroup barrier: the waves walk their units on their own

    const int m = a.m;
    const bool small = m <= 16;
    const int G = small ? 16 / m : 1;            // groups per tile
    const int tpg = small ? 1 : (m + 15) >> 4;   // tiles per group
    const int gi = small ? it / m : 0;           // this lane's group inside the tile
    const int64_t units = small ? (a.n + G - 1) / G : a.n;

#pragma unroll 1
    for (int64_t unit = (int64_t)blockIdx.x * RC_WAVES + wave; unit < units; unit += (int64_t)gridDim.x * RC_WAVES) {
        const int64_t p = small ? unit * G + gi : unit;
        const bool group_ok = gi < G && p < a.n;
        const int first = gi * m;  // the group's first lane (m <= 16)
        float run_z = 0.f;
        int run_j = 0, run_id = 0;
#pragma unroll 1
        for (int tt = 0; tt < tpg; ++tt) {
            const int j = small ? it - first : 16 * tt + it;
            const bool valid = group_ok && j < m;
            const int end = !valid ? it : (small ? first + m : min(16, m - 16 * tt));  // past the group's last lane
            const int cid = valid ? a.cand[p * m + j] : 0;
            const int64_t urow = valid ? (a.by_row ? p : (int64_t)a.users[p]) : 0;
            float part = 0.f;
            if constexpr (C::MLP) {
                f4 h0[T0];
#pragma unroll
                for (int t = 0; t < T0; ++t) {
                    const f4 pu = *reinterpret_cast<const f4*>(a.Pu + urow * C::KP0 + 16 * t + 4 * g);
                    const f4 pi = *reinterpret_cast<const f4*>(a.Pi + (int64_t)cid * C::KP0 + 16 * t + 4 * g);
                    h0[t].x = fmaxf(pu.x + pi.x, 0.f);
                    h0[t].y = fmaxf(pu.y + pi.y, 0.f);
                    h0[t].z = fmaxf(pu.z + pi.z, 0.f);
                    h0[t].w = fmaxf(pu.w + pi.w, 0.f);
                }
                if constexpr (C::NL == 0) {
                    part = rc_dot(h0, WPl, g);
                } else {
                    f4 h1[C::T(1)];
                    rc_layer(h0, h1, Wl + C::woff(1), Bl + C::boff(1), it, g);
                    if constexpr (C::NL == 1) {
                        part = rc_dot(h1, WPl, g);
                    } else {
                        f4 h2[C::T(2)];
                        rc_layer(h1, h2, Wl + C::woff(2), Bl + C::boff(2), it, g);
                        if constexpr (C::NL == 2) {
                            part = rc_dot(h2, WPl, g);
                        } else {
                            f4 h3[C::T(3)];
                            rc_layer(h2, h3, Wl + C::woff(3), Bl + C::boff(3), it, g);
                            part = rc_dot(h3, WPl, g);
                        }
                    }
                }
            }
            if constexpr (C::GMF) {
                float sg = 0.f;  // rc_dot(ag, item row): the same chain, the row read from global memory
#pragma unroll
                for (int t = 0; t < TG; ++t) {
                    const f4 ag = *reinterpret_cast<const f4*>(a.Ag + urow * C::FP + 16 * t + 4 * g);
                    f4 ig = {0.f, 0.f, 0.f, 0.f};
                    if (16 * t + 4 * g < F)  // F % 8 == 0 on this path: whole float4s
                        ig = *reinterpret_cast<const f4*>(prm + a.lay.ig + (int64_t)cid * F + 16 * t + 4 * g);
                    sg = fmaf(ag.x, ig.x, sg);
                    sg = fmaf(ag.y, ig.y, sg);
                    sg = fmaf(ag.z, ig.z, sg);
                    sg = fmaf(ag.w, ig.w, sg);
                }
                part += sg;
            }
            part += shfl_xor(part, 16);
            part += shfl_xor(part, 32);
            // the group's best of this tile, in its first lane: suffix maximum over the item lanes
            float bz = part + bp;
            int bj = j, bid = cid;
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                const float oz = __shfl_down(bz, d, 64);
                const int oj = __shfl_down(bj, d, 64);
                const int oid = __shfl_down(bid, d, 64);
                if (it + d < end && oz > bz) {
                    bz = oz;
                    bj = oj;
                    bid = oid;
                }
            }
            if (tt == 0 || bz > run_z) {  // later tiles hold higher slots: strictly greater only
                run_z = bz;
                run_j = bj;
                run_id = bid;
            }
        }
        if (group_ok && g == 0 && it == (small ? first : 0)) {
            a.neg_out[p] = run_id;
            if (a.slot_out != nullptr) a.slot_out[p] = run_j;
            if (a.score_out != nullptr) a.score_out[p] = run_z;
        }
    }
}

// Materialised path: packed rows of the pairs of groups [pb, pb + gc).
__global__ __launch_bounds__(256) void sel_rows_kernel(const int32_t* __restrict__ users,
                                                       const int32_t* __restrict__ cand, int64_t pb, int64_t gc, int m,
                                                       uint64_t* __restrict__ rows) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= gc * m) return;
    const int64_t p = pb + k / m;
    rows[k] = NCF_ROW_PACK(users[p], cand[pb * m + k], 0);
}

// Materialised path: one thread per group, first strict maximum of logits[gc][m].
__global__ __launch_bounds__(256) void sel_pick_kernel(const float* __restrict__ logits,
                                                       const int32_t* __restrict__ cand, int64_t pb, int64_t gc, int m,
                                                       int32_t* __restrict__ neg_out, int32_t* __restrict__ slot_out,
                                                       float* __restrict__ score_out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= gc) return;
    float bz = logits[q * m];
    int bj = 0;
    for (int j = 1; j < m; ++j) {
        const float z = logits[q * m + j];
        if (z > bz) {
            bz = z;
            bj = j;
        }
    }
    const int64_t p = pb + q;
    neg_out[p] = cand[p * m + bj];
    if (slot_out != nullptr) slot_out[p] = bj;
    if (score_out != nullptr) score_out[p] = bz;
}

struct SelEntry {
    int mode, F, L;
    const void* fn;
    int kp0, fp;
};

template <int F, int L, int MODE>
static SelEntry sel_make() {
    using C = RcShape<F, L, MODE>;
    return SelEntry{MODE, F, L, reinterpret_cast<const void*>(&sel_kernel<F, L, MODE>), C::KP0, C::FP};
}

// The shapes of ncf_recommend's fused path (rc_entry, ncf_recommend.hip).
static const SelEntry* sel_entry(const ncf_layout* lay) {
    static const SelEntry table[] = {
        sel_make<8, 1, NCF_MODEL_GMF>(),  sel_make<16, 1, NCF_MODEL_GMF>(),
        sel_make<32, 1, NCF_MODEL_GMF>(), sel_make<64, 1, NCF_MODEL_GMF>(),
#define NCF_SEL_TOWER(F, L) sel_make<F, L, NCF_MODEL_MLP>(), sel_make<F, L, NCF_MODEL_NEUMF>()
        NCF_SEL_TOWER(8, 1),  NCF_SEL_TOWER(8, 2),  NCF_SEL_TOWER(8, 3),  NCF_SEL_TOWER(8, 4),  NCF_SEL_TOWER(16, 1),
        NCF_SEL_TOWER(16, 2), NCF_SEL_TOWER(16, 3), NCF_SEL_TOWER(32, 1), NCF_SEL_TOWER(32, 2), NCF_SEL_TOWER(64, 1),
#undef NCF_SEL_TOWER
    };
    const int Lk = lay->model_type == NCF_MODEL_GMF ? 1 : lay->num_layers;
    for (const SelEntry& e : table)
        if (e.mode == lay->model_type && e.F == lay->factor_num && e.L == Lk) return &e;
    return nullptr;
}

static const SelEntry* sel_fused(const ncf_layout* lay) {
    if (g_sel_path == NCF_PATH_LAYERED) return nullptr;
    if (ncf_supported(lay->model_type, lay->factor_num, lay->num_layers) != NCF_PATH_FUSED) return nullptr;
    return sel_entry(lay);
}

static int64_t sel_al(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

// Rows of Pu / Ag: the call's rows when they are fewer than the users, else the user table.
static int64_t sel_user_rows(const ncf_layout* lay, int64_t n) { return n < lay->user_num ? n : lay->user_num; }

struct SelFusedWs {
    int64_t pi, pu, ag, total;
};
static SelFusedWs sel_fused_ws(const SelEntry* e, const ncf_layout* lay, int64_t n) {
    const int64_t R = sel_user_rows(lay, n);
    SelFusedWs w;
    int64_t o = 0;
    w.pi = o; o += sel_al((int64_t)lay->item_num * e->kp0 * 4);
    w.pu = o; o += sel_al(R * e->kp0 * 4);
    w.ag = o; o += sel_al(R * e->fp * 4);
    w.total = o;
    return w;
}

static int64_t sel_mat_groups(int64_t n, int m) {
    const int64_t gc = RC_MAT_PAIRS / m;  // m <= 64: at least 2,048 groups
    return gc < n ? gc : n;
}

struct SelMatWs {
    int64_t rows, logits, fwd, fwd_bytes, total;
};
static SelMatWs sel_mat_ws(const ncf_layout* lay, int64_t n, int m) {
    const int64_t pairs = sel_mat_groups(n, m) * m;
    SelMatWs w;
    int64_t o = 0;
    w.rows = o; o += sel_al(pairs * 8);
    w.logits = o; o += sel_al(pairs * 4);
    w.fwd = o;
    w.fwd_bytes = ncf_forward_workspace_bytes(lay, pairs);
    o += sel_al(w.fwd_bytes);
    w.total = o;
    return w;
}

}  // namespace ncf

using namespace ncf;

extern "C" {

int ncf_debug_set_select_path(int path) {
    if (path != 0 && path != NCF_PATH_LAYERED) return NCF_E_ARG;
    g_sel_path = path;
    return NCF_OK;
}

int64_t ncf_select_negatives_workspace_bytes(const ncf_layout* lay, int64_t n, int m) {
    if (!lay || n < 0 || m < 1 || m > SEL_MAXM || lay->item_num <= 0 || lay->user_num <= 0) return -1;
    if (!ncf_supported(lay->model_type, lay->factor_num, lay->num_layers)) return -1;
    if (n == 0) return 0;
    const SelEntry* e = sel_fused(lay);
    return e ? sel_fused_ws(e, lay, n).total : sel_mat_ws(lay, n, m).total;
}

int ncf_select_negatives(const ncf_layout* lay, const float* params, const int32_t* users, const int32_t* cand,
                         int64_t n, int m, int32_t* neg_out, int32_t* slot_out, float* score_out, void* workspace,
                         int64_t workspace_bytes, void* stream) {
    if (!lay || n < 0 || m < 1 || m > SEL_MAXM) return NCF_E_ARG;
    if (n == 0) return NCF_OK;
    if (!params || !users || !cand || !neg_out || !workspace) return NCF_E_ARG;
    if (!ncf_supported(lay->model_type, lay->factor_num, lay->num_layers)) return NCF_E_UNSUPPORTED;
    const int64_t need = ncf_select_negatives_workspace_bytes(lay, n, m);
    if (need < 0 || workspace_bytes < need) return NCF_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);

    if (const SelEntry* e = sel_fused(lay)) {
        const SelFusedWs W = sel_fused_ws(e, lay, n);
        const int64_t R = sel_user_rows(lay, n);
        SelArgs a;
        memset(&a, 0, sizeof(a));
        a.lay = *lay;
        a.params = params;
        a.users = users;
        a.cand = cand;
        a.n = n;
        a.m = m;
        a.by_row = n < lay->user_num ? 1 : 0;
        a.Pi = reinterpret_cast<float*>(ws + W.pi);
        a.Pu = reinterpret_cast<float*>(ws + W.pu);
        a.Ag = reinterpret_cast<float*>(ws + W.ag);
        a.neg_out = neg_out;
        a.slot_out = slot_out;
        a.score_out = score_out;
        const int64_t nproj = ((int64_t)lay->item_num + R) * e->kp0 + R * e->fp;
        hipLaunchKernelGGL(sel_proj_kernel, dim3((unsigned)((nproj + 255) / 256)), dim3(256), 0, st, *lay, params,
                           a.by_row ? users : nullptr, R, e->kp0, e->fp, const_cast<float*>(a.Pi),
                           const_cast<float*>(a.Pu), const_cast<float*>(a.Ag));
        const int64_t units = m <= 16 ? (n + 16 / m - 1) / (16 / m) : n;
        int64_t wgs = (units + RC_WAVES - 1) / RC_WAVES;
        if (wgs > SEL_MAX_WG) wgs = SEL_MAX_WG;
        void* args[] = {&a};
        if (hipLaunchKernel(e->fn, dim3((unsigned)wgs), dim3(RC_WAVES * 64), args, 0, st) != hipSuccess)
            return NCF_E_LAUNCH;
        return hipGetLastError() == hipSuccess ? NCF_OK : NCF_E_LAUNCH;
    }

    const SelMatWs W = sel_mat_ws(lay, n, m);
    const int64_t gcmax = sel_mat_groups(n, m);
    uint64_t* rows = reinterpret_cast<uint64_t*>(ws + W.rows);
    float* logits = reinterpret_cast<float*>(ws + W.logits);
    for (int64_t pb = 0; pb < n; pb += gcmax) {
        const int64_t gc = n - pb < gcmax ? n - pb : gcmax;
        const int64_t pairs = gc * m;
        hipLaunchKernelGGL(sel_rows_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, users, cand, pb, gc,
                           m, rows);
        const int rc = ncf_forward(lay, params, rows, pairs, logits, W.fwd_bytes ? ws + W.fwd : nullptr, W.fwd_bytes,
                                   stream);
        if (rc != NCF_OK) return rc;
        hipLaunchKernelGGL(sel_pick_kernel, dim3((unsigned)((gc + 255) / 256)), dim3(256), 0, st, logits, cand, pb, gc,
                           m, neg_out, slot_out, score_out);
    }
    return hipGetLastError() == hipSuccess ? NCF_OK : NCF_E_LAUNCH;
}

}  // extern "C"
