// Dynamic negative sampling for pairwise (BPR) training (ncf_select_negatives,
// include/ncf_hip.h; added within ABI 21): for each of n positives with m sampled
// candidates, score the n x m (user, candidate) pairs with the current parameters and keep
// the hardest one -- the argmax of the eval-mode logit, equal scores to the lowest slot --
// without materialising rows or logits.
//
// Fused path (NCF_FUSED_SHAPES, dm <= 64).  The prologue is ncf_recommend's (rc_proj_kernel,
// ncf_tower_tile.h): Pi = Im W0[:, dm:]^T + b0 over the catalogue, Pu = Um W0[:, :dm]^T
// and Ag = wp * Ug over the n rows' users, or over the whole user table when
// n >= user_num (row q = user id q then).  The main kernel runs
// workgroups of RC_WAVES waves with the tower weights, biases and predict weights staged in
// LDS in the layout rc_layer reads.  A 16-column tile (ncf_tower_tile.h) holds 16 pairs:
// lane (g, it) gathers its columns of Pu[user of it's group], Pi[cand], Ag and the
// embed_item_GMF row from global memory (L2-resident tables, as ncf_fold.hip gathers),
// then tile_h0, tile_tower, tile_gmf_dot and tile_logit: the functions rc_kernel scores a
// pair with (its GMF dot reads the row from LDS, the same chain), so a pair's score has the
// bits ncf_recommend gives it.
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

#include "ncf_host.h"
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

template <int F, int L, int MODE>
__global__ __launch_bounds__(RC_WAVES * 64) void sel_kernel(SelArgs a) {
    using C = RcShape<F, L, MODE>;
    constexpr int LDSF = C::W_TOTAL + C::B_TOTAL + C::WP;
    __shared__ f4 smem4[(LDSF > 0 ? LDSF : 4) / 4];
    static_assert(LDSF % 4 == 0 && LDSF * 4 <= 64 * 1024, "sel_kernel LDS");
    float* const Wl = reinterpret_cast<float*>(smem4);
    float* const Bl = Wl + C::W_TOTAL;
    float* const WPl = Bl + C::B_TOTAL;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, it = lane & 15;
    const float* __restrict__ prm = a.params;

    tile_stage<C, RC_WAVES * 64>(a.lay, prm, Wl, Bl, WPl, tid);
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
                f4 h0[C::T(0)];
#pragma unroll
                for (int t = 0; t < C::T(0); ++t)
                    h0[t] = tile_h0(*reinterpret_cast<const f4*>(a.Pu + urow * C::KP0 + 16 * t + 4 * g),
                                    *reinterpret_cast<const f4*>(a.Pi + (int64_t)cid * C::KP0 + 16 * t + 4 * g));
                part = tile_tower<C>(h0, Wl, Bl, WPl, it, g);
            }
            if constexpr (C::GMF) {
                f4 ag[C::TG], ig[C::TG];
#pragma unroll
                for (int t = 0; t < C::TG; ++t)
                    ag[t] = *reinterpret_cast<const f4*>(a.Ag + urow * C::FP + 16 * t + 4 * g);
                part += tile_gmf_dot<C>(ag, ig, prm + a.lay.ig + (int64_t)cid * F, g);
            }
            // the group's best of this tile, in its first lane: suffix maximum over the item lanes
            float bz = tile_logit(part, bp);
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

template <int F, int L, int MODE>
struct SelKernel {
    static constexpr auto kernel = &sel_kernel<F, L, MODE>;
};
static const TileEntry* sel_fused(const ncf_layout* lay) { return tile_fused<SelKernel>(lay, g_sel_path); }

static int64_t sel_mat_groups(int64_t n, int m) {
    const int64_t gc = RC_MAT_PAIRS / m;  // m <= 64: at least 2,048 groups
    return gc < n ? gc : n;
}

}  // namespace ncf

using namespace ncf;

extern "C" {

int ncf_debug_set_select_path(int path) { return set_debug_path(&g_sel_path, path); }

int64_t ncf_select_negatives_workspace_bytes(const ncf_layout* lay, int64_t n, int m) {
    if (!lay || n < 0 || m < 1 || m > SEL_MAXM || lay->item_num <= 0 || lay->user_num <= 0) return -1;
    if (!ncf_supported(lay->model_type, lay->factor_num, lay->num_layers)) return -1;
    if (n == 0) return 0;
    const TileEntry* e = sel_fused(lay);
    if (e) return proj_ws(lay, serve_user_rows(lay, n).R, e->kp0, e->fp).total;
    return mat_ws(lay, sel_mat_groups(n, m) * m).total;
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

    if (const TileEntry* e = sel_fused(lay)) {
        const UserRows ur = serve_user_rows(lay, n);
        SelArgs a;
        memset(&a, 0, sizeof(a));
        a.lay = *lay;
        a.params = params;
        a.users = users;
        a.cand = cand;
        a.n = n;
        a.m = m;
        a.by_row = ur.by_row;
        a.neg_out = neg_out;
        a.slot_out = slot_out;
        a.score_out = score_out;
        launch_proj(lay, params, ur.by_row ? users : nullptr, ur.R, e, ws, st, &a.Pi, &a.Pu, &a.Ag);
        const int64_t units = m <= 16 ? (n + 16 / m - 1) / (16 / m) : n;
        int64_t wgs = (units + RC_WAVES - 1) / RC_WAVES;
        if (wgs > SEL_MAX_WG) wgs = SEL_MAX_WG;
        void* args[] = {&a};
        if (hipLaunchKernel(e->fn, dim3((unsigned)wgs), dim3(RC_WAVES * 64), args, 0, st) != hipSuccess)
            return NCF_E_LAUNCH;
        return launch_status();
    }

    const int64_t gcmax = sel_mat_groups(n, m);
    const MatWs W = mat_ws(lay, gcmax * m);
    const int rc = mat_run(
        lay, params, W, ws, nullptr, n, gcmax, stream,
        [&](int64_t pb, int64_t gc, uint64_t* rows) {
            const int64_t pairs = gc * m;
            hipLaunchKernelGGL(sel_rows_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, users, cand,
                               pb, gc, m, rows);
            return pairs;
        },
        [&](int64_t pb, int64_t gc, const float* logits) {
            hipLaunchKernelGGL(sel_pick_kernel, dim3((unsigned)((gc + 255) / 256)), dim3(256), 0, st, logits, cand, pb,
                               gc, m, neg_out, slot_out, score_out);
        });
    return rc != NCF_OK ? rc : launch_status();
}

}  // extern "C"
