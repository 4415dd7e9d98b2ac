// Candidate ranking (ncf_rank_candidates, include/ncf_hip.h; added within ABI 21): for each
// of n_lists (user, candidate list) queries, the top_k candidates of that list under the
// eval-mode logit, score descending then slot (position in the list) ascending.  The lists
// are ragged: list q = cand[cand_ptr[q] .. cand_ptr[q + 1]).  The host never reads cand_ptr.
//
// Fused path (NCF_FUSED_SHAPES, dm <= 64).  The prologue is ncf_recommend's (rc_proj_kernel,
// ncf_tower_tile.h), used as ncf_select_negatives uses it: Pi over the catalogue, Pu and Ag
// over the call's rows when n_lists < user_num, else over the user table.  The main kernel
// runs workgroups of RC_WAVES waves with the tower staged in LDS (tile_stage).  A workgroup
// takes one list at a time (lists blockIdx.x, blockIdx.x + gridDim.x, ...).  A 16-lane tile
// holds 16 consecutive candidates of the list: lane (g, it) gathers its columns of Pu, of
// Pi[cand], of Ag and of the embed_item_GMF row as sel_kernel does, then tile_h0, tile_tower,
// tile_gmf_dot and tile_logit -- the pair score of ncf_recommend and ncf_select_negatives,
// bit for bit.  Every wave keeps a running top-K list in LDS (rc_list_init / rc_feed,
// ncf_common.h) whose id key is the slot; RC_IDMAX marks an empty entry.
//
// Split of a list's tiles.  With nsplit = gridDim.y, tile t goes to walker t mod
// (nsplit RC_WAVES): wave w of split s is walker s RC_WAVES + w.  nsplit comes from n_lists
// alone (rk_splits): 1 from 1,024 lists up, more below so that a few long lists still fill
// the machine.  After the walk wave 0 feeds the other waves' lists into its own.  With one
// split it writes the outputs; otherwise it writes a partial list [n_lists][nsplit][K],
// rc_merge_kernel orders the partials into (slot, score) and rk_items_kernel looks the item
// ids up.  The order is total on (score, slot) and every score is one fixed arithmetic
// sequence, so a list's result is a function of that list alone.
//
// Materialised path (every other accepted shape, and every shape under
// ncf_debug_set_rank_path(NCF_PATH_LAYERED)): the flat candidate array in chunks of at most
// RC_MAT_PAIRS pairs -- a rows kernel that finds each pair's list by a search in cand_ptr,
// ncf_forward into an n_cand-float logit array -- then one wave per list with the same
// rc_feed list over its logits.  A second implementation for coverage, not for speed.
#include <string.h>

#include "ncf_host.h"
#include "ncf_tower_tile.h"

namespace ncf {

static int g_rk_path = 0;  // ncf_debug_set_rank_path

constexpr int RK_MAX_WG = 4096;     // workgroups along grid.x; beyond, a workgroup walks several lists
constexpr int RK_FILL_LISTS = 1024; // lists from which one split per list fills the machine
constexpr int RK_MAX_SPLIT = 64;

struct RkArgs {
    ncf_layout lay;
    const float* params;
    const int32_t* users;
    const int64_t* cand_ptr;
    const int32_t* cand;
    int64_t nq;
    int K;
    int by_row;       // Pu / Ag rows: 1 = the call's row q, 0 = the user id
    const float* Pi;  // [I][KP0]
    const float* Pu;  // [R][KP0]
    const float* Ag;  // [R][FP]
    float* part_s;    // [nq][nsplit][K] (nsplit > 1)
    int32_t* part_i;
    int32_t* items_out;
    int32_t* slots_out;
    float* scores_out;
};

template <int F, int L, int MODE>
__global__ __launch_bounds__(RC_WAVES * 64) void rk_kernel(RkArgs a) {
    using C = RcShape<F, L, MODE>;
    constexpr int LDSF = C::W_TOTAL + C::B_TOTAL + C::WP;
    __shared__ f4 smem4[(LDSF > 0 ? LDSF : 4) / 4];
    __shared__ float lists_s[RC_WAVES][RC_MAXK];
    __shared__ int lists_i[RC_WAVES][RC_MAXK];
    static_assert(LDSF % 4 == 0 && (LDSF + 2 * RC_WAVES * RC_MAXK) * 4 <= 64 * 1024, "rk_kernel LDS");
    float* const Wl = reinterpret_cast<float*>(smem4);
    float* const Bl = Wl + C::W_TOTAL;
    float* const WPl = Bl + C::B_TOTAL;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, it = lane & 15;
    const float* __restrict__ prm = a.params;
    const int K = a.K;
    const int nsplit = gridDim.y, split = blockIdx.y;
    const int walker = split * RC_WAVES + wave, nwalk = nsplit * RC_WAVES;
    volatile float* ls = lists_s[wave];
    volatile int* li = lists_i[wave];

    tile_stage<C, RC_WAVES * 64>(a.lay, prm, Wl, Bl, WPl, tid);
    const float bp = prm[a.lay.bp];
    __syncthreads();  // the staged weights

#pragma unroll 1
    for (int64_t q = blockIdx.x; q < a.nq; q += gridDim.x) {  // workgroup-uniform
        const int64_t b = a.cand_ptr[q];
        const int64_t len = a.cand_ptr[q + 1] - b;
        const int64_t tiles = (len + 15) >> 4;
        const int64_t urow = a.by_row ? q : (int64_t)a.users[q];
        rc_list_init(ls, li, K, lane);  // this wave's own list: wave 0 is done with it (barrier below)

        f4 pu[C::MLP ? C::T(0) : 1], ag[C::GMF ? C::TG : 1];
        if constexpr (C::MLP) {
#pragma unroll
            for (int t = 0; t < C::T(0); ++t) pu[t] = *reinterpret_cast<const f4*>(a.Pu + urow * C::KP0 + 16 * t + 4 * g);
        }
        if constexpr (C::GMF) {
#pragma unroll
            for (int t = 0; t < C::TG; ++t) ag[t] = *reinterpret_cast<const f4*>(a.Ag + urow * C::FP + 16 * t + 4 * g);
        }
#pragma unroll 1
        for (int64_t t = walker; t < tiles; t += nwalk) {
            const int64_t slot = 16 * t + it;
            const bool valid = slot < len;
            const int cid = valid ? a.cand[b + slot] : 0;
            float part = 0.f;
            if constexpr (C::MLP) {
                f4 h0[C::T(0)];
#pragma unroll
                for (int tt = 0; tt < C::T(0); ++tt)
                    h0[tt] = tile_h0(pu[tt], *reinterpret_cast<const f4*>(a.Pi + (int64_t)cid * C::KP0 + 16 * tt + 4 * g));
                part = tile_tower<C>(h0, Wl, Bl, WPl, it, g);
            }
            if constexpr (C::GMF) {
                f4 ig[C::TG];
                part += tile_gmf_dot<C>(ag, ig, prm + a.lay.ig + (int64_t)cid * F, g);
            }
            const float z = tile_logit(part, bp);
            rc_feed(ls, li, K, z, (int)slot, lane < 16 && valid, lane);
        }
        __syncthreads();  // the four lists are complete

        if (wave == 0) {
            for (int w = 1; w < RC_WAVES; ++w) {
                if (split * RC_WAVES + w >= tiles) break;  // that wave and the later ones had no tile
                for (int j0 = 0; j0 < K; j0 += 16) {
                    const int j = j0 + lane;
                    float sc = 0.f;
                    int id = RC_IDMAX;
                    if (lane < 16 && j < K) { sc = lists_s[w][j]; id = lists_i[w][j]; }
                    rc_feed(ls, li, K, sc, id, id != RC_IDMAX, lane);
                }
            }
            if (nsplit == 1) {
                for (int j = lane; j < K; j += 64) {
                    const int id = li[j];
                    const bool empty = id == RC_IDMAX;
                    a.items_out[q * K + j] = empty ? -1 : a.cand[b + id];
                    if (a.slots_out != nullptr) a.slots_out[q * K + j] = empty ? -1 : id;
                    a.scores_out[q * K + j] = ls[j];
                }
            } else {
                const int64_t o = (q * nsplit + split) * K;
                for (int j = lane; j < K; j += 64) {
                    a.part_s[o + j] = ls[j];
                    a.part_i[o + j] = li[j];
                }
            }
        }
        __syncthreads();  // wave 0 is done with the other waves' lists
    }
}

// After rc_merge_kernel (nsplit > 1): slots [nq][K] (-1 = empty) -> item ids.
__global__ __launch_bounds__(256) void rk_items_kernel(const int64_t* __restrict__ cand_ptr,
                                                       const int32_t* __restrict__ cand,
                                                       const int32_t* __restrict__ slots, int64_t nq, int K,
                                                       int32_t* __restrict__ items_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nq * K) return;
    const int s = slots[e];
    items_out[e] = s < 0 ? -1 : cand[cand_ptr[e / K] + s];
}

// Materialised path: packed rows of the flat pairs [pb, pb + pc).  Pair k belongs to the
// list q with cand_ptr[q] <= k < cand_ptr[q + 1] (empty lists own no pair).
__global__ __launch_bounds__(256) void rk_rows_kernel(const int32_t* __restrict__ users,
                                                      const int64_t* __restrict__ cand_ptr,
                                                      const int32_t* __restrict__ cand, int64_t nq, int64_t pb,
                                                      int64_t pc, uint64_t* __restrict__ rows) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= pc) return;
    const int64_t k = pb + r;
    int64_t lo = 0, hi = nq;  // the first q in [0, nq] with cand_ptr[q] > k; cand_ptr[nq] = n_cand > k
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cand_ptr[mid] <= k) lo = mid + 1; else hi = mid;
    }
    rows[r] = NCF_ROW_PACK(users[lo - 1], cand[k], 0);
}

// Materialised path: one wave per list selects from its logits.
__global__ __launch_bounds__(RC_WAVES * 64) void rk_select_kernel(const float* __restrict__ logits,
                                                                  const int64_t* __restrict__ cand_ptr,
                                                                  const int32_t* __restrict__ cand, int64_t nq, int K,
                                                                  int32_t* __restrict__ items_out,
                                                                  int32_t* __restrict__ slots_out,
                                                                  float* __restrict__ scores_out) {
    __shared__ float lists_s[RC_WAVES][RC_MAXK];
    __shared__ int lists_i[RC_WAVES][RC_MAXK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t q = (int64_t)blockIdx.x * RC_WAVES + wave;
    if (q >= nq) return;  // wave-uniform; no workgroup barrier below
    volatile float* ls = lists_s[wave];
    volatile int* li = lists_i[wave];
    rc_list_init(ls, li, K, lane);
    const int64_t b = cand_ptr[q];
    const int64_t len = cand_ptr[q + 1] - b;
    for (int64_t s0 = 0; s0 < len; s0 += 16) {
        const int64_t slot = s0 + (lane & 15);
        const bool valid = lane < 16 && slot < len;
        const float z = valid ? logits[b + slot] : 0.f;
        rc_feed(ls, li, K, z, (int)slot, valid, lane);
    }
    for (int j = lane; j < K; j += 64) {
        const int id = li[j];
        const bool empty = id == RC_IDMAX;
        items_out[q * K + j] = empty ? -1 : cand[b + id];
        if (slots_out != nullptr) slots_out[q * K + j] = empty ? -1 : id;
        scores_out[q * K + j] = ls[j];
    }
}

template <int F, int L, int MODE>
struct RankKernel {
    static constexpr auto kernel = &rk_kernel<F, L, MODE>;
};
static const TileEntry* rk_fused(const ncf_layout* lay) { return tile_fused<RankKernel>(lay, g_rk_path); }

// Splits of every list's tiles over grid.y, from the number of lists alone.
static int rk_splits(int64_t nq) {
    if (nq >= RK_FILL_LISTS) return 1;
    const int64_t want = (RK_FILL_LISTS + nq - 1) / nq;
    return (int)(want > RK_MAX_SPLIT ? RK_MAX_SPLIT : want);
}

// Workspace of the fused path: the projections; with more than one split the partial lists
// [nq][nsplit][K] (scores, slots) and a [nq][K] slot array for a call without slots_out.
struct RkFusedWs {
    ProjWs p;
    int64_t ps, pid, slots, total;
};
static RkFusedWs rk_fused_ws(const TileEntry* e, const ncf_layout* lay, int64_t nq, int K) {
    RkFusedWs w;
    const int nsplit = rk_splits(nq);
    w.p = proj_ws(lay, serve_user_rows(lay, nq).R, e->kp0, e->fp);
    const int64_t part = nsplit > 1 ? ws_align(nq * nsplit * K * 4) : 0;
    w.ps = w.p.total;
    w.pid = w.ps + part;
    w.slots = w.pid + part;
    w.total = w.slots + (nsplit > 1 ? ws_align(nq * K * 4) : 0);
    return w;
}

// Workspace of the materialised path: mat_ws of one chunk, then the n_cand logits.
struct RkMatWs {
    MatWs m;
    int64_t chunk, all, total;
};
static RkMatWs rk_mat_ws(const ncf_layout* lay, int64_t n_cand) {
    RkMatWs w;
    w.chunk = n_cand < RC_MAT_PAIRS ? (n_cand > 0 ? n_cand : 1) : RC_MAT_PAIRS;
    w.m = mat_ws(lay, w.chunk);
    w.all = w.m.total;
    w.total = w.all + ws_align(n_cand * 4);
    return w;
}

}  // namespace ncf

using namespace ncf;

extern "C" {

int ncf_debug_set_rank_path(int path) { return set_debug_path(&g_rk_path, path); }

int64_t ncf_rank_candidates_workspace_bytes(const ncf_layout* lay, int64_t n_lists, int64_t n_cand, int top_k) {
    if (!lay || n_lists < 0 || n_cand < 0 || top_k < 1 || top_k > RC_MAXK || lay->item_num <= 0 ||
        lay->user_num <= 0)
        return -1;
    if (!ncf_supported(lay->model_type, lay->factor_num, lay->num_layers)) return -1;
    if (n_lists == 0) return 0;
    if (const TileEntry* e = rk_fused(lay)) return rk_fused_ws(e, lay, n_lists, top_k).total;
    return rk_mat_ws(lay, n_cand).total;
}

int ncf_rank_candidates(const ncf_layout* lay, const float* params, const int32_t* users, const int64_t* cand_ptr,
                        const int32_t* cand, int64_t n_lists, int64_t n_cand, int top_k, int32_t* items_out,
                        int32_t* slots_out, float* scores_out, void* workspace, int64_t workspace_bytes,
                        void* stream) {
    if (!lay || n_lists < 0 || n_cand < 0 || top_k < 1 || top_k > RC_MAXK) return NCF_E_ARG;
    if (n_lists == 0) return NCF_OK;
    if (!params || !users || !cand_ptr || (!cand && n_cand > 0) || !items_out || !scores_out || !workspace)
        return NCF_E_ARG;
    if (!ncf_supported(lay->model_type, lay->factor_num, lay->num_layers)) return NCF_E_UNSUPPORTED;
    const int64_t need = ncf_rank_candidates_workspace_bytes(lay, n_lists, n_cand, top_k);
    if (need < 0 || workspace_bytes < need) return NCF_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const int K = top_k;

    if (const TileEntry* e = rk_fused(lay)) {
        const UserRows ur = serve_user_rows(lay, n_lists);
        const RkFusedWs W = rk_fused_ws(e, lay, n_lists, K);
        const int nsplit = rk_splits(n_lists);
        RkArgs a;
        memset(&a, 0, sizeof(a));
        a.lay = *lay;
        a.params = params;
        a.users = users;
        a.cand_ptr = cand_ptr;
        a.cand = cand;
        a.nq = n_lists;
        a.K = K;
        a.by_row = ur.by_row;
        a.part_s = reinterpret_cast<float*>(ws + W.ps);
        a.part_i = reinterpret_cast<int32_t*>(ws + W.pid);
        a.items_out = items_out;
        a.slots_out = slots_out;
        a.scores_out = scores_out;
        launch_proj(lay, params, ur.by_row ? users : nullptr, ur.R, e, ws, st, &a.Pi, &a.Pu, &a.Ag);
        const int64_t wgs = n_lists < RK_MAX_WG ? n_lists : RK_MAX_WG;
        void* args[] = {&a};
        if (hipLaunchKernel(e->fn, dim3((unsigned)wgs, (unsigned)nsplit), dim3(RC_WAVES * 64), args, 0, st) !=
            hipSuccess)
            return NCF_E_LAUNCH;
        if (nsplit > 1) {
            // the merged id key is the slot: into slots_out, or the workspace's array without one
            int32_t* slots = slots_out != nullptr ? slots_out : reinterpret_cast<int32_t*>(ws + W.slots);
            launch_merge(a.part_s, a.part_i, n_lists, nsplit, K, slots, scores_out, st);
            hipLaunchKernelGGL(rk_items_kernel, dim3((unsigned)((n_lists * K + 255) / 256)), dim3(256), 0, st,
                               cand_ptr, cand, slots, n_lists, K, items_out);
        }
        return launch_status();
    }

    const RkMatWs W = rk_mat_ws(lay, n_cand);
    float* logits = reinterpret_cast<float*>(ws + W.all);  // all n_cand of them: chunk pb writes logits + pb
    const int rc = mat_run(
        lay, params, W.m, ws, logits, n_cand, W.chunk, stream,
        [&](int64_t pb, int64_t pc, uint64_t* rows) {
            hipLaunchKernelGGL(rk_rows_kernel, dim3((unsigned)((pc + 255) / 256)), dim3(256), 0, st, users, cand_ptr,
                               cand, n_lists, pb, pc, rows);
            return pc;
        },
        [](int64_t, int64_t, const float*) {});  // the lists are selected once every chunk is scored
    if (rc != NCF_OK) return rc;
    hipLaunchKernelGGL(rk_select_kernel, dim3((unsigned)((n_lists + RC_WAVES - 1) / RC_WAVES)), dim3(RC_WAVES * 64), 0,
                       st, logits, cand_ptr, cand, n_lists, K, items_out, slots_out, scores_out);
    return launch_status();
}

}  // extern "C"
