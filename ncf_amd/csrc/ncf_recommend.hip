// Evaluation kernels.  HR / NDCG per batch of scored candidates (ncf_hr_ndcg), and the
// full-catalogue top-K recommendation (ncf_recommend, include/ncf_hip.h; since ABI 20):
//
// Fused path (every shape with a fused kernel: dm <= 64).  Layer 0 factors per entity,
//   pre0(u, i) = Pu[u] + Pi[i],  Pu = Um W0[:, :dm]^T,  Pi = Im W0[:, dm:]^T + b0,
// so a prologue projects the catalogue and the queried users once and the main kernel
// does, per pair, one add + ReLU of width dm, layers 1..L-1 on v_mfma_f32_16x16x4_f32,
// the predict dot and the GMF dot (user side pre-scaled by the predict weights).  No
// per-pair gathers and no U x I array.
//
// The register layout of a 16-item tile, the projection prologue (rc_proj_kernel), the
// staging of the tower and the pair score are in ncf_tower_tile.h, shared with
// ncf_select.hip and ncf_fold.hip.
//
// A workgroup (4 waves) owns a tile of 4 or 16 queried users and a range of 64-item
// chunks; each chunk (Pi rows, Ig rows) is staged once in LDS and shared by the tile's
// users.  Each (wave, user) keeps a sorted top-K list in LDS (score descending, item id
// ascending) with a threshold test against its last entry.  The item range is split
// over workgroups (grid.y); a merge pass orders the partial lists.  The order is total
// on (score, id) and every score is one fixed arithmetic sequence, so the result does
// not depend on tiling, the split or the users per workgroup.  The list insert and the
// merge pass (rc_feed, rc_list_init, rc_merge_kernel) live in ncf_common.h, shared with
// ncf_neighbors.hip.
//
// Materialised path (the other accepted shapes): user chunks of at most RC_MAT_PAIRS
// (user, item) pairs -- rows kernel, ncf_forward, select-from-logits with the same
// mask, order and list.
#include <string.h>

#include "ncf_host.h"
#include "ncf_tower_tile.h"

namespace ncf {

static int g_rc_path = 0;  // ncf_debug_set_recommend_path

struct RcArgs {
    ncf_layout lay;
    const float* params;
    const int32_t* users;
    int64_t nq;
    int K;
    const int64_t* seen_ptr;
    const int32_t* seen_items;
    const float* Pi;  // [I][KP0]
    const float* Pu;  // [nq][KP0]
    const float* Ag;  // [nq][FP]
    float* part_s;    // [nq][nsplit][K]
    int32_t* part_i;
    int nsplit, cps;  // item splits; chunks per split
    int upw;          // users per wave
};

template <int F, int L, int MODE>
__global__ __launch_bounds__(RC_WAVES * 64) void rc_kernel(RcArgs a) {
    using C = RcShape<F, L, MODE>;
    extern __shared__ f4 rc_smem4[];
    float* const smem = reinterpret_cast<float*>(rc_smem4);
    float* const Wl = smem;
    float* const Bl = Wl + C::W_TOTAL;
    float* const WPl = Bl + C::B_TOTAL;
    float* const PiL = WPl + C::WP;
    float* const IgL = PiL + RC_CH * C::SP;
    const int K = a.K, UT = RC_WAVES * a.upw;
    float* const lists_s = IgL + RC_CH * C::SG;
    int* const lists_i = reinterpret_cast<int*>(lists_s + UT * K);
    int* const scr = lists_i + UT * K;                                       // [RC_WAVES][64]
    int64_t* const cur = reinterpret_cast<int64_t*>(scr + RC_WAVES * 64);    // [UT] (8-byte aligned: see rc_lds_bytes)

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, it = lane & 15;
    const float* __restrict__ prm = a.params;
    const int I = a.lay.item_num;
    const int nchunks = (I + RC_CH - 1) / RC_CH;
    const int split = blockIdx.y;
    const int cb = split * a.cps, ce = min(cb + a.cps, nchunks);
    const int64_t q0 = (int64_t)blockIdx.x * UT;

    tile_stage<C, RC_WAVES * 64>(a.lay, prm, Wl, Bl, WPl, tid);
    const float bp = prm[a.lay.bp];

    for (int uu = 0; uu < a.upw; ++uu) {
        const int slot = wave * a.upw + uu;
        rc_list_init(lists_s + slot * K, lists_i + slot * K, K, lane);
        const int64_t q = q0 + slot;
        if (a.seen_ptr != nullptr && q < a.nq && lane == 0) {
            const int u = a.users[q];
            cur[slot] = rc_lower_bound(a.seen_items, a.seen_ptr[u], a.seen_ptr[u + 1], cb * RC_CH);
        }
    }

    for (int ch = cb; ch < ce; ++ch) {
        const int c0 = ch * RC_CH;
        __syncthreads();  // the previous chunk is consumed (first pass: weights and lists are written)
        if constexpr (C::MLP) {
            constexpr int C4 = C::KP0 / 4;
            for (int idx = tid; idx < RC_CH * C4; idx += RC_WAVES * 64) {
                const int r = idx / C4, c4 = idx - r * C4;
                f4 v = {0.f, 0.f, 0.f, 0.f};
                if (c0 + r < I) v = reinterpret_cast<const f4*>(a.Pi)[(int64_t)(c0 + r) * C4 + c4];
                *reinterpret_cast<f4*>(PiL + r * C::SP + 4 * c4) = v;
            }
        }
        if constexpr (C::GMF) {
            for (int idx = tid; idx < RC_CH * C::FP; idx += RC_WAVES * 64) {
                const int r = idx / C::FP, f = idx - r * C::FP;
                IgL[r * C::SG + f] = (c0 + r < I && f < F) ? prm[a.lay.ig + (int64_t)(c0 + r) * F + f] : 0.f;
            }
        }
        __syncthreads();

        for (int uu = 0; uu < a.upw; ++uu) {
            const int slot = wave * a.upw + uu;
            const int64_t q = q0 + slot;
            if (q >= a.nq) break;  // wave-uniform
            unsigned long long seen = 0;
            if (a.seen_ptr != nullptr) {
                const int u = a.users[q];
                int64_t c = cur[slot];
                seen = rc_seen_mask(a.seen_items, &c, a.seen_ptr[u + 1], c0, scr + wave * 64, lane);
                if (lane == 0) cur[slot] = c;
            }
            f4 pu[C::MLP ? C::T(0) : 1], ag[C::GMF ? C::TG : 1];
            if constexpr (C::MLP) {
#pragma unroll
                for (int t = 0; t < C::T(0); ++t)
                    pu[t] = reinterpret_cast<const f4*>(a.Pu)[q * (C::KP0 / 4) + 4 * t + g];
            }
            if constexpr (C::GMF) {
#pragma unroll
                for (int t = 0; t < C::TG; ++t)
                    ag[t] = reinterpret_cast<const f4*>(a.Ag)[q * (C::FP / 4) + 4 * t + g];
            }
            volatile float* ls = lists_s + slot * K;
            volatile int* li = lists_i + slot * K;
#pragma unroll 1
            for (int tt = 0; tt < RC_CH / 16; ++tt) {
                if (c0 + 16 * tt >= I) break;
                const int row = 16 * tt + it;
                float part = 0.f;
                if constexpr (C::MLP) {
                    f4 h0[C::T(0)];
#pragma unroll
                    for (int t = 0; t < C::T(0); ++t)
                        h0[t] = tile_h0(pu[t], *reinterpret_cast<const f4*>(PiL + row * C::SP + 16 * t + 4 * g));
                    part = tile_tower<C>(h0, Wl, Bl, WPl, it, g);
                }
                if constexpr (C::GMF) part += rc_dot(ag, IgL + row * C::SG, g);
                const float z = tile_logit(part, bp);
                const int item = c0 + row;
                const bool valid = lane < 16 && item < I && !((seen >> row) & 1ull);
                rc_feed(ls, li, K, z, item, valid, lane);
            }
        }
    }

    for (int uu = 0; uu < a.upw; ++uu) {
        const int slot = wave * a.upw + uu;
        const int64_t q = q0 + slot;
        if (q >= a.nq) break;
        const int64_t o = (q * a.nsplit + split) * K;
        volatile float* ls = lists_s + slot * K;
        volatile int* li = lists_i + slot * K;
        for (int j = lane; j < K; j += 64) {
            a.part_s[o + j] = ls[j];
            a.part_i[o + j] = li[j];
        }
    }
}

// Materialised path: packed rows of users [qb, qb + uc) x every item.
__global__ __launch_bounds__(256) void rc_rows_kernel(const int32_t* __restrict__ users, int64_t qb, int64_t uc, int I,
                                                      uint64_t* __restrict__ rows) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= uc * I) return;
    const int64_t qq = p / I;
    rows[p] = NCF_ROW_PACK(users[qb + qq], (int)(p - qq * I), 0);
}

// Materialised path: one wave per user selects from logits[uc][I].
__global__ __launch_bounds__(RC_WAVES * 64) void rc_select_kernel(const float* __restrict__ logits,
                                                                  const int32_t* __restrict__ users, int64_t qb,
                                                                  int64_t uc, int I, int K,
                                                                  const int64_t* __restrict__ seen_ptr,
                                                                  const int32_t* __restrict__ seen_items,
                                                                  int32_t* __restrict__ items_out,
                                                                  float* __restrict__ scores_out) {
    extern __shared__ f4 rc_smem4[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* const lsf = reinterpret_cast<float*>(rc_smem4) + wave * (2 * K + 64);
    int* const lif = reinterpret_cast<int*>(lsf + K);
    int* const scr = lif + K;
    const int64_t qq = (int64_t)blockIdx.x * RC_WAVES + wave;
    if (qq >= uc) return;
    const int64_t q = qb + qq;
    volatile float* ls = lsf;
    volatile int* li = lif;
    rc_list_init(ls, li, K, lane);
    int64_t cur = 0, hi = 0;
    if (seen_ptr != nullptr) {
        const int u = users[q];
        cur = seen_ptr[u];
        hi = seen_ptr[u + 1];
    }
    for (int c0 = 0; c0 < I; c0 += RC_CH) {
        unsigned long long seen = 0;
        if (seen_ptr != nullptr) seen = rc_seen_mask(seen_items, &cur, hi, c0, scr, lane);
        for (int tt = 0; tt < RC_CH / 16; ++tt) {
            if (c0 + 16 * tt >= I) break;
            const int row = 16 * tt + (lane & 15);
            const int item = c0 + row;
            const bool valid = lane < 16 && item < I && !((seen >> row) & 1ull);
            const float z = valid ? logits[qq * I + item] : 0.f;
            rc_feed(ls, li, K, z, item, valid, lane);
        }
    }
    for (int j = lane; j < K; j += 64) {
        const int id = li[j];
        items_out[q * K + j] = id == RC_IDMAX ? -1 : id;
        scores_out[q * K + j] = ls[j];
    }
}

template <int F, int L, int MODE>
struct RcKernel {
    static constexpr auto kernel = &rc_kernel<F, L, MODE>;
};
static const TileEntry* rc_fused(const ncf_layout* lay) { return tile_fused<RcKernel>(lay, g_rc_path); }

static int64_t rc_lds_bytes(const TileEntry* e, const RcGeo& G, int K) {
    const int UT = RC_WAVES * G.upw;
    // fixed, 2 UT K and the 256 scratch ints are even counts of 4-byte words: cur is 8-byte aligned
    return ((int64_t)e->fixed + 2 * UT * K + RC_WAVES * 64) * 4 + (int64_t)UT * 8;
}

// Workspace of the fused path: the projections, then the partial lists [nq][nsplit][K]
struct RcFusedWs {
    ProjWs p;
    int64_t ps, pid, total;
};
static RcFusedWs rc_fused_ws(const TileEntry* e, const ncf_layout* lay, int64_t nq, int K, const RcGeo& G) {
    RcFusedWs w;
    w.p = proj_ws(lay, nq, e->kp0, e->fp);
    w.ps = w.p.total;
    w.pid = w.ps + ws_align(nq * G.nsplit * K * 4);
    w.total = w.pid + ws_align(nq * G.nsplit * K * 4);
    return w;
}

static int64_t rc_mat_users(const ncf_layout* lay, int64_t nq) {
    int64_t uc = RC_MAT_PAIRS / lay->item_num;
    if (uc < 1) uc = 1;
    return uc < nq ? uc : nq;
}

// ---------------------------------------------------------------------------
// HR / NDCG per batch.  One wave per batch; the batch's logits staged in LDS.
// rank(e) = #{e' : x[e'] > x[e] or (x[e'] == x[e] and e' < e)}  (stable order)
constexpr int HR_MAXB = 1024;
__global__ __launch_bounds__(256) void hr_ndcg_kernel(const float* __restrict__ logits, const int32_t* __restrict__ items,
                                                      int64_t n, int bs, int k, int64_t nb, int32_t* hr, float* ndcg) {
    __shared__ float sx[4][HR_MAXB];
    __shared__ int si[4][HR_MAXB];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + w;
    if (b >= nb) return;  // wave-uniform; no workgroup barrier below
    const int64_t r0 = b * bs;
    const int cnt = (int)((n - r0) < bs ? (n - r0) : bs);
    for (int e = l; e < cnt; e += 64) {
        sx[w][e] = logits[r0 + e];
        si[w][e] = items[r0 + e];
    }
    __builtin_amdgcn_wave_barrier();  // LDS is in-order per wave: the writes above are seen below
    const int gt = si[w][0];
    int best = 0x7fffffff;
    for (int e = l; e < cnt; e += 64) {
        if (si[w][e] != gt) continue;
        const float x = sx[w][e];
        int rank = 0;
        for (int e2 = 0; e2 < cnt; ++e2) {
            const float y = sx[w][e2];
            rank += (y > x) || (y == x && e2 < e);
        }
        if (rank < k && rank < best) best = rank;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int o = __shfl_xor(best, m, 64);
        best = o < best ? o : best;
    }
    if (l == 0) {
        const bool hit = best < k;
        hr[b] = hit ? 1 : 0;
        ndcg[b] = hit ? (float)(1.0 / log2((double)best + 2.0)) : 0.0f;
    }
}

}  // namespace ncf

using namespace ncf;

extern "C" {

int ncf_debug_set_recommend_path(int path) { return set_debug_path(&g_rc_path, path); }

int64_t ncf_recommend_workspace_bytes(const ncf_layout* lay, int64_t n_users, int top_k) {
    if (!lay || n_users < 0 || top_k < 1 || top_k > RC_MAXK || lay->item_num <= 0) return -1;
    if (!ncf_supported(lay->model_type, lay->factor_num, lay->num_layers)) return -1;
    if (n_users == 0) return 0;
    if (const TileEntry* e = rc_fused(lay))
        return rc_fused_ws(e, lay, n_users, top_k, rc_geometry(n_users, lay->item_num)).total;
    return mat_ws(lay, rc_mat_users(lay, n_users) * lay->item_num).total;
}

int ncf_recommend(const ncf_layout* lay, const float* params, const int32_t* users, int64_t n_users, int top_k,
                  const int64_t* seen_ptr, const int32_t* seen_items, int32_t* items_out, float* scores_out,
                  void* workspace, int64_t workspace_bytes, void* stream) {
    if (!lay || n_users < 0 || top_k < 1 || top_k > RC_MAXK) return NCF_E_ARG;
    if (n_users == 0) return NCF_OK;
    if (!params || !users || !items_out || !scores_out || !workspace) return NCF_E_ARG;
    if ((seen_ptr == nullptr) != (seen_items == nullptr)) return NCF_E_ARG;
    if (!ncf_supported(lay->model_type, lay->factor_num, lay->num_layers)) return NCF_E_UNSUPPORTED;
    if (workspace_bytes < ncf_recommend_workspace_bytes(lay, n_users, top_k)) return NCF_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const int I = lay->item_num, K = top_k;

    if (const TileEntry* e = rc_fused(lay)) {
        const RcGeo G = rc_geometry(n_users, I);
        const RcFusedWs W = rc_fused_ws(e, lay, n_users, K, G);
        const int64_t lds = rc_lds_bytes(e, G, K);
        if (lds > LDS_LIMIT_BYTES) return NCF_E_UNSUPPORTED;
        if (ensure_lds(e->fn, lds) != NCF_OK) return NCF_E_LAUNCH;
        RcArgs a;
        memset(&a, 0, sizeof(a));
        a.lay = *lay;
        a.params = params;
        a.users = users;
        a.nq = n_users;
        a.K = K;
        a.seen_ptr = seen_ptr;
        a.seen_items = seen_items;
        a.part_s = reinterpret_cast<float*>(ws + W.ps);
        a.part_i = reinterpret_cast<int32_t*>(ws + W.pid);
        a.nsplit = G.nsplit;
        a.cps = G.cps;
        a.upw = G.upw;
        launch_proj(lay, params, users, n_users, e, ws, st, &a.Pi, &a.Pu, &a.Ag);
        void* args[] = {&a};
        if (hipLaunchKernel(e->fn, dim3((unsigned)G.tiles, (unsigned)G.nsplit), dim3(RC_WAVES * 64), args, (size_t)lds,
                            st) != hipSuccess)
            return NCF_E_LAUNCH;
        launch_merge(a.part_s, a.part_i, n_users, G.nsplit, K, items_out, scores_out, st);
        return launch_status();
    }

    const int64_t ucmax = rc_mat_users(lay, n_users);
    const MatWs W = mat_ws(lay, ucmax * I);
    const int rc = mat_run(
        lay, params, W, ws, nullptr, n_users, ucmax, stream,
        [&](int64_t qb, int64_t uc, uint64_t* rows) {
            const int64_t pairs = uc * I;
            hipLaunchKernelGGL(rc_rows_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, users, qb, uc,
                               I, rows);
            return pairs;
        },
        [&](int64_t qb, int64_t uc, const float* logits) {
            hipLaunchKernelGGL(rc_select_kernel, dim3((unsigned)((uc + RC_WAVES - 1) / RC_WAVES)),
                               dim3(RC_WAVES * 64), (size_t)RC_WAVES * (2 * K + 64) * 4, st, logits, users, qb, uc, I,
                               K, seen_ptr, seen_items, items_out, scores_out);
        });
    return rc != NCF_OK ? rc : launch_status();
}

int ncf_hr_ndcg(const float* logits, const int32_t* items, int64_t n, int batch, int top_k, int32_t* hr, float* ndcg,
                void* stream) {
    if (!logits || !items || !hr || !ndcg || n <= 0 || batch <= 0 || batch > HR_MAXB || top_k <= 0) return NCF_E_ARG;
    const int64_t nb = (n + batch - 1) / batch;
    const int64_t last = n - (nb - 1) * batch;
    if (top_k > batch || top_k > last) return NCF_E_ARG;  // torch.topk: "selected index k out of range"
    const int64_t grid = (nb + 3) / 4;
    hipLaunchKernelGGL(hr_ndcg_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, logits, items, n, batch,
                       top_k, nb, hr, ndcg);
    return launch_status();
}

}  // extern "C"
