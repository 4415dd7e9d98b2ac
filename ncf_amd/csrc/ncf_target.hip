// Exact full-catalogue ranks of given target items (ncf_target_ranks, include/ncf_hip.h; added
// within ABI 21): for each of n_lists (user, target list) queries and each target t of the list,
//   rank(u, t) = #{ j : j != t, j not in seen(u), z(u, j) > z(u, t) or (z(u, j) == z(u, t) and j < t) }
// -- the 0-based position t takes in ncf_recommend's order among the user's eligible items -- and
// the target's own logit.  The lists are ragged: list q = targets[tgt_ptr[q] .. tgt_ptr[q + 1]).
// The host never reads tgt_ptr.  The third reduction over the serving kernels' pair score, after
// top-K and argmax: a count.
//
// Fused path (NCF_FUSED_SHAPES, dm <= 64), three launches.
//
// Prologue: ncf_recommend's (rc_proj_kernel): Pi over the catalogue, Pu and Ag over the call's
// rows when n_lists < user_num, else over the user table.
//
// Units.  A list is cut into blocks of at most tb targets, tb a power of two in [16, 128] chosen
// by the host from the mean list length (tg_block_shift).  Block j of list q is unit
// q + (tgt_ptr[q] >> log2 tb) + j: strictly ascending in (q, j), below n_lists + (n_tgt >> log2 tb),
// and found back from the unit number by one binary search in tgt_ptr, so no scan kernel and no
// host read is needed.  Unit numbers that no block takes are empty.
//
// Pre-pass (tg_prep_kernel, one workgroup per unit): finds the unit's list, scores its targets 16
// per MFMA tile as rk_kernel scores candidates (tile_h0, tile_tower, tile_gmf_dot, tile_logit: the
// bits ncf_recommend and ncf_rank_candidates give that pair), writes the scores out, zeroes the
// targets' entries of ranks_out, and rank-sorts the block in LDS by (score descending, id
// ascending): the sorted keys and the permutation back to input order go to the workspace.
//
// Sweep (tg_sweep_kernel): rc_kernel with the list taken out.  A workgroup of four waves owns a
// tile of 4 or 16 units and a range of 64-item chunks (rc_geometry over the units); Pi / Ig rows
// are staged once per chunk and shared by the tile.  A wave holds its units' sorted keys in LDS.
// For every scored, unmasked item: a unit of at most TG_SMALL targets compares each target and
// adds the ballot's population count to a wave-uniform counter; a longer unit searches the
// item's key in the sorted keys (log2 tb + 1 compares) and bumps one LDS histogram bucket -- the
// item beats exactly the targets from that position on -- and a prefix sum over the buckets at
// the end turns them into counts.  The counts of the item splits meet in ranks_out by global
// integer atomics through the permutation: integer sums, so the result does not depend on the
// split, the tile, tb or the order of arrival.
//
// Materialised path (every other accepted shape, and every shape under
// ncf_debug_set_target_path(NCF_PATH_LAYERED)): list chunks of at most RC_MAT_PAIRS (user, item)
// pairs -- a rows kernel (the chunk's users x every item), ncf_forward -- then one wave per list
// counts from its logits row with the same mask and order; the target's score is its entry of
// the row.  A second implementation for coverage, not for speed.
#include <string.h>

#include "ncf_host.h"
#include "ncf_tower_tile.h"

namespace ncf {

static int g_tg_path = 0;  // ncf_debug_set_target_path

constexpr int TG_TB = 128;     // most targets of a unit
constexpr int TG_TB_MIN = 16;  // fewest a unit is sized for
constexpr int TG_SMALL = 4;    // units up to this many targets count by ballot, longer ones by search

struct TgArgs {
    ncf_layout lay;
    const float* params;
    const int32_t* users;
    const int64_t* tgt_ptr;
    const int32_t* targets;
    int64_t nq, n_tgt, nunits;
    int sh;      // log2 tb
    int by_row;  // Pu / Ag rows: 1 = the call's row q, 0 = the user id
    const int64_t* seen_ptr;
    const int32_t* seen_items;
    const float* Pi;  // [I][KP0]
    const float* Pu;  // [R][KP0]
    const float* Ag;  // [R][FP]
    float* key_s;     // [n_tgt]: every unit's targets, sorted
    int32_t* key_i;
    int32_t* perm;       // [n_tgt]: sorted position -> position in the unit
    int64_t* unit_q;     // [nunits]
    int64_t* unit_base;  // [nunits]: the unit's first flat target
    int32_t* unit_nb;    // [nunits]: its targets, 0 = empty unit
    int32_t* ranks_out;
    float* scores;  // scores_out, or the workspace's array
    int nsplit, cps, upw;
};

// Targets of a sorted unit that are not behind (z, item): the item beats exactly the targets
// from this position on.  ks / ki: nb keys, score descending then id ascending.
__device__ __forceinline__ int tg_position(const volatile float* ks, const volatile int* ki, int nb, float z,
                                           int item) {
    int lo = 0, hi = nb;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rc_better(z, item, ks[mid], ki[mid])) hi = mid; else lo = mid + 1;
    }
    return lo;
}

template <int F, int L, int MODE>
__global__ __launch_bounds__(RC_WAVES * 64) void tg_prep_kernel(TgArgs a) {
    using C = RcShape<F, L, MODE>;
    constexpr int LDSF = C::W_TOTAL + C::B_TOTAL + C::WP;
    __shared__ f4 smem4[(LDSF > 0 ? LDSF : 4) / 4];
    __shared__ float ks[TG_TB];
    __shared__ int ki[TG_TB];
    static_assert(LDSF % 4 == 0 && (LDSF + 2 * TG_TB) * 4 <= 64 * 1024, "tg_prep_kernel LDS");
    float* const Wl = reinterpret_cast<float*>(smem4);
    float* const Bl = Wl + C::W_TOTAL;
    float* const WPl = Bl + C::B_TOTAL;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, it = lane & 15;
    const float* __restrict__ prm = a.params;
    const int64_t s = blockIdx.x;
    const int tb = 1 << a.sh;

    // the unit's list: the last q with q + (tgt_ptr[q] >> sh) <= s (workgroup-uniform)
    int64_t lo = 0, hi = a.nq;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (mid + (a.tgt_ptr[mid] >> a.sh) <= s) lo = mid + 1; else hi = mid;
    }
    const int64_t q = lo - 1;
    int64_t base = 0;
    int nb = 0;
    if (q >= 0) {
        const int64_t b = a.tgt_ptr[q];
        int64_t e = a.tgt_ptr[q + 1];
        if (e > a.n_tgt) e = a.n_tgt;  // nothing outside [0, n_tgt), whatever tgt_ptr holds
        base = b + (s - (q + (b >> a.sh))) * tb;
        if (b >= 0 && base < e) nb = (int)(e - base < tb ? e - base : tb);
    }
    if (tid == 0) {
        a.unit_q[s] = q;
        a.unit_base[s] = base;
        a.unit_nb[s] = nb;
    }
    if (nb == 0) return;  // workgroup-uniform, before any barrier

    tile_stage<C, RC_WAVES * 64>(a.lay, prm, Wl, Bl, WPl, tid);
    const float bp = prm[a.lay.bp];
    __syncthreads();  // the staged weights

    const int64_t urow = a.by_row ? q : (int64_t)a.users[q];
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
    for (int t = wave; 16 * t < nb; t += RC_WAVES) {
        const int k = 16 * t + it;
        const bool valid = k < nb;
        const int cid = valid ? a.targets[base + k] : 0;
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
        if (lane < 16 && valid) {
            ks[k] = z;
            ki[k] = cid;
        }
    }
    __syncthreads();  // the unit's keys

    // rank sort: equal keys (one id twice) keep their input order
    for (int k = tid; k < nb; k += RC_WAVES * 64) {
        const float z = ks[k];
        const int id = ki[k];
        int pos = 0;
        for (int m = 0; m < nb; ++m) {
            const float zm = ks[m];
            const int im = ki[m];
            pos += rc_better(zm, im, z, id) || (zm == z && im == id && m < k);
        }
        a.key_s[base + pos] = z;
        a.key_i[base + pos] = id;
        a.perm[base + pos] = k;
        a.scores[base + k] = z;
        a.ranks_out[base + k] = 0;  // the sweep adds into it
    }
}

template <int F, int L, int MODE>
__global__ __launch_bounds__(RC_WAVES * 64) void tg_sweep_kernel(TgArgs a) {
    using C = RcShape<F, L, MODE>;
    extern __shared__ f4 rc_smem4[];
    float* const smem = reinterpret_cast<float*>(rc_smem4);
    float* const Wl = smem;
    float* const Bl = Wl + C::W_TOTAL;
    float* const WPl = Bl + C::B_TOTAL;
    float* const PiL = WPl + C::WP;
    float* const IgL = PiL + RC_CH * C::SP;
    const int tb = 1 << a.sh, UT = RC_WAVES * a.upw;
    float* const keys_s = IgL + RC_CH * C::SG;                            // [UT][tb]
    int* const keys_i = reinterpret_cast<int*>(keys_s + UT * tb);         // [UT][tb]
    int* const hist = keys_i + UT * tb;                                   // [UT][tb]
    int* const scr = hist + UT * tb;                                      // [RC_WAVES][64]
    int64_t* const cur = reinterpret_cast<int64_t*>(scr + RC_WAVES * 64); // [UT] (8-byte aligned: see tg_lds_bytes)
    int64_t* const rowL = cur + UT;                                       // [UT]: the unit's row of Pu / Ag
    int* const nbL = reinterpret_cast<int*>(rowL + UT);                   // [UT]: its targets, 0 = nothing to do
    int* const userL = nbL + UT;                                          // [UT]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, it = lane & 15;
    const float* __restrict__ prm = a.params;
    const int I = a.lay.item_num;
    const int nchunks = (I + RC_CH - 1) / RC_CH;
    const int split = blockIdx.y;
    const int cb = split * a.cps, ce = min(cb + a.cps, nchunks);
    const int64_t s0 = (int64_t)blockIdx.x * UT;

    tile_stage<C, RC_WAVES * 64>(a.lay, prm, Wl, Bl, WPl, tid);
    const float bp = prm[a.lay.bp];

    for (int uu = 0; uu < a.upw; ++uu) {  // a wave's own units: no other wave touches their LDS
        const int slot = wave * a.upw + uu;
        const int64_t s = s0 + slot;
        const int nb = s < a.nunits ? a.unit_nb[s] : 0;
        if (nb > 0) {
            const int64_t base = a.unit_base[s];
            for (int k = lane; k < nb; k += 64) {
                keys_s[slot * tb + k] = a.key_s[base + k];
                keys_i[slot * tb + k] = a.key_i[base + k];
            }
        }
        for (int k = lane; k < tb; k += 64) hist[slot * tb + k] = 0;
        if (lane == 0) {
            nbL[slot] = nb;
            if (nb > 0) {
                const int64_t q = a.unit_q[s];
                const int u = a.users[q];
                userL[slot] = u;
                rowL[slot] = a.by_row ? q : (int64_t)u;
                if (a.seen_ptr != nullptr)
                    cur[slot] = rc_lower_bound(a.seen_items, a.seen_ptr[u], a.seen_ptr[u + 1], cb * RC_CH);
            }
        }
    }

    for (int ch = cb; ch < ce; ++ch) {
        const int c0 = ch * RC_CH;
        __syncthreads();  // the previous chunk is consumed (first pass: weights and units are written)
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
            const int nb = nbL[slot];
            if (nb == 0) continue;  // wave-uniform
            const int64_t row = rowL[slot];
            unsigned long long seen = 0;
            if (a.seen_ptr != nullptr) {
                int64_t c = cur[slot];
                seen = rc_seen_mask(a.seen_items, &c, a.seen_ptr[userL[slot] + 1], c0, scr + wave * 64, lane);
                if (lane == 0) cur[slot] = c;
            }
            f4 pu[C::MLP ? C::T(0) : 1], ag[C::GMF ? C::TG : 1];
            if constexpr (C::MLP) {
#pragma unroll
                for (int t = 0; t < C::T(0); ++t)
                    pu[t] = reinterpret_cast<const f4*>(a.Pu)[row * (C::KP0 / 4) + 4 * t + g];
            }
            if constexpr (C::GMF) {
#pragma unroll
                for (int t = 0; t < C::TG; ++t)
                    ag[t] = reinterpret_cast<const f4*>(a.Ag)[row * (C::FP / 4) + 4 * t + g];
            }
            volatile float* ks = keys_s + slot * tb;
            volatile int* ki = keys_i + slot * tb;
            volatile int* hs = hist + slot * tb;
            const bool small = nb <= TG_SMALL;
            float tz[TG_SMALL];
            int ti[TG_SMALL], cnt[TG_SMALL];
#pragma unroll
            for (int k = 0; k < TG_SMALL; ++k) {
                cnt[k] = 0;
                tz[k] = small && k < nb ? ks[k] : 0.f;
                ti[k] = small && k < nb ? ki[k] : 0;
            }
#pragma unroll 1
            for (int tt = 0; tt < RC_CH / 16; ++tt) {
                if (c0 + 16 * tt >= I) break;
                const int r = 16 * tt + it;
                float part = 0.f;
                if constexpr (C::MLP) {
                    f4 h0[C::T(0)];
#pragma unroll
                    for (int t = 0; t < C::T(0); ++t)
                        h0[t] = tile_h0(pu[t], *reinterpret_cast<const f4*>(PiL + r * C::SP + 16 * t + 4 * g));
                    part = tile_tower<C>(h0, Wl, Bl, WPl, it, g);
                }
                if constexpr (C::GMF) part += rc_dot(ag, IgL + r * C::SG, g);
                const float z = tile_logit(part, bp);
                const int item = c0 + r;
                const bool valid = lane < 16 && item < I && !((seen >> r) & 1ull);
                if (small) {
#pragma unroll
                    for (int k = 0; k < TG_SMALL; ++k)
                        if (k < nb) cnt[k] += __popcll(__ballot(valid && rc_better(z, item, tz[k], ti[k])));
                } else if (valid) {
                    const int p = tg_position(ks, ki, nb, z, item);
                    if (p < nb) atomicAdd(hist + slot * tb + p, 1);
                }
            }
            if (small && lane == 0) {
#pragma unroll
                for (int k = 0; k < TG_SMALL; ++k)
                    if (k < nb) hs[k] += cnt[k];
            }
        }
    }

    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // this wave's LDS adds are done
    for (int uu = 0; uu < a.upw; ++uu) {
        const int slot = wave * a.upw + uu;
        const int nb = nbL[slot];
        if (nb == 0) continue;
        const int64_t base = a.unit_base[s0 + slot];
        volatile int* hs = hist + slot * tb;
        for (int k = lane; k < nb; k += 64) {
            int c = hs[k];
            if (nb > TG_SMALL)  // buckets -> counts: every bucket up to the target's own position
                for (int p = 0; p < k; ++p) c += hs[p];
            const int at = a.perm[base + k];  // in [0, nb) for finite scores; a NaN can leave it unwritten
            if (c && (unsigned)at < (unsigned)nb) atomicAdd(a.ranks_out + base + at, c);
        }
    }
}

// Materialised path: packed rows of the users of lists [qb, qb + uc) x every item.
__global__ __launch_bounds__(256) void tg_rows_kernel(const int32_t* __restrict__ users, int64_t qb, int64_t uc, int I,
                                                      uint64_t* __restrict__ rows) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= uc * I) return;
    const int64_t qq = p / I;
    rows[p] = NCF_ROW_PACK(users[qb + qq], (int)(p - qq * I), 0);
}

// Materialised path: one wave per list counts from its row of logits[uc][I].
__global__ __launch_bounds__(RC_WAVES * 64) void tg_count_kernel(const float* __restrict__ logits,
                                                                 const int32_t* __restrict__ users,
                                                                 const int64_t* __restrict__ tgt_ptr,
                                                                 const int32_t* __restrict__ targets, int64_t qb,
                                                                 int64_t uc, int I, int64_t n_tgt,
                                                                 const int64_t* __restrict__ seen_ptr,
                                                                 const int32_t* __restrict__ seen_items,
                                                                 int32_t* __restrict__ ranks_out,
                                                                 float* __restrict__ scores_out) {
    __shared__ int scr_all[RC_WAVES][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t qq = (int64_t)blockIdx.x * RC_WAVES + wave;
    if (qq >= uc) return;  // wave-uniform; no workgroup barrier below
    const int64_t q = qb + qq;
    const float* __restrict__ row = logits + qq * I;
    int* const scr = scr_all[wave];
    int64_t sb = 0, se = 0;
    if (seen_ptr != nullptr) {
        const int u = users[q];
        sb = seen_ptr[u];
        se = seen_ptr[u + 1];
    }
    const int64_t b = tgt_ptr[q];
    int64_t e = tgt_ptr[q + 1];
    if (e > n_tgt) e = n_tgt;
    for (int64_t k = b < 0 ? e : b; k < e; ++k) {
        const int t = targets[k];
        const float zt = row[t];
        int64_t cur = sb;
        int cnt = 0;
        for (int c0 = 0; c0 < I; c0 += RC_CH) {
            unsigned long long seen = 0;
            if (seen_ptr != nullptr) seen = rc_seen_mask(seen_items, &cur, se, c0, scr, lane);
            const int item = c0 + lane;
            const bool valid = item < I && !((seen >> lane) & 1ull);
            const float z = valid ? row[item] : 0.f;
            cnt += __popcll(__ballot(valid && rc_better(z, item, zt, t)));
        }
        if (lane == 0) {
            ranks_out[k] = cnt;
            if (scores_out != nullptr) scores_out[k] = zt;
        }
    }
}

template <int F, int L, int MODE>
struct TgPrepKernel {
    static constexpr auto kernel = &tg_prep_kernel<F, L, MODE>;
};
template <int F, int L, int MODE>
struct TgSweepKernel {
    static constexpr auto kernel = &tg_sweep_kernel<F, L, MODE>;
};
static const TileEntry* tg_fused(const ncf_layout* lay) { return tile_fused<TgSweepKernel>(lay, g_tg_path); }

// log2 of the unit size: the power of two in [TG_TB_MIN, TG_TB] that covers the mean list length,
// from the call's two counts alone.  One-target lists keep the sweep's LDS small; long lists
// sweep the catalogue once per TG_TB targets.
static int tg_block_shift(int64_t nq, int64_t n_tgt) {
    const int64_t mean = (n_tgt + nq - 1) / nq;
    int sh = 4;
    static_assert(TG_TB_MIN == 1 << 4 && TG_TB == 1 << 7, "tg_block_shift");
    while ((1 << sh) < mean && (1 << sh) < TG_TB) ++sh;
    return sh;
}
static int64_t tg_units(int64_t nq, int64_t n_tgt, int sh) { return nq + (n_tgt >> sh); }

static int64_t tg_lds_bytes(const TileEntry* e, const RcGeo& G, int sh) {
    const int UT = RC_WAVES * G.upw;
    // fixed, 3 UT tb and the 256 scratch ints are even counts of 4-byte words: cur is 8-byte aligned
    return ((int64_t)e->fixed + 3 * (UT << sh) + RC_WAVES * 64) * 4 + (int64_t)UT * (8 + 8 + 4 + 4);
}

// Workspace of the fused path: the projections, the target scores (for a call without
// scores_out), the sorted keys and the permutation [n_tgt], the unit table [nunits].
struct TgFusedWs {
    ProjWs p;
    int64_t scores, ks, ki, perm, uq, ub, unb, total;
};
static TgFusedWs tg_fused_ws(const TileEntry* e, const ncf_layout* lay, int64_t nq, int64_t n_tgt) {
    TgFusedWs w;
    const int64_t nunits = tg_units(nq, n_tgt, tg_block_shift(nq, n_tgt));
    w.p = proj_ws(lay, serve_user_rows(lay, nq).R, e->kp0, e->fp);
    w.scores = w.p.total;
    w.ks = w.scores + ws_align(n_tgt * 4);
    w.ki = w.ks + ws_align(n_tgt * 4);
    w.perm = w.ki + ws_align(n_tgt * 4);
    w.uq = w.perm + ws_align(n_tgt * 4);
    w.ub = w.uq + ws_align(nunits * 8);
    w.unb = w.ub + ws_align(nunits * 8);
    w.total = w.unb + ws_align(nunits * 4);
    return w;
}

static int64_t tg_mat_lists(const ncf_layout* lay, int64_t nq) {
    int64_t uc = RC_MAT_PAIRS / lay->item_num;
    if (uc < 1) uc = 1;
    return uc < nq ? uc : nq;
}

}  // namespace ncf

using namespace ncf;

extern "C" {

int ncf_debug_set_target_path(int path) { return set_debug_path(&g_tg_path, path); }

int64_t ncf_target_ranks_workspace_bytes(const ncf_layout* lay, int64_t n_lists, int64_t n_tgt) {
    if (!lay || n_lists < 0 || n_tgt < 0 || lay->item_num <= 0 || lay->user_num <= 0) return -1;
    if (!ncf_supported(lay->model_type, lay->factor_num, lay->num_layers)) return -1;
    if (n_lists == 0) return 0;
    if (const TileEntry* e = tg_fused(lay)) return tg_fused_ws(e, lay, n_lists, n_tgt).total;
    return mat_ws(lay, tg_mat_lists(lay, n_lists) * lay->item_num).total;
}

int ncf_target_ranks(const ncf_layout* lay, const float* params, const int32_t* users, const int64_t* tgt_ptr,
                     const int32_t* targets, int64_t n_lists, int64_t n_tgt, const int64_t* seen_ptr,
                     const int32_t* seen_items, int32_t* ranks_out, float* scores_out, void* workspace,
                     int64_t workspace_bytes, void* stream) {
    if (!lay || n_lists < 0 || n_tgt < 0) return NCF_E_ARG;
    if (n_lists == 0) return NCF_OK;
    if (!params || !users || !tgt_ptr || (!targets && n_tgt > 0) || (!ranks_out && n_tgt > 0) || !workspace)
        return NCF_E_ARG;
    if ((seen_ptr == nullptr) != (seen_items == nullptr)) return NCF_E_ARG;
    if (!ncf_supported(lay->model_type, lay->factor_num, lay->num_layers)) return NCF_E_UNSUPPORTED;
    const int64_t need = ncf_target_ranks_workspace_bytes(lay, n_lists, n_tgt);
    if (need < 0 || workspace_bytes < need) return NCF_E_ARG;
    if (n_tgt == 0) return NCF_OK;  // only empty lists
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    const int I = lay->item_num;

    if (const TileEntry* e = tg_fused(lay)) {
        const TileEntry* prep = tile_fused<TgPrepKernel>(lay, g_tg_path);
        const UserRows ur = serve_user_rows(lay, n_lists);
        const TgFusedWs W = tg_fused_ws(e, lay, n_lists, n_tgt);
        TgArgs a;
        memset(&a, 0, sizeof(a));
        a.sh = tg_block_shift(n_lists, n_tgt);
        a.nunits = tg_units(n_lists, n_tgt, a.sh);
        const RcGeo G = rc_geometry(a.nunits, I);
        const int64_t lds = tg_lds_bytes(e, G, a.sh);
        if (lds > LDS_LIMIT_BYTES) return NCF_E_UNSUPPORTED;
        if (ensure_lds(e->fn, lds) != NCF_OK) return NCF_E_LAUNCH;
        a.lay = *lay;
        a.params = params;
        a.users = users;
        a.tgt_ptr = tgt_ptr;
        a.targets = targets;
        a.nq = n_lists;
        a.n_tgt = n_tgt;
        a.by_row = ur.by_row;
        a.seen_ptr = seen_ptr;
        a.seen_items = seen_items;
        a.key_s = reinterpret_cast<float*>(ws + W.ks);
        a.key_i = reinterpret_cast<int32_t*>(ws + W.ki);
        a.perm = reinterpret_cast<int32_t*>(ws + W.perm);
        a.unit_q = reinterpret_cast<int64_t*>(ws + W.uq);
        a.unit_base = reinterpret_cast<int64_t*>(ws + W.ub);
        a.unit_nb = reinterpret_cast<int32_t*>(ws + W.unb);
        a.ranks_out = ranks_out;
        a.scores = scores_out != nullptr ? scores_out : reinterpret_cast<float*>(ws + W.scores);
        a.nsplit = G.nsplit;
        a.cps = G.cps;
        a.upw = G.upw;
        launch_proj(lay, params, ur.by_row ? users : nullptr, ur.R, e, ws, st, &a.Pi, &a.Pu, &a.Ag);
        void* args[] = {&a};
        if (hipLaunchKernel(prep->fn, dim3((unsigned)a.nunits), dim3(RC_WAVES * 64), args, 0, st) != hipSuccess)
            return NCF_E_LAUNCH;
        if (hipLaunchKernel(e->fn, dim3((unsigned)G.tiles, (unsigned)G.nsplit), dim3(RC_WAVES * 64), args, (size_t)lds,
                            st) != hipSuccess)
            return NCF_E_LAUNCH;
        return launch_status();
    }

    const int64_t ucmax = tg_mat_lists(lay, n_lists);
    const MatWs W = mat_ws(lay, ucmax * I);
    const int rc = mat_run(
        lay, params, W, ws, nullptr, n_lists, ucmax, stream,
        [&](int64_t qb, int64_t uc, uint64_t* rows) {
            const int64_t pairs = uc * I;
            hipLaunchKernelGGL(tg_rows_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, users, qb, uc,
                               I, rows);
            return pairs;
        },
        [&](int64_t qb, int64_t uc, const float* logits) {
            hipLaunchKernelGGL(tg_count_kernel, dim3((unsigned)((uc + RC_WAVES - 1) / RC_WAVES)), dim3(RC_WAVES * 64),
                               0, st, logits, users, tgt_ptr, targets, qb, uc, I, n_tgt, seen_ptr, seen_items,
                               ranks_out, scores_out);
        });
    return rc != NCF_OK ? rc : launch_status();
}

}  // extern "C"
