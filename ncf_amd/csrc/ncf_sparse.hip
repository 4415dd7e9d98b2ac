// The row-wise optimizers and exchanges over the embedding tables, which share the table
// geometry of LazyArgs: the deferred (lazy) Adam with the touched-row lists and their packed
// form (dp_mode "touched"), and the owner-sharded exchange (dp_mode "owner") -- with their
// C ABI (include/ncf_hip.h).  gfx950 only.
#include <stdlib.h>
#include <string.h>

#include "ncf_host.h"

namespace ncf {

// ---------------------------------------------------------------------------
// Deferred ("catch-up") Adam over the embedding tables -- exactly the dense
// torch.optim.Adam of train_neumf.py:90,115, moving only the rows that need it.
// For a row whose gradient is exactly zero, Adam step s is a fixed per-element fp32
// sequence with step-s scalars (adam_f4 with g = 0), so the steps a row sat out
// can be replayed, in order, when it is next needed, with a bitwise-identical
// result.  last[row] (users [0, U), items [U, U + I)) is the last step applied to
// the row; ring[s % ring_n] the step-s scalars, written by step s's launch.
//
// ncf_batch_touched builds, per global batch b of the epoch stream and per side
// (users, items), three disjoint sorted lists (segments k = 2 * list + side):
//   A_b = the rows batch b touches            (their gradient is in grads)
//   B_b = the rows batch b + 1 touches, not A_b (the next forward reads them);
//         on the epoch's last batch: every row not in A_b
//   C_b = the rows of slice (b % span) of the side's ids, in neither
//         (rolling catch-up: no row falls more than `span` steps behind)
// Step t's launch brings every listed row from last + 1 through t: the replays
// with g = 0, then step t with its gradient (A rows; zero for B and C rows, whose
// gradient is not read).  A rows sat out nothing (they were in A or B the step
// before), B and C rows at most `span` steps, whose scalars are staged in LDS.
// The lists are disjoint, so no row is claimed twice: no atomics.  Each wave
// takes whole rows -- floor(64 / W) rows of W float4 side by side, or one row
// looped over 64 lanes -- so a row's lanes read last before any of them writes it.
// Flush: every row through t = ctl->adam_t (all gradients zero by then).
struct LazyArgs {
    float* p;
    float* g;
    float* m;
    float* v;
    int64_t off[4];  // Ug, Ig, Um, Im flat offsets (< 0: table inactive)
    int w4[4];       // float4s per row of each table
    int U, I;
    const int64_t* seg;  // ncf_batch_touched: [nb * 6 + 1] list offsets (segment k of batch b: 6b + k)
    const int32_t* ids;  // the lists' ids
    int64_t nb;
    int32_t* last;  // [U + I]
    float* ring;    // [ring_n][2]
    int64_t ring_n;
    // packed mode (data parallel, ncf_touched_pack): A_b's summed gradients at
    // packed[k * wrow[side] + ...] (k = position in A_b's list, users first)
    const float* packed;
    int64_t pk_items;  // float offset of the item rows
    int64_t pk_tail;   // float offset of the tower gradient
    int wrow[2];       // floats per packed user / item row
};

constexpr int LZ_WIN = 512;  // step scalars of the last LZ_WIN steps staged in LDS per block

// The block's copy of the step scalars ring[s] for s in [t - LZ_WIN, t).
__device__ __forceinline__ void stage_ring(const LazyArgs& a, int64_t t, float2* win) {
    for (int k = threadIdx.x; k < LZ_WIN; k += blockDim.x) {
        const int64_t s = t - LZ_WIN + k;
        win[k] = s >= 1 ? reinterpret_cast<const float2*>(a.ring)[s % a.ring_n] : float2{0.f, 0.f};
    }
}

__host__ __device__ __forceinline__ int lz_row_w4(const LazyArgs& a, int side) {
    return (a.off[side] >= 0 ? a.w4[side] : 0) + (a.off[side + 2] >= 0 ? a.w4[side + 2] : 0);
}

// flat index of float4 slot k of a row (g table first, then m table)
__device__ __forceinline__ int64_t lz_elem(const LazyArgs& a, int side, int id, int k) {
    const int wa = a.off[side] >= 0 ? a.w4[side] : 0;
    return k < wa ? a.off[side] + ((int64_t)id * a.w4[side] + k) * 4
                  : a.off[side + 2] + ((int64_t)id * a.w4[side + 2] + (k - wa)) * 4;
}

// Bring one float4 of a row from `old` + 1 through t (grad: step t's gradient, or
// null for zero) and store it.
__device__ __forceinline__ void lz_update(const LazyArgs& a, int64_t e, int old, int64_t t, const float* grad,
                                          bool clear_g, float neg_t, float bc2s_t, float w1, float b2, float omb2,
                                          float eps, const float2* win) {
#pragma clang fp contract(off)
    const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
    f4 pp = *reinterpret_cast<const f4*>(a.p + e);
    f4 mm = *reinterpret_cast<const f4*>(a.m + e);
    f4 vv = *reinterpret_cast<const f4*>(a.v + e);
    const f4 gg = grad != nullptr ? *reinterpret_cast<const f4*>(grad) : zero;
    for (int s = old + 1; s < (int)t; ++s) {  // the steps this row sat out: g = 0
        const int64_t kw = s - (t - LZ_WIN);
        const float2 sc = kw >= 0 ? win[kw] : reinterpret_cast<const float2*>(a.ring)[s % a.ring_n];
        adam_f4(pp, mm, vv, zero, w1, b2, omb2, sc.y, eps, sc.x);
    }
    adam_f4(pp, mm, vv, gg, w1, b2, omb2, bc2s_t, eps, neg_t);
    *reinterpret_cast<f4*>(a.m + e) = mm;
    *reinterpret_cast<f4*>(a.v + e) = vv;
    *reinterpret_cast<f4*>(a.p + e) = pp;
    if (clear_g) *reinterpret_cast<f4*>(a.g + e) = zero;
}

// The embedding rows of step t, batch b (flush: every row), one wave task per
// group of rows; tasks per segment: ceil(rows / rows per wave).
__device__ __forceinline__ void lazy_rows(const LazyArgs& a, int64_t t, int64_t b, bool flush, float neg_t,
                                          float bc2s_t, float w1, float b2, float omb2, float eps,
                                          const float2* win, int64_t wave, int64_t nwaves) {
    const int lane = threadIdx.x & 63;
    int64_t n[6], first[6];  // the six segments (flush: every user, every item as segments 2, 3)
    for (int k = 0; k < 6; ++k) {
        if (flush) {
            n[k] = k == 2 ? a.U : (k == 3 ? a.I : 0);
            first[k] = 0;
        } else {
            first[k] = a.seg[6 * b + k];
            n[k] = a.seg[6 * b + k + 1] - first[k];
        }
    }
    int W[2], per[2];
    for (int sd = 0; sd < 2; ++sd) {
        W[sd] = lz_row_w4(a, sd);
        per[sd] = W[sd] == 0 ? 0 : (W[sd] <= 64 ? 64 / W[sd] : 1);
    }
    int64_t tasks[6], tsum = 0;
    for (int k = 0; k < 6; ++k) {
        const int sd = k & 1;
        tasks[k] = per[sd] == 0 ? 0 : (n[k] + per[sd] - 1) / per[sd];
        tsum += tasks[k];
    }
    for (int64_t task = wave; task < tsum; task += nwaves) {
        int k = 0;
        int64_t q = task;
        while (q >= tasks[k]) q -= tasks[k++];
        const int sd = k & 1;
        const int w = W[sd];
        const int r = w <= 64 ? lane / w : 0;  // this lane's row of the task
        const int64_t item = q * per[sd] + r;
        if (r >= per[sd] || item >= n[k]) continue;
        const int id = flush ? (int)item : a.ids[first[k] + item];
        const int64_t slot = sd ? a.U + id : id;
        const int old = a.last[slot];
        const bool is_a = k < 2;  // A rows carry step t's gradient
        if (old < (int)t) {
            const int k0 = w <= 64 ? lane - r * w : lane, kstep = w <= 64 ? w : 64;
            for (int kk = k0; kk < w; kk += kstep) {
                const int64_t e = lz_elem(a, sd, id, kk);
                const float* grad = nullptr;
                if (is_a)
                    grad = a.packed != nullptr
                               ? a.packed + (sd ? a.pk_items + item * a.wrow[1] : item * a.wrow[0]) + 4 * kk
                               : a.g + e;
                lz_update(a, e, old, t, grad, is_a && a.packed == nullptr, neg_t, bc2s_t, w1, b2, omb2, eps, win);
            }
            // every lane of the row has read `last` (one wave, in program order): publish t
            if (lane == (w <= 64 ? r * w : 0)) a.last[slot] = (int)t;
        }
    }
}

__global__ __launch_bounds__(256) void lazy_adam_kernel(const float* __restrict__ slab, int lo, int stride, int rows,
                                                        int nA, int64_t tb, int64_t tower_len, Ranges R,
                                                        ncf_step_ctl* ctl, double lr, double beta1, double beta2,
                                                        float eps, float* loss_hist, int64_t hist_len, W0Part wp,
                                                        LazyArgs a, ScCache* scc) {
#pragma clang fp contract(off)
    __shared__ float sc[2];
    __shared__ f4 part[16][16];
    __shared__ float2 win[LZ_WIN];
    const int64_t t_step = ctl->snap_t;
    const int64_t b_step = ctl->snap_batch;
    step_scalars_ahead(scc, t_step, lr, beta1, beta2);
    if ((int)blockIdx.x < nA) {
        tower_reduce_adam_block(slab, lo, stride, rows, tb, tower_len, a.p, a.m, a.v, R, t_step, b_step, lr, beta1,
                                beta2, eps, loss_hist, hist_len, wp, sc, part, scc,
                                a.packed != nullptr ? a.packed + a.pk_tail : nullptr);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.ring[2 * (t_step % a.ring_n)] = sc[0];
            a.ring[2 * (t_step % a.ring_n) + 1] = sc[1];
        }
    } else {
        const ScCache sce = sc_peek(scc, t_step);
        stage_ring(a, t_step, win);
        sc_resolve(sce, t_step, lr, beta1, beta2, sc);
        __syncthreads();
        const int64_t b = ((b_step % a.nb) + a.nb) % a.nb;
        const int64_t wpb = blockDim.x >> 6;
        lazy_rows(a, t_step, b, false, sc[0], sc[1], (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps, win,
                  (int64_t)(blockIdx.x - nA) * wpb + (threadIdx.x >> 6), (int64_t)(gridDim.x - nA) * wpb);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->adam_t = t_step;
        ctl->batch = b_step + 1;
    }
}

__global__ __launch_bounds__(256) void lazy_flush_kernel(const ncf_step_ctl* ctl, double beta1, double beta2, float eps,
                                                         LazyArgs a) {
    const int64_t t = ctl->adam_t;
    if (t <= 0) return;
    __shared__ float2 win[LZ_WIN];
    stage_ring(a, t, win);
    __syncthreads();
    const float* sc = a.ring + 2 * (t % a.ring_n);
    const int64_t wpb = blockDim.x >> 6;
    lazy_rows(a, t, 0, true, sc[0], sc[1], (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps, win,
              (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6), (int64_t)gridDim.x * wpb);
}

// ---------------------------------------------------------------------------
// ncf_batch_touched: per (global batch b, side) block, LDS bitmaps of the side's ids
// in batch b and in batch b + 1; the three lists A, B, C of lazy_rows' comment.
// Pass 0 counts them into seg[6 b + k + 1]; a one-block scan turns the counts into
// offsets; pass 1 writes the ids in order (block prefix scans of popcounts).
constexpr int BT_THREADS = 1024;

__device__ __forceinline__ int bt_block_scan(int c, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    __syncthreads();
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int base = 0, all = 0;
    for (int q = 0; q < BT_THREADS / 64; ++q) {
        if (q < wv) base += wsum[q];
        all += wsum[q];
    }
    *total = all;
    return base + incl - c;
}

__global__ __launch_bounds__(BT_THREADS) void batch_touched_kernel(const uint64_t* __restrict__ rows, int64_t n,
                                                                   int64_t B, int U, int I, int64_t nb, int span,
                                                                   int pass, int64_t* __restrict__ seg,
                                                                   int32_t* __restrict__ ids) {
    extern __shared__ uint32_t bits[];  // [cur | nxt], nw words each
    __shared__ int wsum[BT_THREADS / 64];
    const int64_t b = blockIdx.x >> 1;
    const int side = blockIdx.x & 1;
    const int N = side ? I : U;
    const int nw = (N + 31) / 32;
    uint32_t* cur = bits;
    uint32_t* nxt = bits + nw;
    const bool last_b = b + 1 >= nb;
    for (int k = threadIdx.x; k < 2 * nw; k += BT_THREADS) bits[k] = 0u;
    __syncthreads();
    for (int h = 0; h < (last_b ? 1 : 2); ++h) {
        uint32_t* bm = h ? nxt : cur;
        const int64_t r0 = (b + h) * B, r1 = r0 + B < n ? r0 + B : n;
        for (int64_t r = r0 + threadIdx.x; r < r1; r += BT_THREADS) {
            const uint64_t row = rows[r];
            const uint32_t u = (uint32_t)row;
            if (u == 0xffffffffu) continue;  // padding row
            const uint32_t id = side ? (uint32_t)((row >> 32) & 0x7fffffffu) : u;
            if (id < (uint32_t)N) atomicOr(&bm[id >> 5], 1u << (id & 31));
        }
    }
    __syncthreads();
    // slice (b % span) of the ids: [lo, hi)
    const int64_t sl = span > 0 ? b % span : 0;
    const int lo = span > 0 ? (int)(sl * N / span) : 0, hi = span > 0 ? (int)((sl + 1) * N / span) : 0;
    const int per = (nw + BT_THREADS - 1) / BT_THREADS;
    const int w0 = threadIdx.x * per, w1 = w0 + per < nw ? w0 + per : nw;
    auto slice_mask = [&](int w) -> uint32_t {  // bits of word w inside [lo, hi)
        const int a0 = w * 32, a1 = a0 + 32;
        if (last_b || a1 <= lo || a0 >= hi) return 0u;
        uint32_t m = 0xffffffffu;
        if (lo > a0) m &= 0xffffffffu << (lo - a0);
        if (hi < a1) m &= 0xffffffffu >> (a1 - hi);
        return m;
    };
    auto tail_mask = [&](int w) -> uint32_t {  // ids < N
        const int a1 = w * 32 + 32;
        return a1 <= N ? 0xffffffffu : (0xffffffffu >> (a1 - N));
    };
    for (int list = 0; list < 3; ++list) {
        auto word = [&](int w) -> uint32_t {
            const uint32_t c = cur[w], x = nxt[w];
            if (list == 0) return c;
            if (list == 1) return last_b ? (~c & tail_mask(w)) : (x & ~c);
            return slice_mask(w) & ~c & ~x;
        };
        int c = 0;
        for (int w = w0; w < w1; ++w) c += __popc(word(w));
        int total;
        const int pos0 = bt_block_scan(c, wsum, &total);
        const int64_t k = 6 * b + 2 * list + side;
        if (pass == 0) {
            if (threadIdx.x == 0) seg[k + 1] = total;
        } else {
            int32_t* dst = ids + seg[k];
            int pos = pos0;
            for (int w = w0; w < w1; ++w) {
                uint32_t x = word(w);
                while (x) {
                    const int q = __ffs(x) - 1;
                    x &= x - 1;
                    dst[pos++] = w * 32 + q;
                }
            }
        }
    }
}

// counts (seg[1 .. m]) -> offsets (seg[0 .. m]), one block
__global__ __launch_bounds__(BT_THREADS) void touched_scan_kernel(int64_t* __restrict__ seg, int64_t m) {
    __shared__ int64_t wsum[BT_THREADS / 64];
    const int per = (int)((m + BT_THREADS - 1) / BT_THREADS);
    const int64_t i0 = (int64_t)threadIdx.x * per, i1 = i0 + per < m ? i0 + per : m;
    int64_t c = 0;
    for (int64_t i = i0; i < i1; ++i) c += seg[i + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int64_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int64_t base = 0;
    for (int q = 0; q < wv; ++q) base += wsum[q];
    int64_t run = base + incl - c;
    __syncthreads();
    for (int64_t i = i0; i < i1; ++i) {
        const int64_t v = seg[i + 1];
        seg[i + 1] = run + v;  // inclusive: seg[i + 1] = offset of segment i + 1
        run += v;
    }
    if (threadIdx.x == 0) seg[0] = 0;
}

// ncf_touched_pack: this rank's gradient of batch b's A rows (users, then items;
// each row its active tables' floats, g table first) into packed slots in list
// order, those rows of grads cleared; slots past the batch's count are zeroed so
// the all-reduce adds nothing stale.  One wave task per group of rows.
__global__ __launch_bounds__(256) void touched_pack_kernel(const ncf_step_ctl* __restrict__ ctl, LazyArgs a, int64_t su,
                                                           int64_t si, float* __restrict__ packed) {
    const int lane = threadIdx.x & 63;
    const int64_t b = ((ctl->snap_batch % a.nb) + a.nb) % a.nb;
    const int64_t nu = a.seg[6 * b + 1] - a.seg[6 * b], ni = a.seg[6 * b + 2] - a.seg[6 * b + 1];
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
    int W[2], per[2];
    for (int sd = 0; sd < 2; ++sd) {
        W[sd] = lz_row_w4(a, sd);
        per[sd] = W[sd] == 0 ? 0 : (W[sd] <= 64 ? 64 / W[sd] : 1);
    }
    const int64_t tu = per[0] ? (su + per[0] - 1) / per[0] : 0, ti = per[1] ? (si + per[1] - 1) / per[1] : 0;
    for (int64_t task = wave; task < tu + ti; task += nwaves) {
        const int sd = task < tu ? 0 : 1;
        const int64_t q = sd ? task - tu : task;
        const int w = W[sd];
        const int r = w <= 64 ? lane / w : 0;
        const int64_t item = q * per[sd] + r;
        if (r >= per[sd] || item >= (sd ? si : su)) continue;
        float* dst = packed + (sd ? a.pk_items + item * a.wrow[1] : item * a.wrow[0]);
        const int k0 = w <= 64 ? lane - r * w : lane, kstep = w <= 64 ? w : 64;
        if (item >= (sd ? ni : nu)) {
            for (int kk = k0; kk < w; kk += kstep) *reinterpret_cast<f4*>(dst + 4 * kk) = zero;
            continue;
        }
        const int id = a.ids[a.seg[6 * b + sd] + item];
        for (int kk = k0; kk < w; kk += kstep) {
            const int64_t e = lz_elem(a, sd, id, kk);
            *reinterpret_cast<f4*>(dst + 4 * kk) = *reinterpret_cast<const f4*>(a.g + e);
            *reinterpret_cast<f4*>(a.g + e) = zero;
        }
    }
}

// ---------------------------------------------------------------------------
// Owner-sharded sparse gradient exchange -- dp_mode "owner" (include/ncf_hip.h,
// since ABI 17).  It shares the optimizers' Adam arithmetic (adam_f4), slab reduction
// order and step-scalar cache (ncf_adam.h, ncf_host.h) and the table geometry above
// (LazyArgs / lz_elem).
//
// The reference trains one device with dense torch.optim.Adam over nn.Embedding
// tables (scripts/train_neumf.py:90,115; src/ncf/models.py:11-16).  Across W ranks,
// every rank builds the same epoch stream, so every rank knows which embedding rows
// every rank slice of every global batch touches.  Row id (either side) is owned by
// rank id % W.  Per step:
//   pack    this rank's gradient rows, bucketed by owner (slots in ascending id order,
//           the bucket lists built once per epoch), and the reduced tower gradient
//           (slab, W0 partials, loss) into send[o]; those grads rows cleared
//                                                   -> all_to_all  (RCCL, xGMI)
//   adam    owner: per owned row, the W ranks' contributions summed in rank order,
//           then dense Adam over EVERY owned row (the reference's semantics: rows
//           with a zero gradient still move through their moments); tower: the W
//           tails summed in rank order, replicated Adam (bitwise the same on every
//           rank); the updated rows that rank q's NEXT batch reads into send2[q]
//                                                   -> all_to_all
//   unpack  those rows into this rank's parameter replica.
// A rank reads only rows it fetched for the step, so the rest of its replica may be
// stale between full syncs (TrainEngine gathers every owner's rows at the end of a
// run).  Bytes per rank and step: the touched rows out and the next batch's rows in,
// instead of the whole flat gradient through a ring.

constexpr int OW_MAX_WORLD = 16;
constexpr int OW_THREADS = 256;

__device__ __forceinline__ int ow_cnt(const int32_t* rec, int W, int kind, int q, int sd) {
    return rec[(kind * W + q) * 2 + sd];
}
// sorted id list: kind 0 = S (this rank's slice, rows owned by q), 1 = R (slice of rank
// q, rows owned here)
__device__ __forceinline__ int64_t ow_ids_off(const ncf_owner_plan& P, int kind, int q, int sd) {
    const int64_t base = 4 * (int64_t)P.world + (int64_t)kind * P.world * (P.max_u + P.max_i);
    return base + (sd ? (int64_t)P.world * P.max_u + (int64_t)q * P.max_i : (int64_t)q * P.max_u);
}
// start of owned-row chunk c inside list R(q, sd): [nchunk + 1] entries per (q, sd)
__device__ __forceinline__ int64_t ow_starts_off(const ncf_owner_plan& P, int q, int sd) {
    const int64_t base = 4 * (int64_t)P.world + 2 * (int64_t)P.world * (P.max_u + P.max_i);
    return base + (sd ? (int64_t)P.world * (P.nchunk_u + 1) + (int64_t)q * (P.nchunk_i + 1)
                      : (int64_t)q * (P.nchunk_u + 1));
}
// float offset of slot k of side sd inside one exchange chunk
__device__ __forceinline__ int64_t ow_slot(const ncf_owner_plan& P, int sd, int64_t k) {
    return sd ? (int64_t)P.max_u * P.row_u + k * P.row_i : k * P.row_u;
}
__device__ __forceinline__ int64_t ow_own_rows(int64_t N, int W, int me) { return N > me ? (N - 1 - me) / W + 1 : 0; }

// ---------------------------------------------------------------------------
// ncf_owner_lists: one 1024-thread block per (batch b, rank slice r).  LDS bitmaps
// of the slice's user and item ids (the rows ncf_train_step gives rank r:
// [r ceil(cnt/W), ...) of the batch), then per owner o the ids with id % W == o in
// ascending order (block prefix scans of masked popcounts): rank `me` keeps S(o) =
// its own slice's lists and R(r) = every slice's list of the rows it owns, with the
// chunk starts of R(r) over its owned rows.  Every block also takes the maximum list
// length over all (r, o) into max_counts (identical on every rank: the a2a chunk
// sizes); lists longer than max_u / max_i are truncated (the host regrows).
__global__ __launch_bounds__(BT_THREADS) void owner_lists_kernel(const uint64_t* __restrict__ rows, ncf_owner_plan P,
                                                                 int U, int I, int32_t* __restrict__ lists,
                                                                 int32_t* __restrict__ max_counts) {
    extern __shared__ uint32_t bits[];  // [users nwu | items nwi]
    __shared__ int wsum[BT_THREADS / 64];
    __shared__ uint32_t rep[32];
    __shared__ int tot[OW_MAX_WORLD];
    const int W = P.world, me = P.rank;
    const int64_t b = blockIdx.x / W;
    const int r = (int)(blockIdx.x % W);
    const int nwu = (U + 31) / 32, nwi = (I + 31) / 32;
    for (int k = threadIdx.x; k < nwu + nwi; k += BT_THREADS) bits[k] = 0u;
    if (threadIdx.x < 32) {  // rep[k]: the bits j of a word with j % W == k
        uint32_t m = 0u;
        for (int j = (int)threadIdx.x; j < 32 && (int)threadIdx.x < W; j += W) m |= 1u << j;
        rep[threadIdx.x] = m;
    }
    __syncthreads();
    const int64_t r0 = b * P.batch_global;
    const int64_t cnt = P.n_total - r0 < P.batch_global ? P.n_total - r0 : P.batch_global;
    const int64_t per = (cnt + W - 1) / W;
    const int64_t lo = (int64_t)r * per < cnt ? (int64_t)r * per : cnt;
    const int64_t hi = lo + per < cnt ? lo + per : cnt;
    for (int64_t k = r0 + lo + threadIdx.x; k < r0 + hi; k += BT_THREADS) {
        const uint64_t row = rows[k];
        const uint32_t u = (uint32_t)row;
        if (u == 0xffffffffu) continue;  // padding row
        const uint32_t it = (uint32_t)((row >> 32) & 0x7fffffffu);
        if (u < (uint32_t)U) atomicOr(&bits[u >> 5], 1u << (u & 31));
        if (it < (uint32_t)I) atomicOr(&bits[nwu + (it >> 5)], 1u << (it & 31));
    }
    __syncthreads();
    int32_t* rec = lists + b * P.record_ints;
    for (int sd = 0; sd < 2; ++sd) {
        const uint32_t* bm = sd ? bits + nwu : bits;
        const int nw = sd ? nwi : nwu;
        const int M = sd ? P.max_i : P.max_u;
        const int pw = (nw + BT_THREADS - 1) / BT_THREADS;
        const int w0 = threadIdx.x * pw < nw ? threadIdx.x * pw : nw;
        const int w1 = w0 + pw < nw ? w0 + pw : nw;
        auto omask = [&](int w, int o) -> uint32_t { return rep[(o - (32 * w) % W + W) % W]; };
        // every owner's list length: the global maximum sizes the exchange
        if (threadIdx.x < OW_MAX_WORLD) tot[threadIdx.x] = 0;
        __syncthreads();
        for (int o = 0; o < W; ++o) {
            int c = 0;
            for (int w = w0; w < w1; ++w) c += __popc(bm[w] & omask(w, o));
            if (c) atomicAdd(&tot[o], c);
        }
        __syncthreads();
        if ((int)threadIdx.x < W) atomicMax(&max_counts[sd], tot[threadIdx.x]);
        const int64_t nch = sd ? P.nchunk_i : P.nchunk_u;
        const int64_t span = (int64_t)W * (sd ? P.chunk_i : P.chunk_u);  // ids per owned-row chunk
        for (int o = 0; o < W; ++o) {
            const bool ks = r == me, kr = o == me;
            if (!ks && !kr) continue;
            int c = 0;
            for (int w = w0; w < w1; ++w) c += __popc(bm[w] & omask(w, o));
            int total;
            const int pos0 = bt_block_scan(c, wsum, &total);
            const int kept = total < M ? total : M;
            if (threadIdx.x == 0) {
                if (ks) rec[(0 * W + o) * 2 + sd] = kept;
                if (kr) rec[(1 * W + r) * 2 + sd] = kept;
            }
            int32_t* sids = rec + ow_ids_off(P, 0, o, sd);
            int32_t* rids = rec + ow_ids_off(P, 1, r, sd);
            int32_t* starts = rec + ow_starts_off(P, r, sd);
            int pos = pos0;
            for (int w = w0; w < w1; ++w) {
                uint32_t x = bm[w] & omask(w, o);
                if (kr) {  // chunk boundaries B_c = me + span c inside this word
                    int64_t cb = 32 * (int64_t)w <= me ? 0 : (32 * (int64_t)w - me + span - 1) / span;
                    for (; cb <= nch && me + span * cb < 32 * (int64_t)w + 32; ++cb) {
                        const int below = (int)(me + span * cb - 32 * (int64_t)w);  // bits under B_c
                        const uint32_t lowm = below >= 32 ? 0xffffffffu : ((1u << below) - 1u);
                        const int s = pos + __popc(x & lowm);
                        starts[cb] = s < M ? s : M;
                    }
                }
                while (x) {
                    const int q = __ffs(x) - 1;
                    x &= x - 1;
                    if (pos < M) {
                        if (ks) sids[pos] = w * 32 + q;
                        if (kr) rids[pos] = w * 32 + q;
                    }
                    ++pos;
                }
            }
            if (kr && threadIdx.x == 0) {  // boundaries past the bitmap: the whole list
                int64_t cb = 32 * (int64_t)nw <= me ? 0 : (32 * (int64_t)nw - me + span - 1) / span;
                for (; cb <= nch; ++cb) starts[cb] = kept;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// ncf_owner_pack: blocks [0, nA) reduce 64 slab columns each (reduce_slab_kernel's
// order) into the tail of every destination chunk; the rest copy this rank's
// gradient rows of batch b into the slots of S(o) and clear them in grads.  One wave
// task per group of rows (floor(64 / w4) rows of w4 float4 side by side).
__device__ __forceinline__ void ow_row_task(const ncf_owner_plan& P, const LazyArgs& a, int64_t task, int lane,
                                            int* o_out, int* sd_out, int64_t* item_out, int* k0, int* kstep,
                                            int* w4_out) {
    int W4[2], per[2];
    int64_t tk[2];
    for (int sd = 0; sd < 2; ++sd) {
        W4[sd] = lz_row_w4(a, sd);
        per[sd] = W4[sd] == 0 ? 0 : (W4[sd] <= 64 ? 64 / W4[sd] : 1);
        const int M = sd ? P.max_i : P.max_u;
        tk[sd] = per[sd] ? (M + per[sd] - 1) / per[sd] : 0;
    }
    const int64_t tpo = tk[0] + tk[1];
    const int o = (int)(task / tpo);
    int64_t q = task - (int64_t)o * tpo;
    const int sd = q < tk[0] ? 0 : 1;
    if (sd) q -= tk[0];
    const int w = W4[sd];
    const int r = w <= 64 ? lane / w : 0;
    *o_out = o;
    *sd_out = sd;
    *item_out = r < per[sd] ? q * per[sd] + r : -1;
    *k0 = w <= 64 ? lane - r * w : lane;
    *kstep = w <= 64 ? w : 64;
    *w4_out = w;
}

__host__ __device__ __forceinline__ int64_t ow_row_tasks(const ncf_owner_plan& P, const LazyArgs& a) {
    int64_t t = 0;
    for (int sd = 0; sd < 2; ++sd) {
        const int w = lz_row_w4(a, sd);
        const int per = w == 0 ? 0 : (w <= 64 ? 64 / w : 1);
        const int M = sd ? P.max_i : P.max_u;
        t += per ? (M + per - 1) / per : 0;
    }
    return t * P.world;
}

__global__ __launch_bounds__(OW_THREADS) void owner_pack_kernel(const float* __restrict__ slab, int lo, int stride,
                                                                int rows, int nA, W0Part wp, ncf_owner_plan P, LazyArgs a,
                                                                const int32_t* __restrict__ lists,
                                                                const ncf_step_ctl* __restrict__ ctl,
                                                                float* __restrict__ send) {
    __shared__ f4 part[16][16];
    if ((int)blockIdx.x < nA) {
        const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;
        const int j = lo + (blockIdx.x * 16 + c4) * 4;
        const f4 t = slab_column_total(slab, j, stride, rows, wp, rg, c4, part);
        if (rg == 0 && j < stride)
            for (int o = 0; o < P.world; ++o) *reinterpret_cast<f4*>(send + o * P.send_floats + P.tail_offset + j) = t;
        return;
    }
    const int lane = threadIdx.x & 63;
    const int64_t b = ((ctl->snap_batch % P.nb) + P.nb) % P.nb;
    const int32_t* rec = lists + b * P.record_ints;
    const int64_t wave = ((int64_t)(blockIdx.x - nA) * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)(gridDim.x - nA) * blockDim.x) >> 6;
    const int64_t ntask = ow_row_tasks(P, a);
    const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
    for (int64_t task = wave; task < ntask; task += nwaves) {
        int o, sd, k0, kstep, w;
        int64_t item;
        ow_row_task(P, a, task, lane, &o, &sd, &item, &k0, &kstep, &w);
        if (item < 0) continue;
        // count and id requested together (the slot is inside the record either way)
        const int cnt = ow_cnt(rec, P.world, 0, o, sd);
        const int id = rec[ow_ids_off(P, 0, o, sd) + item];
        if (item >= cnt) continue;
        float* dst = send + o * P.send_floats + ow_slot(P, sd, item);
        for (int kk = k0; kk < w; kk += kstep) {
            const int64_t e = lz_elem(a, sd, id, kk);
            *reinterpret_cast<f4*>(dst + 4 * kk) = *reinterpret_cast<const f4*>(a.g + e);
            *reinterpret_cast<f4*>(a.g + e) = zero;
        }
    }
}

// ---------------------------------------------------------------------------
// ncf_owner_adam.  Blocks [0, nA): 256 tower float4 columns each -- the W tails summed
// in rank order, Adam on the active ones (replicated), the loss column to the history,
// block 0 commits the control block.  Other blocks: one chunk of owned rows each
// (users, then items), one float4 of the chunk per thread (chunk = floor(256 / w4)
// rows).  The dependent memory round trips are kept to four: the control block; the
// chunk's entry ranges in the lists of this batch (R(r)) and of the next (R(q)); the
// entries' ids (-> per-list slot of each chunk row, in LDS); the W ranks' gradient
// values -- all issued together, summed in rank order.  The row's parameters and
// moments are requested at the top.  The updated float4 goes straight to every rank
// whose next batch reads the row.
constexpr int OW_MAX_CH = 64;  // rows per chunk at most (w4 >= 4)

// WM: register slots for the world's contributions (8 or 16); EPT: float4 per thread
template <int WM, int EPT>
__global__ __launch_bounds__(OW_THREADS) void owner_adam_kernel(ncf_owner_plan P, LazyArgs a, int lo, int stride, int nA,
                                                                int64_t tb, int64_t tower_len, Ranges R,
                                                                ncf_step_ctl* ctl, double lr, double beta1,
                                                                double beta2, float eps, float* loss_hist,
                                                                int64_t hist_len, const int32_t* __restrict__ lists,
                                                                const float* __restrict__ recv,
                                                                float* __restrict__ send2, ScCache* scc) {
#pragma clang fp contract(off)
    __shared__ float sc[2];
    __shared__ int rng[2][OW_MAX_WORLD][2];               // [this / next batch][list][k0, k1]
    __shared__ int smap[2][OW_MAX_WORLD * OW_MAX_CH];    // slot of chunk row jl in list r, -1: absent
    const int64_t t_step = ctl->snap_t;
    const int64_t b_step = ctl->snap_batch;
    step_scalars_ahead(scc, t_step, lr, beta1, beta2);
    const ScCache sce = sc_peek(scc, t_step);
    const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
    const int W = P.world, me = P.rank;
    const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
    if ((int)blockIdx.x < nA) {
        const int j = lo + (blockIdx.x * OW_THREADS + threadIdx.x) * 4;
        const int64_t i = tb + j;
        const bool upd = j < tower_len && in_ranges(R, i);
        f4 pp, mm, vv;
        if (upd) {
            pp = *reinterpret_cast<const f4*>(a.p + i);
            mm = *reinterpret_cast<const f4*>(a.m + i);
            vv = *reinterpret_cast<const f4*>(a.v + i);
        }
        f4 x[WM];
#pragma unroll
        for (int r = 0; r < WM; ++r)
            x[r] = (r < W && j < stride) ? *reinterpret_cast<const f4*>(recv + r * P.send_floats + P.tail_offset + j)
                                         : zero;
        f4 s = zero;
#pragma unroll
        for (int r = 0; r < WM; ++r)
            if (r < W) { s.x += x[r].x; s.y += x[r].y; s.z += x[r].z; s.w += x[r].w; }
        sc_resolve(sce, t_step, lr, beta1, beta2, sc);
        __syncthreads();
        if (j == tower_len) {
            if (loss_hist != nullptr && hist_len > 0) loss_hist[((b_step % hist_len) + hist_len) % hist_len] = s.x;
        } else if (upd) {
            adam_f4(pp, mm, vv, s, w1, b2, omb2, sc[1], eps, sc[0]);
            *reinterpret_cast<f4*>(a.m + i) = mm;
            *reinterpret_cast<f4*>(a.v + i) = vv;
            *reinterpret_cast<f4*>(a.p + i) = pp;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {  // no other block of this launch reads these two
            ctl->adam_t = t_step;
            ctl->batch = b_step + 1;
        }
        return;
    }
    const int64_t blk = blockIdx.x - nA;
    const int sd = blk < P.nchunk_u ? 0 : 1;
    const int64_t c = sd ? blk - P.nchunk_u : blk;
    const int CH = sd ? P.chunk_i : P.chunk_u;
    const int w4 = lz_row_w4(a, sd);
    const int64_t nown = ow_own_rows(sd ? a.I : a.U, W, me);
    const int64_t j0 = c * CH;
    const int jn = (int)(nown - j0 < CH ? nown - j0 : CH);
    // EPT float4 of the chunk per thread (elements e = tid + k 256), parameters and
    // moments requested first
    int jl[EPT], kk[EPT];
    int64_t el[EPT];
    bool act[EPT];
    f4 pp[EPT], mm[EPT], vv[EPT];
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
        const int e = threadIdx.x + q * OW_THREADS;
        act[q] = e < jn * w4;
        jl[q] = act[q] ? e / w4 : 0;
        kk[q] = act[q] ? e - jl[q] * w4 : 0;
        const int id = (int)(me + (int64_t)W * (j0 + jl[q]));
        el[q] = act[q] ? lz_elem(a, sd, id, kk[q]) : 0;
        pp[q] = mm[q] = vv[q] = zero;
        if (act[q]) {
            pp[q] = *reinterpret_cast<const f4*>(a.p + el[q]);
            mm[q] = *reinterpret_cast<const f4*>(a.m + el[q]);
            vv[q] = *reinterpret_cast<const f4*>(a.v + el[q]);
        }
    }
    const int64_t b = ((b_step % P.nb) + P.nb) % P.nb, b1 = (b + 1) % P.nb;
    const int32_t* rec[2] = {lists + b * P.record_ints, lists + b1 * P.record_ints};
    for (int k = threadIdx.x; k < 2 * OW_MAX_WORLD * OW_MAX_CH; k += OW_THREADS) (&smap[0][0])[k] = -1;
    if (threadIdx.x < 2 * W) {  // the chunk's entry range in list r of this batch / the next
        const int h = threadIdx.x / W, r = threadIdx.x - h * W;
        const int32_t* st = rec[h] + ow_starts_off(P, r, sd);
        rng[h][r][0] = st[c];
        rng[h][r][1] = st[c + 1];
    }
    sc_resolve(sce, t_step, lr, beta1, beta2, sc);
    __syncthreads();
    // every entry of the 2W lists inside the chunk -> its slot in smap (next batch: only
    // the other ranks' lists, this replica holds its own rows)
    int tot = 0;
    for (int h = 0; h < 2; ++h)
        for (int r = 0; r < W; ++r)
            if (!(h == 1 && r == me)) tot += rng[h][r][1] - rng[h][r][0];
    for (int q = threadIdx.x; q < tot; q += OW_THREADS) {
        int h = 0, r = 0, k = q;
        for (;; ) {
            const int n = (h == 1 && r == me) ? 0 : rng[h][r][1] - rng[h][r][0];
            if (k < n) break;
            k -= n;
            if (++r == W) { r = 0; ++h; }
        }
        k += rng[h][r][0];
        const int rid = rec[h][ow_ids_off(P, 1, r, sd) + k];
        smap[h][r * OW_MAX_CH + (int)((rid - me) / W - j0)] = k;
    }
    __syncthreads();
    // the W ranks' contributions to each float4, all requested, summed in rank order
    f4 x[EPT][WM];
#pragma unroll
    for (int q = 0; q < EPT; ++q)
#pragma unroll
        for (int r = 0; r < WM; ++r) {
            const int k = (act[q] && r < W) ? smap[0][r * OW_MAX_CH + jl[q]] : -1;
            x[q][r] = k >= 0 ? *reinterpret_cast<const f4*>(recv + r * P.send_floats + ow_slot(P, sd, k) + 4 * kk[q])
                             : zero;
        }
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
        if (!act[q]) continue;
        f4 g = zero;
#pragma unroll
        for (int r = 0; r < WM; ++r)
            if (r < W && smap[0][r * OW_MAX_CH + jl[q]] >= 0) {
                g.x += x[q][r].x; g.y += x[q][r].y; g.z += x[q][r].z; g.w += x[q][r].w;
            }
        // dense Adam on every owned row (a zero gradient still moves the moments)
        adam_f4(pp[q], mm[q], vv[q], g, w1, b2, omb2, sc[1], eps, sc[0]);
        *reinterpret_cast<f4*>(a.m + el[q]) = mm[q];
        *reinterpret_cast<f4*>(a.v + el[q]) = vv[q];
        *reinterpret_cast<f4*>(a.p + el[q]) = pp[q];
        for (int r = 0; r < W; ++r) {  // the ranks whose next batch reads the row
            const int k = smap[1][r * OW_MAX_CH + jl[q]];
            if (k >= 0) *reinterpret_cast<f4*>(send2 + r * P.param_floats + ow_slot(P, sd, k) + 4 * kk[q]) = pp[q];
        }
    }
}

// ncf_owner_unpack: the next batch's rows of S(o), o != this rank, from recv2[o] into
// the parameter replica.
__global__ __launch_bounds__(OW_THREADS) void owner_unpack_kernel(ncf_owner_plan P, LazyArgs a,
                                                                  const int32_t* __restrict__ lists,
                                                                  const ncf_step_ctl* __restrict__ ctl,
                                                                  const float* __restrict__ recv2) {
    const int lane = threadIdx.x & 63;
    const int64_t b1 = (((ctl->snap_batch % P.nb) + P.nb) % P.nb + 1) % P.nb;
    const int32_t* rec = lists + b1 * P.record_ints;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t ntask = ow_row_tasks(P, a);
    for (int64_t task = wave; task < ntask; task += nwaves) {
        int o, sd, k0, kstep, w;
        int64_t item;
        ow_row_task(P, a, task, lane, &o, &sd, &item, &k0, &kstep, &w);
        if (o == P.rank || item < 0) continue;
        const int cnt = ow_cnt(rec, P.world, 0, o, sd);
        const int id = rec[ow_ids_off(P, 0, o, sd) + item];
        if (item >= cnt) continue;
        const float* src = recv2 + o * P.param_floats + ow_slot(P, sd, item);
        for (int kk = k0; kk < w; kk += kstep)
            *reinterpret_cast<f4*>(a.p + lz_elem(a, sd, id, kk)) = *reinterpret_cast<const f4*>(src + 4 * kk);
    }
}

// float4 per thread in ncf_owner_adam: two where one float4 a thread would take more
// than ~4 blocks per CU (and up to 8 ranks: 8 contribution registers each) -- one round
// of resident blocks at C4's 8-rank shard; one otherwise (C3: more, shorter blocks)
static int ow_ept(int world, int64_t owned_f4) { return world <= 8 && owned_f4 > 1024LL * OW_THREADS ? 2 : 1; }

static int64_t ow_grid(int64_t waves) {
    int64_t nb = (waves + OW_THREADS / 64 - 1) / (OW_THREADS / 64);
    if (nb > 4096) nb = 4096;
    return nb < 1 ? 1 : nb;
}

}  // namespace ncf

using namespace ncf;

extern "C" {

// ---- deferred Adam (ABI 14)
// C-list slice count: a row not touched by two consecutive batches falls at most
// this many steps behind (NCF_LAZY_SPAN, default 32, < LZ_WIN)
static int lazy_span() {
    static const int span = [] {
        const char* e = getenv("NCF_LAZY_SPAN");
        const int v = e ? atoi(e) : 32;
        return v < 1 ? 1 : (v > LZ_WIN - 2 ? LZ_WIN - 2 : v);
    }();
    return span;
}

constexpr int LZ_MAX_ROWS = 1 << 19;  // per side: two LDS bitmaps of the ids in ncf_batch_touched

static int lazy_args(const ncf_layout* lay, float* params, float* grads, float* m, float* v, const int64_t* ranges,
                     int nranges, int32_t* last, float* ring, int64_t ring_n, LazyArgs* a) {
    const int f = lay->factor_num, dm = f << (lay->num_layers - 1);
    if (f % 4 != 0 || lay->user_num > LZ_MAX_ROWS || lay->item_num > LZ_MAX_ROWS) return NCF_E_UNSUPPORTED;
    const int64_t offs[4] = {lay->ug, lay->ig, lay->um, lay->im};
    const int64_t widths[4] = {f, f, dm, dm};
    const int64_t nrows[4] = {lay->user_num, lay->item_num, lay->user_num, lay->item_num};
    memset(a, 0, sizeof(*a));
    for (int k = 0; k < 4; ++k) {
        const int64_t b = offs[k], e = offs[k] + nrows[k] * widths[k];
        bool act = false;
        for (int i = 0; i < nranges; ++i)
            if (ranges[2 * i] < e && ranges[2 * i + 1] > b) act = true;
        a->off[k] = act ? offs[k] : -1;
        a->w4[k] = (int)(widths[k] / 4);
    }
    a->p = params;
    a->g = grads;
    a->m = m;
    a->v = v;
    a->U = lay->user_num;
    a->I = lay->item_num;
    a->last = last;
    a->ring = ring;
    a->ring_n = ring_n;
    return NCF_OK;
}

// touched-list geometry: batches, per-batch A slots per side, id capacity
struct TouchedShape {
    int64_t nb, su, si, segs, cap;
};

static TouchedShape touched_shape(int64_t n, int64_t B, int U, int I) {
    TouchedShape t;
    t.nb = (n + B - 1) / B;
    t.su = U < B ? U : B;
    t.si = I < B ? I : B;
    t.segs = 6 * t.nb + 1;
    const int span = lazy_span();
    // per batch and side: |A| + |B| <= min(N, 2 min(N, B)), |C| <= N / span + 1; the
    // last batch lists every id once
    const int64_t ab = (U < 2 * t.su ? U : 2 * t.su) + (I < 2 * t.si ? I : 2 * t.si);
    t.cap = t.nb * (ab + U / span + I / span + 2) + U + I;
    return t;
}

int64_t ncf_touched_bytes(int64_t n, int64_t batch_global, int user_num, int item_num) {
    if (n <= 0 || batch_global <= 0 || user_num <= 0 || item_num <= 0) return -1;
    const TouchedShape t = touched_shape(n, batch_global, user_num, item_num);
    return (8 * t.segs + 4 * t.cap + 15) / 16 * 16;
}

static void touched_lists(LazyArgs* a, const int32_t* touched, const TouchedShape& t) {
    a->nb = t.nb;
    a->seg = reinterpret_cast<const int64_t*>(touched);
    a->ids = touched + 2 * t.segs;
}

int ncf_batch_touched(const uint64_t* rows, int64_t n, int64_t batch_global, int user_num, int item_num,
                      int32_t* touched, void* stream) {
    if (!rows || !touched || n <= 0 || batch_global <= 0 || user_num <= 0 || item_num <= 0) return NCF_E_ARG;
    if ((reinterpret_cast<uintptr_t>(touched) & 7) != 0) return NCF_E_ARG;
    if (user_num > LZ_MAX_ROWS || item_num > LZ_MAX_ROWS) return NCF_E_UNSUPPORTED;
    const TouchedShape t = touched_shape(n, batch_global, user_num, item_num);
    const int mx = user_num > item_num ? user_num : item_num;
    const int64_t lds = 2 * (int64_t)((mx + 31) / 32) * 4;
    if (lds > 64 * 1024 && ensure_lds((const void*)batch_touched_kernel, lds) != NCF_OK) return NCF_E_LAUNCH;
    int64_t* seg = reinterpret_cast<int64_t*>(touched);
    int32_t* ids = touched + 2 * t.segs;
    const int span = lazy_span();
    hipLaunchKernelGGL(batch_touched_kernel, dim3((unsigned)(2 * t.nb)), dim3(BT_THREADS), (size_t)lds,
                       (hipStream_t)stream, rows, n, batch_global, user_num, item_num, t.nb, span, 0, seg, ids);
    hipLaunchKernelGGL(touched_scan_kernel, dim3(1), dim3(BT_THREADS), 0, (hipStream_t)stream, seg, t.segs - 1);
    hipLaunchKernelGGL(batch_touched_kernel, dim3((unsigned)(2 * t.nb)), dim3(BT_THREADS), (size_t)lds,
                       (hipStream_t)stream, rows, n, batch_global, user_num, item_num, t.nb, span, 1, seg, ids);
    return launch_status();
}

// blocks for one step's rows: an upper bound of its wave tasks, 4 waves a block
static int64_t lazy_blocks(const LazyArgs& a, int64_t rows_u, int64_t rows_i) {
    int64_t waves = 0;
    for (int sd = 0; sd < 2; ++sd) {
        const int w = (a.off[sd] >= 0 ? a.w4[sd] : 0) + (a.off[sd + 2] >= 0 ? a.w4[sd + 2] : 0);
        if (w == 0) continue;
        const int per = w <= 64 ? 64 / w : 1;
        waves += ((sd ? rows_i : rows_u) + per - 1) / per;
    }
    int64_t nB = (waves + 3) / 4;
    if (nB > 2048) nB = 2048;
    return nB < 1 ? 1 : nB;
}

static int64_t step_blocks(const LazyArgs& a, const TouchedShape& t) {
    const int span = lazy_span();
    const int64_t ru = (a.U < 2 * t.su ? a.U : 2 * t.su) + a.U / span + 1;
    const int64_t ri = (a.I < 2 * t.si ? a.I : 2 * t.si) + a.I / span + 1;
    return lazy_blocks(a, ru, ri);
}

int ncf_lazy_adam_step(const ncf_layout* lay, const void* workspace, float* params, float* grads, float* exp_avg,
                       float* exp_avg_sq, const int64_t* ranges, int nranges, ncf_step_ctl* ctl, double lr,
                       double beta1, double beta2, double eps, float* loss_hist, int64_t hist_len,
                       const int32_t* touched, int64_t n_total, int64_t batch_global, int32_t* last_step,
                       float* step_scalars, int64_t ring, void* stream) {
    if (!lay || !workspace || !params || !grads || !exp_avg || !exp_avg_sq || !ranges || !ctl || !touched ||
        !last_step || !step_scalars || n_total <= 0 || batch_global <= 0 || ring < LZ_WIN + 2)
        return NCF_E_ARG;
    int err = 0;
    Ranges R = make_ranges(ranges, nranges, &err);
    if (err) return NCF_E_ARG;
    LazyArgs a;
    const int rc = lazy_args(lay, params, grads, exp_avg, exp_avg_sq, ranges, nranges, last_step, step_scalars, ring, &a);
    if (rc != NCF_OK) return rc;
    const TouchedShape t = touched_shape(n_total, batch_global, lay->user_num, lay->item_num);
    touched_lists(&a, touched, t);
    const int stride = (int)ncf_slab_stride(lay);
    const int lo = slab_lo(lay);
    const int nA = (stride - lo + 63) / 64;
    const int rows = reduce_rows(lay);
    const int64_t nB = step_blocks(a, t);
    hipLaunchKernelGGL(lazy_adam_kernel, dim3((unsigned)(nA + nB)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const float*>(workspace), lo, stride, rows, nA, lay->tower_begin, lay->tower_len, R,
                       ctl, lr, beta1, beta2, (float)eps, loss_hist, hist_len, w0_part(lay, workspace), a,
                       sc_cache_for(ctl, stream));
    return launch_status();
}

// packed mode geometry: floats per packed user / item row, the item rows' offset,
// the tail (tower gradient + loss, ncf_slab_stride floats) and the total
static void packed_geometry(const ncf_layout* lay, LazyArgs* a, int64_t su, int64_t si, int64_t* total) {
    a->wrow[0] = 4 * ((a->off[0] >= 0 ? a->w4[0] : 0) + (a->off[2] >= 0 ? a->w4[2] : 0));
    a->wrow[1] = 4 * ((a->off[1] >= 0 ? a->w4[1] : 0) + (a->off[3] >= 0 ? a->w4[3] : 0));
    a->pk_items = su * a->wrow[0];
    a->pk_tail = a->pk_items + si * a->wrow[1];
    *total = a->pk_tail + ncf_slab_stride(lay);
}

int64_t ncf_touched_packed_floats(const ncf_layout* lay, const int64_t* ranges, int nranges, int64_t batch_global) {
    if (!lay || !ranges || batch_global <= 0) return -1;
    LazyArgs a;
    if (lazy_args(lay, nullptr, nullptr, nullptr, nullptr, ranges, nranges, nullptr, nullptr, 1, &a) != NCF_OK)
        return -1;
    const TouchedShape t = touched_shape(1, batch_global, lay->user_num, lay->item_num);
    int64_t total;
    packed_geometry(lay, &a, t.su, t.si, &total);
    return total;
}

int ncf_touched_pack(const ncf_layout* lay, const void* workspace, float* grads, const int64_t* ranges, int nranges,
                     const int32_t* touched, int64_t n_total, int64_t batch_global, const ncf_step_ctl* ctl,
                     float* packed, void* stream) {
    if (!lay || !workspace || !grads || !ranges || !touched || !ctl || !packed || n_total <= 0 || batch_global <= 0 )
        return NCF_E_ARG;
    LazyArgs a;
    const int rc = lazy_args(lay, nullptr, grads, nullptr, nullptr, ranges, nranges, nullptr, nullptr, 1, &a);
    if (rc != NCF_OK) return rc;
    const TouchedShape t = touched_shape(n_total, batch_global, lay->user_num, lay->item_num);
    touched_lists(&a, touched, t);
    int64_t total;
    packed_geometry(lay, &a, t.su, t.si, &total);
    // tower gradient (slab rows, W0 partials; loss at tower_len) into the tail
    launch_reduce_slab(lay, workspace, packed + a.pk_tail, nullptr, (hipStream_t)stream);
    // tail[0, lo) is never written: it stays as allocated (zero), and sums to zero
    hipLaunchKernelGGL(touched_pack_kernel, dim3((unsigned)lazy_blocks(a, t.su, t.si)), dim3(256), 0,
                       (hipStream_t)stream, ctl, a, t.su, t.si, packed);
    return launch_status();
}

int ncf_lazy_adam_step_packed(const ncf_layout* lay, float* params, float* exp_avg, float* exp_avg_sq,
                              const int64_t* ranges, int nranges, ncf_step_ctl* ctl, double lr, double beta1,
                              double beta2, double eps, float* loss_hist, int64_t hist_len, const int32_t* touched,
                              int64_t n_total, int64_t batch_global, int32_t* last_step, float* step_scalars,
                              int64_t ring, const float* packed, void* stream) {
    if (!lay || !params || !exp_avg || !exp_avg_sq || !ranges || !ctl || !touched || !last_step || !step_scalars ||
        !packed || n_total <= 0 || batch_global <= 0 || ring < LZ_WIN + 2)
        return NCF_E_ARG;
    int err = 0;
    Ranges R = make_ranges(ranges, nranges, &err);
    if (err) return NCF_E_ARG;
    LazyArgs a;
    const int rc = lazy_args(lay, params, nullptr, exp_avg, exp_avg_sq, ranges, nranges, last_step, step_scalars,
                             ring, &a);
    if (rc != NCF_OK) return rc;
    const TouchedShape t = touched_shape(n_total, batch_global, lay->user_num, lay->item_num);
    touched_lists(&a, touched, t);
    a.packed = packed;
    int64_t total;
    packed_geometry(lay, &a, t.su, t.si, &total);
    const int stride = (int)ncf_slab_stride(lay);
    const int lo = slab_lo(lay);
    const int nA = (stride - lo + 63) / 64;
    const int64_t nB = step_blocks(a, t);
    hipLaunchKernelGGL(lazy_adam_kernel, dim3((unsigned)(nA + nB)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)nullptr, lo, stride, 0, nA, lay->tower_begin, lay->tower_len, R, ctl, lr, beta1,
                       beta2, (float)eps, loss_hist, hist_len, W0Part{nullptr, 0, 0, 0, 0}, a, sc_cache_for(ctl, stream));
    return launch_status();
}

int ncf_lazy_adam_flush(const ncf_layout* lay, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                        const int64_t* ranges, int nranges, const ncf_step_ctl* ctl, double beta1, double beta2,
                        double eps, int32_t* last_step, const float* step_scalars, int64_t ring, void* stream) {
    if (!lay || !params || !grads || !exp_avg || !exp_avg_sq || !ranges || !ctl || !last_step || !step_scalars ||
        ring < LZ_WIN + 2)
        return NCF_E_ARG;
    LazyArgs a;
    const int rc = lazy_args(lay, params, grads, exp_avg, exp_avg_sq, ranges, nranges, last_step,
                             const_cast<float*>(step_scalars), ring, &a);
    if (rc != NCF_OK) return rc;
    a.nb = 1;
    hipLaunchKernelGGL(lazy_flush_kernel, dim3((unsigned)lazy_blocks(a, a.U, a.I)), dim3(256), 0, (hipStream_t)stream,
                       ctl, beta1, beta2, (float)eps, a);
    return launch_status();
}

int ncf_owner_plan_init(const ncf_layout* lay, const int64_t* ranges, int nranges, int64_t n_total,
                        int64_t batch_global, int world, int rank, int max_u, int max_i, ncf_owner_plan* out) {
    if (!lay || !ranges || !out || n_total <= 0 || batch_global <= 0 || world < 1 || world > OW_MAX_WORLD ||
        rank < 0 || rank >= world || max_u < 0 || max_i < 0)
        return NCF_E_ARG;
    LazyArgs a;
    const int rc = lazy_args(lay, nullptr, nullptr, nullptr, nullptr, ranges, nranges, nullptr, nullptr, 1, &a);
    if (rc != NCF_OK) return rc;
    ncf_owner_plan& P = *out;
    memset(&P, 0, sizeof(P));
    P.world = world;
    P.rank = rank;
    P.max_u = max_u;
    P.max_i = max_i;
    P.n_total = n_total;
    P.batch_global = batch_global;
    P.nb = (n_total + batch_global - 1) / batch_global;
    P.row_u = 4 * lz_row_w4(a, 0);
    P.row_i = 4 * lz_row_w4(a, 1);
    if (P.row_u > 4 * OW_THREADS || P.row_i > 4 * OW_THREADS) return NCF_E_UNSUPPORTED;  // a row per optimizer block
    // owned rows per optimizer block: ow_ept float4 per thread of a 256-thread block
    const int64_t own_u = lay->user_num > rank ? (lay->user_num - 1 - rank) / world + 1 : 0;
    const int64_t own_i = lay->item_num > rank ? (lay->item_num - 1 - rank) / world + 1 : 0;
    const int ept = ow_ept(world, own_u * (P.row_u / 4) + own_i * (P.row_i / 4));
    auto chunk = [ept](int row) {
        const int w4 = row / 4;
        if (w4 <= 0) return OW_MAX_CH;
        const int c = ept * OW_THREADS / w4;
        return c < 1 ? 1 : (c > OW_MAX_CH ? OW_MAX_CH : c);
    };
    P.chunk_u = chunk(P.row_u);
    P.chunk_i = chunk(P.row_i);
    P.nchunk_u = P.row_u ? (own_u + P.chunk_u - 1) / P.chunk_u : 0;
    P.nchunk_i = P.row_i ? (own_i + P.chunk_i - 1) / P.chunk_i : 0;
    const int64_t ints = 4 * (int64_t)world + 2 * (int64_t)world * (max_u + max_i) +
                         (int64_t)world * (P.nchunk_u + 1 + P.nchunk_i + 1);
    P.record_ints = (ints + 3) & ~(int64_t)3;
    P.lists_bytes = P.nb * P.record_ints * 4;
    P.tail_offset = (int64_t)max_u * P.row_u + (int64_t)max_i * P.row_i;
    P.param_floats = P.tail_offset;
    P.send_floats = P.tail_offset + ncf_slab_stride(lay);
    for (int k = 0; k < 4; ++k) P.off[k] = a.off[k];
    return NCF_OK;
}

static int owner_check(const ncf_owner_plan* P, const ncf_layout* lay, LazyArgs* a, float* p, float* g, float* m,
                       float* v) {
    if (!P || !lay || P->world < 1 || P->world > OW_MAX_WORLD || P->nb <= 0) return NCF_E_ARG;
    int64_t rg[8];  // the plan's active tables as ranges (lazy_args reads activity from them)
    const int64_t f = lay->factor_num, dm = f << (lay->num_layers - 1);
    const int64_t w[4] = {f, f, dm, dm}, n[4] = {lay->user_num, lay->item_num, lay->user_num, lay->item_num};
    int nr = 0;
    for (int k = 0; k < 4; ++k)
        if (P->off[k] >= 0) {
            rg[2 * nr] = P->off[k];
            rg[2 * nr + 1] = P->off[k] + ((n[k] * w[k] + 3) & ~(int64_t)3);
            ++nr;
        }
    if (nr == 0) return NCF_E_ARG;
    return lazy_args(lay, p, g, m, v, rg, nr, nullptr, nullptr, 1, a);
}

int ncf_owner_lists(const ncf_owner_plan* plan, const ncf_layout* lay, const uint64_t* rows, int32_t* lists,
                    int32_t* max_counts, void* stream) {
    LazyArgs a;
    int rc = owner_check(plan, lay, &a, nullptr, nullptr, nullptr, nullptr);
    if (rc != NCF_OK) return rc;
    if (!rows || !lists || !max_counts) return NCF_E_ARG;
    if ((int64_t)plan->nb * plan->world > 0x7fffffff) return NCF_E_ARG;
    const int64_t lds = 4 * (int64_t)((lay->user_num + 31) / 32 + (lay->item_num + 31) / 32);
    if (lds > LDS_LIMIT_BYTES - 4096) return NCF_E_UNSUPPORTED;
    if (lds > 64 * 1024 && ensure_lds(reinterpret_cast<const void*>(&owner_lists_kernel), lds) != NCF_OK)
        return NCF_E_LAUNCH;
    if (hipMemsetAsync(max_counts, 0, 2 * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return NCF_E_LAUNCH;
    hipLaunchKernelGGL(owner_lists_kernel, dim3((unsigned)(plan->nb * plan->world)), dim3(BT_THREADS), (size_t)lds,
                       (hipStream_t)stream, rows, *plan, lay->user_num, lay->item_num, lists, max_counts);
    return launch_status();
}

int ncf_owner_pack(const ncf_owner_plan* plan, const ncf_layout* lay, const void* workspace, float* grads,
                   const int32_t* lists, const ncf_step_ctl* ctl, float* send, void* stream) {
    LazyArgs a;
    int rc = owner_check(plan, lay, &a, nullptr, grads, nullptr, nullptr);
    if (rc != NCF_OK) return rc;
    if (!workspace || !grads || !lists || !ctl || !send) return NCF_E_ARG;
    const int stride = (int)ncf_slab_stride(lay);
    const int lo = slab_lo(lay);
    const int nA = (stride - lo + 63) / 64;
    const int64_t nR = ow_grid(ow_row_tasks(*plan, a));
    hipLaunchKernelGGL(owner_pack_kernel, dim3((unsigned)(nA + nR)), dim3(OW_THREADS), 0, (hipStream_t)stream,
                       static_cast<const float*>(workspace), lo, stride, reduce_rows(lay), nA, w0_part(lay, workspace),
                       *plan, a, lists, ctl, send);
    return launch_status();
}

int ncf_owner_adam(const ncf_owner_plan* plan, const ncf_layout* lay, float* params, float* exp_avg,
                   float* exp_avg_sq, const int64_t* ranges, int nranges, const int32_t* lists, ncf_step_ctl* ctl,
                   double lr, double beta1, double beta2, double eps, float* loss_hist, int64_t hist_len,
                   const float* recv, float* send2, void* stream) {
    LazyArgs a;
    int rc = owner_check(plan, lay, &a, params, nullptr, exp_avg, exp_avg_sq);
    if (rc != NCF_OK) return rc;
    if (!params || !exp_avg || !exp_avg_sq || !ranges || !lists || !ctl || !recv || !send2) return NCF_E_ARG;
    int err = 0;
    Ranges R = make_ranges(ranges, nranges, &err);
    if (err) return NCF_E_ARG;
    const int stride = (int)ncf_slab_stride(lay);
    const int lo = slab_lo(lay);
    const int nA = ((stride - lo) / 4 + OW_THREADS - 1) / OW_THREADS;
    const int64_t nblk = nA + plan->nchunk_u + plan->nchunk_i;
    // the plan's chunks say how many float4 a thread takes
    const int ept = (plan->chunk_u * (plan->row_u / 4) > OW_THREADS || plan->chunk_i * (plan->row_i / 4) > OW_THREADS)
                        ? 2 : 1;
    auto fn = plan->world > 8 ? &owner_adam_kernel<OW_MAX_WORLD, 1>
                              : (ept == 2 ? &owner_adam_kernel<8, 2> : &owner_adam_kernel<8, 1>);
    hipLaunchKernelGGL(fn, dim3((unsigned)nblk), dim3(OW_THREADS), 0, (hipStream_t)stream,
                       *plan, a, lo, stride, nA, lay->tower_begin, lay->tower_len, R, ctl, lr, beta1, beta2,
                       (float)eps, loss_hist, hist_len, lists, recv, send2, sc_cache_for(ctl, stream));
    return launch_status();
}

int ncf_owner_unpack(const ncf_owner_plan* plan, const ncf_layout* lay, float* params, const int32_t* lists,
                     const ncf_step_ctl* ctl, const float* recv2, void* stream) {
    LazyArgs a;
    int rc = owner_check(plan, lay, &a, params, nullptr, nullptr, nullptr);
    if (rc != NCF_OK) return rc;
    if (!params || !lists || !ctl || !recv2) return NCF_E_ARG;
    hipLaunchKernelGGL(owner_unpack_kernel, dim3((unsigned)ow_grid(ow_row_tasks(*plan, a))), dim3(OW_THREADS), 0,
                       (hipStream_t)stream, *plan, a, lists, ctl, recv2);
    return launch_status();
}

}  // extern "C"
