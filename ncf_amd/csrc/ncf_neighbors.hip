// Nearest neighbours over the embedding tables (ncf_neighbors, include/ncf_hip.h; added
// within ABI 21): for every queried row of one side's table, the top_k most similar rows
// of the same table by dot product or cosine, without a Q x N score array.
//
// Vectors.  A space is one or two segments of the flat parameter buffer: GMF = rows of
// embed_*_GMF (width F), MLP = rows of embed_*_MLP (width F << (L - 1)), CONCAT = the GMF
// row followed by the MLP row.  Each segment is zero padded to a multiple of 16 columns.
//
// Score of a pair.  D[16 queries][16 rows] accumulates on v_mfma_f32_16x16x4_f32, which is
// bitwise an fmaf chain over its four k values.  Lane l = (g = l >> 4, it = l & 15) holds
// columns 16 t + 4 g + r (r = 0..3) of query `it` (A operand, from LDS) and of catalogue
// row `it` (B operand, one 16-byte load straight from L2), and MFMA (t, r) multiplies them.
// So the dot of a pair is the one chain
//   for segment, for t, for r = 0..3, for g = 0..3:  acc = fmaf(q[16 t + 4 g + r], c[16 t + 4 g + r], acc)
// whatever tile, chunk or split the pair falls in.  Cosine multiplies by inv[q], then by
// inv[c]; inv[x] = 1 / sqrtf(sum of squares), an fmaf chain in column order written by a
// prologue, and 0 for a zero row.
//
// Geometry.  A workgroup (4 waves) owns a tile of 16 queries, staged once in LDS, and a
// range of 64-row chunks; wave w takes rows 16 w .. 16 w + 15 of each chunk, so no B value
// is used twice inside a workgroup and none is staged.  Each (wave, query) keeps a sorted
// top-K list in LDS, and each lane the last score of the four lists its accumulator
// registers feed, so a tile without a candidate costs four compares and ballots; the four
// lists of a query are merged in LDS after the last chunk.
// Few queries: the chunk range is split over grid.y and rc_merge_kernel orders the
// partial lists.
#include <string.h>

#include "ncf_host.h"

namespace ncf {

constexpr int NB_QT = 16;  // queries per workgroup (the M of one MFMA tile)
constexpr int NB_CH = 64;  // catalogue rows per chunk: 16 per wave

struct NbSeg {
    int64_t off;  // first float of the table in params
    int d, dp;    // row width; width padded to a multiple of 16
    int vec;      // rows are 16-byte aligned: one load per four columns
};

struct NbArgs {
    const float* params;
    const int32_t* queries;
    int64_t nq;
    int N, K;
    NbSeg seg[2];
    int nseg, DP;  // DP: sum of the padded widths
    int cosine, exclude_self;
    float* inv;     // [N]
    float* part_s;  // [nq][nsplit][K]
    int32_t* part_i;
    int nsplit, cps;  // chunk splits; chunks per split
};

// Columns c .. c + 3 of a row of width d (c % 4 == 0), zero beyond d.
__device__ __forceinline__ f4 nb_load4(const float* __restrict__ row, int c, int d, int vec) {
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        if (c < d) v = *reinterpret_cast<const f4*>(row + c);
    } else {
        if (c < d) v.x = row[c];
        if (c + 1 < d) v.y = row[c + 1];
        if (c + 2 < d) v.z = row[c + 2];
        if (c + 3 < d) v.w = row[c + 3];
    }
    return v;
}

// Scores of the last entries of a wave's lists of queries 4 g + r (r = 0..3; ls: the first
// of the four lists): the thresholds lane (g, it) holds for its four accumulator
// registers.  have: how many of the four queries exist; an absent one gets +inf.
__device__ __forceinline__ void nb_thresholds(volatile float* ls, int K, int64_t have, float& t0, float& t1, float& t2,
                                              float& t3) {
    t0 = have > 0 ? ls[K - 1] : INFINITY;
    t1 = have > 1 ? ls[2 * K - 1] : INFINITY;
    t2 = have > 2 ? ls[3 * K - 1] : INFINITY;
    t3 = have > 3 ? ls[4 * K - 1] : INFINITY;
}

// Prologue (cosine): inv[r] of every catalogue row.
__global__ __launch_bounds__(256) void nb_norm_kernel(NbArgs a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.N) return;
    float ss = 0.f;
    for (int s = 0; s < a.nseg; ++s) {
        const float* __restrict__ row = a.params + a.seg[s].off + r * a.seg[s].d;
        for (int i = 0; i < a.seg[s].d; ++i) ss = fmaf(row[i], row[i], ss);
    }
    a.inv[r] = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
}

__global__ __launch_bounds__(RC_WAVES * 64) void nb_kernel(NbArgs a) {
    extern __shared__ f4 nb_smem4[];
    float* const smem = reinterpret_cast<float*>(nb_smem4);
    const int K = a.K, SA = a.DP + 4;
    float* const Aq = smem;                                                      // [NB_QT][SA]
    float* const lists_s = Aq + NB_QT * SA;                                      // [RC_WAVES][NB_QT][K]
    int* const lists_i = reinterpret_cast<int*>(lists_s + RC_WAVES * NB_QT * K);
    float* const invq = reinterpret_cast<float*>(lists_i + RC_WAVES * NB_QT * K);  // [NB_QT]
    int* const qid = reinterpret_cast<int*>(invq + NB_QT);                         // [NB_QT]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, it = lane & 15;
    const float* __restrict__ prm = a.params;
    const int N = a.N;
    const int nchunks = (N + NB_CH - 1) / NB_CH;
    const int split = blockIdx.y;
    const int cb = split * a.cps, ce = min(cb + a.cps, nchunks);
    const int64_t q0 = (int64_t)blockIdx.x * NB_QT;

    // the query tile: ids, inverse norms, rows (zero padded; absent queries are zero rows)
    if (tid < NB_QT) {
        const bool have = q0 + tid < a.nq;
        const int id = have ? a.queries[q0 + tid] : -1;
        qid[tid] = id;
        invq[tid] = (have && a.cosine) ? a.inv[id] : 0.f;
    }
    {
        const int C4 = a.DP / 4;
        for (int idx = tid; idx < NB_QT * C4; idx += RC_WAVES * 64) {
            const int r = idx / C4;
            int col = 4 * (idx - r * C4);
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (q0 + r < a.nq) {
                const int s = (a.nseg > 1 && col >= a.seg[0].dp) ? 1 : 0;
                const int c = col - (s ? a.seg[0].dp : 0);
                v = nb_load4(prm + a.seg[s].off + (int64_t)a.queries[q0 + r] * a.seg[s].d, c, a.seg[s].d, a.seg[s].vec);
            }
            *reinterpret_cast<f4*>(Aq + r * SA + col) = v;
        }
    }
    for (int i = 0; i < NB_QT; ++i)
        rc_list_init(lists_s + (wave * NB_QT + i) * K, lists_i + (wave * NB_QT + i) * K, K, lane);
    __syncthreads();
    float thr0, thr1, thr2, thr3;
    nb_thresholds(lists_s + (wave * NB_QT + 4 * g) * K, K, a.nq - q0 - 4 * g, thr0, thr1, thr2, thr3);

    for (int ch = cb; ch < ce; ++ch) {
        const int row0 = ch * NB_CH + 16 * wave;
        if (row0 >= N) break;  // wave-uniform; no workgroup barrier inside the loop
        const int crow = row0 + it;
        const int64_t rr = crow < N ? crow : N - 1;  // loads stay inside the table
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* aq = Aq + it * SA + 4 * g;
        for (int s = 0; s < a.nseg; ++s) {
            const int d = a.seg[s].d, vec = a.seg[s].vec, T = a.seg[s].dp / 16;
            const float* __restrict__ row = prm + a.seg[s].off + rr * d;
            for (int t = 0; t < T; ++t) {
                const f4 b = nb_load4(row, 16 * t + 4 * g, d, vec);
                const f4 q = *reinterpret_cast<const f4*>(aq + 16 * t);
                acc = MFMA4(q.x, b.x, acc);
                acc = MFMA4(q.y, b.y, acc);
                acc = MFMA4(q.z, b.z, acc);
                acc = MFMA4(q.w, b.w, acc);
            }
            aq += a.seg[s].dp;
        }
        // lane (g, it), register r: query 4 g + r against catalogue row `it`
        if (a.cosine) {
            const float ic = a.inv[rr];
            acc.x = acc.x * invq[4 * g + 0] * ic;
            acc.y = acc.y * invq[4 * g + 1] * ic;
            acc.z = acc.z * invq[4 * g + 2] * ic;
            acc.w = acc.w * invq[4 * g + 3] * ic;
        }
        // a candidate enters a list only with score >= the list's last: four compares and
        // ballots reject the whole 16 x 16 tile in the common case
        const bool rowok = crow < N;
        const unsigned long long m0 = __ballot(rowok && acc.x >= thr0), m1 = __ballot(rowok && acc.y >= thr1),
                                 m2 = __ballot(rowok && acc.z >= thr2), m3 = __ballot(rowok && acc.w >= thr3);
        if ((m0 | m1 | m2 | m3) == 0) continue;  // wave-uniform
        const int cand = row0 + (lane & 15);
#pragma unroll 1
        for (int i = 0; i < NB_QT; ++i) {
            if (q0 + i >= a.nq) break;  // wave-uniform
            const unsigned long long mr = (i & 2) ? ((i & 1) ? m3 : m2) : ((i & 1) ? m1 : m0);
            if (((mr >> (16 * (i >> 2))) & 0xffffull) == 0) continue;  // wave-uniform
            const float s = __shfl(lane_get(acc, i & 3), 16 * (i >> 2) + (lane & 15), 64);
            const bool valid = lane < 16 && cand < N && !(a.exclude_self && cand == qid[i]);
            const int slot = wave * NB_QT + i;
            rc_feed(lists_s + slot * K, lists_i + slot * K, K, s, cand, valid, lane);
        }
        nb_thresholds(lists_s + (wave * NB_QT + 4 * g) * K, K, a.nq - q0 - 4 * g, thr0, thr1, thr2, thr3);
    }
    __syncthreads();

    // wave w merges, for its queries 4 w + r, the lists of the other waves into its own:
    // no list is written by one wave while another reads it
    for (int r = 0; r < 4; ++r) {
        const int i = 4 * wave + r;
        const int64_t q = q0 + i;
        if (q >= a.nq) break;  // wave-uniform
        volatile float* ls = lists_s + (wave * NB_QT + i) * K;
        volatile int* li = lists_i + (wave * NB_QT + i) * K;
        for (int w2 = 0; w2 < RC_WAVES; ++w2) {
            if (w2 == wave) continue;
            volatile float* ss = lists_s + (w2 * NB_QT + i) * K;
            volatile int* si = lists_i + (w2 * NB_QT + i) * K;
            for (int j0 = 0; j0 < K; j0 += 16) {
                const int j = j0 + lane;
                float sc = 0.f;
                int id = RC_IDMAX;
                if (lane < 16 && j < K) { sc = ss[j]; id = si[j]; }
                rc_feed(ls, li, K, sc, id, id != RC_IDMAX, lane);
            }
        }
        const int64_t o = (q * a.nsplit + split) * K;
        for (int j = lane; j < K; j += 64) {
            a.part_s[o + j] = ls[j];
            a.part_i[o + j] = li[j];
        }
    }
}

// Launch shape from the query count and the table: 16-query tiles, and as many chunk
// splits as bring the grid to about four workgroups per compute unit.
struct NbGeo {
    int nsplit, cps;
    int64_t tiles;
};
static NbGeo nb_geometry(int64_t nq, int N) {
    NbGeo G;
    G.tiles = (nq + NB_QT - 1) / NB_QT;
    const int64_t nchunks = ((int64_t)N + NB_CH - 1) / NB_CH;
    int64_t want = (1024 + G.tiles - 1) / G.tiles;
    if (want > nchunks) want = nchunks;
    if (want < 1) want = 1;
    G.cps = (int)((nchunks + want - 1) / want);
    G.nsplit = (int)((nchunks + G.cps - 1) / G.cps);
    return G;
}

struct NbWs {
    int64_t inv, ps, pid, total;
};
static NbWs nb_ws(int N, int64_t nq, int K, const NbGeo& G) {
    NbWs w;
    int64_t o = 0;
    w.inv = o; o += ws_align((int64_t)N * 4);
    w.ps = o; o += ws_align(nq * G.nsplit * K * 4);
    w.pid = o; o += ws_align(nq * G.nsplit * K * 4);
    w.total = o;
    return w;
}

static bool nb_valid(const ncf_layout* lay, int side, int space, int64_t nq, int K) {
    if (!lay || nq < 0 || K < 1 || K > RC_MAXK) return false;
    if (side != NCF_SIDE_USER && side != NCF_SIDE_ITEM) return false;
    if (space != NCF_SPACE_GMF && space != NCF_SPACE_MLP && space != NCF_SPACE_CONCAT) return false;
    if (lay->factor_num <= 0 || lay->num_layers < 1 || lay->num_layers > 4) return false;
    return (side == NCF_SIDE_ITEM ? lay->item_num : lay->user_num) > 0;
}

static int64_t nb_lds_bytes(int DP, int K) {
    return ((int64_t)NB_QT * (DP + 4) + 2 * RC_WAVES * NB_QT * K + 2 * NB_QT) * 4;
}

}  // namespace ncf

using namespace ncf;

extern "C" {

int64_t ncf_neighbors_workspace_bytes(const ncf_layout* lay, int side, int space, int64_t n_queries, int top_k) {
    if (!nb_valid(lay, side, space, n_queries, top_k)) return -1;
    if (n_queries == 0) return 0;
    const int N = side == NCF_SIDE_ITEM ? lay->item_num : lay->user_num;
    return nb_ws(N, n_queries, top_k, nb_geometry(n_queries, N)).total;
}

int ncf_neighbors(const ncf_layout* lay, const float* params, int side, int space, int metric, const int32_t* queries,
                  int64_t n_queries, int top_k, int exclude_self, int32_t* ids_out, float* scores_out, void* workspace,
                  int64_t workspace_bytes, void* stream) {
    if (!nb_valid(lay, side, space, n_queries, top_k)) return NCF_E_ARG;
    if (metric != NCF_SIM_COSINE && metric != NCF_SIM_DOT) return NCF_E_ARG;
    if (n_queries == 0) return NCF_OK;
    if (!params || !queries || !ids_out || !scores_out || !workspace) return NCF_E_ARG;
    const bool item = side == NCF_SIDE_ITEM;
    const int N = item ? lay->item_num : lay->user_num, K = top_k;
    const NbGeo G = nb_geometry(n_queries, N);
    const NbWs W = nb_ws(N, n_queries, K, G);
    if (workspace_bytes < W.total) return NCF_E_ARG;

    NbArgs a;
    memset(&a, 0, sizeof(a));
    const bool aligned = (reinterpret_cast<uintptr_t>(params) & 15) == 0;
    auto add = [&](int64_t off, int d) {
        NbSeg& s = a.seg[a.nseg++];
        s.off = off;
        s.d = d;
        s.dp = (d + 15) / 16 * 16;
        s.vec = aligned && d % 4 == 0 && off % 4 == 0;
        a.DP += s.dp;
    };
    if (space != NCF_SPACE_MLP) add(item ? lay->ig : lay->ug, lay->factor_num);
    if (space != NCF_SPACE_GMF) add(item ? lay->im : lay->um, lay->factor_num << (lay->num_layers - 1));
    const int64_t lds = nb_lds_bytes(a.DP, K);
    if (lds > LDS_LIMIT_BYTES) return NCF_E_UNSUPPORTED;
    if (lds > 64 * 1024 && ensure_lds(reinterpret_cast<const void*>(&nb_kernel), lds) != NCF_OK) return NCF_E_LAUNCH;
    char* ws = static_cast<char*>(workspace);
    a.params = params;
    a.queries = queries;
    a.nq = n_queries;
    a.N = N;
    a.K = K;
    a.cosine = metric == NCF_SIM_COSINE;
    a.exclude_self = exclude_self != 0;
    a.inv = reinterpret_cast<float*>(ws + W.inv);
    a.part_s = reinterpret_cast<float*>(ws + W.ps);
    a.part_i = reinterpret_cast<int32_t*>(ws + W.pid);
    a.nsplit = G.nsplit;
    a.cps = G.cps;

    hipStream_t st = (hipStream_t)stream;
    if (a.cosine) hipLaunchKernelGGL(nb_norm_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(nb_kernel, dim3((unsigned)G.tiles, (unsigned)G.nsplit), dim3(RC_WAVES * 64), (size_t)lds, st, a);
    launch_merge(a.part_s, a.part_i, n_queries, G.nsplit, K, ids_out, scores_out, st);
    return launch_status();
}

}  // extern "C"
