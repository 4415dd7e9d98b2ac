// Epoch preparation: row packing, the shuffle / group-by-item / canonical sort of an
// epoch's stream, the per-slice user order, and their C ABI (include/ncf_hip.h).
// gfx950 only.
#include "ncf_host.h"

namespace ncf {

// Packed rows (include/ncf_hip.h NCF_ROW_PACK): u | item << 32 | label << 63.
__device__ __forceinline__ int row_item(uint64_t r) { return (int)((r >> 32) & 0x7fffffffu); }

__global__ __launch_bounds__(256) void pack_rows_kernel(const int32_t* __restrict__ u, const int32_t* __restrict__ it,
                                                        const float* __restrict__ y, int64_t n, uint64_t* __restrict__ out) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        out[k] = NCF_ROW_PACK(u[k], it[k], y ? y[k] : 0.f);
}

__global__ __launch_bounds__(256) void gather_epoch_kernel(const uint64_t* __restrict__ rows,
                                                           const int64_t* __restrict__ perm, int64_t n,
                                                           uint64_t* __restrict__ out) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        out[k] = rows[perm[k]];
}

// ---------------------------------------------------------------------------
// Epoch preparation (ncf_prepare_epoch).  Global batch b is rows perm[b*B ..
// b*B+cnt) of the unshuffled stream (DataLoader shuffle=True membership); it is
// written back grouped by item.  Three launches, all HBM/L2-bound byte work:
//   1. shuffle_hist: shuf[j] = rows[perm[j]] (one random 8-byte gather per row,
//      coalesced write) and hist[b][item]++ (global atomics, no return).
//   2. scan_parts: per batch, hist -> exclusive item offsets in place, and the
//      batch is cut into P parts of ~cnt/P rows at item boundaries: part q owns
//      the items whose start offset s satisfies floor(s*P/cnt) == q, i.e. a
//      contiguous item range [I_q, I_q+1) and output region [R_q, R_q+1).
//   3. sort_part: one workgroup per (batch, part) streams the batch's shuffled
//      rows (L2-resident: the P parts of a batch run on one XCD), keeps those of
//      its items, places them by LDS atomics on the item offsets into an LDS
//      staging buffer and writes its region out contiguously.  Regions or item
//      ranges too large for LDS fall back to global offsets / direct writes.
constexpr int SH_THREADS = 256, SH_UNROLL = 8;
constexpr int SCAN_THREADS = 1024;
constexpr int SORT_THREADS = 1024, SORT_UNROLL = 8;
constexpr int STAGE_ROWS = 16384, ITEM_CAP = 6144;
constexpr int64_t SORT_LDS = (int64_t)STAGE_ROWS * 8 + (int64_t)ITEM_CAP * 4;
constexpr int PART_ROWS = 8192;  // nominal rows per part
constexpr int64_t PREP_GROUP_MIN = 4096;  // smaller global batches are shuffled, not grouped

__global__ __launch_bounds__(SH_THREADS) void shuffle_hist_kernel(const uint64_t* __restrict__ rows,
                                                                  const int64_t* __restrict__ perm, int64_t n,
                                                                  int64_t B, int item_num, uint64_t* __restrict__ shuf,
                                                                  int* __restrict__ hist) {
    const int64_t j0 = (int64_t)blockIdx.x * (SH_THREADS * SH_UNROLL) + threadIdx.x;
    int64_t src[SH_UNROLL];
    uint64_t r[SH_UNROLL];
#pragma unroll
    for (int k = 0; k < SH_UNROLL; ++k) {
        const int64_t j = j0 + k * SH_THREADS;
        const int64_t s = j < n ? perm[j] : 0;
        src[k] = s < 0 ? 0 : (s >= n ? n - 1 : s);
    }
#pragma unroll
    for (int k = 0; k < SH_UNROLL; ++k) r[k] = rows[src[k]];
#pragma unroll
    for (int k = 0; k < SH_UNROLL; ++k) {
        const int64_t j = j0 + k * SH_THREADS;
        if (j < n) {
            shuf[j] = r[k];
            atomicAdd(hist + (j / B) * item_num + min(row_item(r[k]), item_num - 1), 1);
        }
    }
}

// LDS-privatised variant for large batches: block (b, c) covers rows
// [b*B + c*SH_CHUNK, ...) of batch b only, counts its items in LDS and adds each
// non-zero bin to hist once -- no same-address atomic chains on hot items.
constexpr int SH2_THREADS = 1024, SH2_UNROLL = 8, SH_CHUNK = 16384;
constexpr int SH2_MAX_ITEMS = 32768;
__global__ __launch_bounds__(SH2_THREADS) void shuffle_hist_lds_kernel(const uint64_t* __restrict__ rows,
                                                                      const int64_t* __restrict__ perm, int64_t n,
                                                                      int64_t B, int item_num, int chunks,
                                                                      uint64_t* __restrict__ shuf,
                                                                      int* __restrict__ hist) {
    extern __shared__ int lh[];  // [item_num]
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / chunks;
    const int c = blockIdx.x - (int)(b * chunks);
    const int64_t b0 = b * B;
    const int cnt = (int)((n - b0) < B ? (n - b0) : B);
    const int r0 = c * SH_CHUNK, r1 = min(cnt, r0 + SH_CHUNK);
    if (r0 >= r1) return;  // block-uniform
    for (int i = tid; i < item_num; i += SH2_THREADS) lh[i] = 0;
    __syncthreads();
    for (int q0 = r0; q0 < r1; q0 += SH2_UNROLL * SH2_THREADS) {
        int64_t src[SH2_UNROLL];
        uint64_t r[SH2_UNROLL];
#pragma unroll
        for (int k = 0; k < SH2_UNROLL; ++k) {
            const int q = q0 + k * SH2_THREADS + tid;
            const int64_t s = q < r1 ? perm[b0 + q] : 0;
            src[k] = s < 0 ? 0 : (s >= n ? n - 1 : s);
        }
#pragma unroll
        for (int k = 0; k < SH2_UNROLL; ++k) r[k] = rows[src[k]];
#pragma unroll
        for (int k = 0; k < SH2_UNROLL; ++k) {
            const int q = q0 + k * SH2_THREADS + tid;
            if (q < r1) {
                shuf[b0 + q] = r[k];
                atomicAdd(&lh[min(row_item(r[k]), item_num - 1)], 1);
            }
        }
    }
    __syncthreads();
    int* h = hist + b * item_num;
    for (int i = tid; i < item_num; i += SH2_THREADS) {
        const int v = lh[i];
        if (v) atomicAdd(h + i, v);
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_parts_kernel(int* __restrict__ hist, int64_t n, int64_t B,
                                                                  int item_num, int P, int* __restrict__ parts) {
    __shared__ int wpart[SCAN_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t b0 = b * B;
    const int cnt = (int)((n - b0) < B ? (n - b0) : B);
    int* h = hist + b * item_num;
    int* pb = parts + b * (P + 1) * 2;
    const int per = (item_num + SCAN_THREADS - 1) / SCAN_THREADS;
    const int i0 = min(item_num, tid * per), i1 = min(item_num, i0 + per);
    int tot = 0;
    for (int i = i0; i < i1; ++i) tot += h[i];
    const int lane = tid & 63, wv = tid >> 6;
    int incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wpart[wv] = incl;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int q = 0; q < SCAN_THREADS / 64; ++q) {
            const int v = wpart[q];
            wpart[q] = acc;
            acc += v;
        }
        pb[0] = 0;
        pb[1] = 0;
    }
    __syncthreads();
    int s = wpart[wv] + incl - tot;
    // first part whose threshold T_q = ceil(q*cnt/P) lies above s
    int q = (int)((int64_t)s * P / cnt) + 1;
    for (int i = i0; i < i1; ++i) {
        const int c = h[i];
        h[i] = s;
        const int sn = s + c;
        while (q <= P) {
            const int T = (int)(((int64_t)q * cnt + P - 1) / P);
            if (T > sn) break;
            pb[2 * q] = i + 1;  // items [.., i] end before part q; item i + 1 starts it
            pb[2 * q + 1] = sn;
            ++q;
        }
        s = sn;
    }
}

// Canonical order of a batch's grouped rows (ncf_prepare_epoch2, NCF_PREP_CANONICAL):
// the LDS-atomic placement leaves the rows of one item in arrival order, which
// differs from run to run; data parallelism needs every rank's stream identical
// (rank r takes rows [r per, (r + 1) per) of each global batch), so with the flag
// each part is sorted by (item, user, label) -- a total order on the rows' values,
// identical duplicates being interchangeable -- which keeps the item grouping.
__device__ __forceinline__ uint64_t canon_key(uint64_t r) {
    return (((r >> 32) & 0x7fffffffull) << 33) | ((r & 0xffffffffull) << 1) | (r >> 63);
}
// Ascending sort of a[0 .. n) in place by canon_key, one workgroup (any n): the
// bitonic network in its all-ascending form (each merge stage starts with a flip
// comparison i <-> i ^ (k - 1), then half-cleaners i <-> i + j), so positions past
// n act as +infinity and are simply skipped.
template <int NT, class T>
__device__ void canon_sort(T* a, int n) {
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int q = threadIdx.x; q < (n2 >> 1); q += NT) {
                const int i = (q / j) * 2 * j + (q % j);
                const int p = j == (k >> 1) ? (i ^ (k - 1)) : i + j;  // flip, then half-cleaners
                if (p < n) {
                    const uint64_t x = a[i], y = a[p];
                    if (canon_key(x) > canon_key(y)) {
                        a[i] = y;
                        a[p] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(SORT_THREADS) void sort_part_kernel(const uint64_t* __restrict__ shuf,
                                                                 int* __restrict__ hist, const int* __restrict__ parts,
                                                                 int64_t n, int64_t B, int item_num, int P, int64_t nb,
                                                                 uint64_t* __restrict__ out, int canon) {
    extern __shared__ uint64_t stg[];                       // [STAGE_ROWS]
    int* loff = reinterpret_cast<int*>(stg + STAGE_ROWS);  // [ITEM_CAP]
    const int tid = threadIdx.x;
    const int x = blockIdx.x;
    int64_t b;
    int o;
    if (P >= 8) {  // the P parts of a batch share one XCD (blocks are dealt round-robin to the 8 XCDs)
        const int xcd = x & 7, k = x >> 3;
        b = (int64_t)(k / P) * 8 + xcd;
        o = k % P;
    } else {
        b = x / P;
        o = x % P;
    }
    if (b >= nb) return;
    const int64_t b0 = b * B;
    const int cnt = (int)((n - b0) < B ? (n - b0) : B);
    const int* pb = parts + b * (P + 1) * 2;
    const int ilo = pb[2 * o], rlo = pb[2 * o + 1], ihi = pb[2 * o + 2], rhi = pb[2 * o + 3];
    const int nrows = rhi - rlo, nit = ihi - ilo;
    if (nrows <= 0) return;  // block-uniform
    int* h = hist + b * item_num;
    const bool stage = nrows <= STAGE_ROWS, local = nit <= ITEM_CAP;
    if (local)
        for (int e = tid; e < nit; e += SORT_THREADS) loff[e] = h[ilo + e] - rlo;
    __syncthreads();
    const uint64_t* sb = shuf + b0;
    uint64_t* ob = out + b0 + rlo;
    for (int j0 = 0; j0 < cnt; j0 += SORT_UNROLL * SORT_THREADS) {
        uint64_t r[SORT_UNROLL];
#pragma unroll
        for (int k = 0; k < SORT_UNROLL; ++k) {
            const int j = j0 + k * SORT_THREADS + tid;
            r[k] = sb[j < cnt ? j : 0];
        }
#pragma unroll
        for (int k = 0; k < SORT_UNROLL; ++k) {
            const int j = j0 + k * SORT_THREADS + tid;
            const int it = min(row_item(r[k]), item_num - 1);
            if (j < cnt && it >= ilo && it < ihi) {
                const int pos = local ? atomicAdd(&loff[it - ilo], 1) : atomicAdd(&h[it], 1) - rlo;
                if (stage)
                    stg[pos] = r[k];
                else
                    ob[pos] = r[k];
            }
        }
    }
    if (stage) {
        __syncthreads();
        if (canon) canon_sort<SORT_THREADS>(stg, nrows);
        for (int e = tid; e < nrows; e += SORT_THREADS) ob[e] = stg[e];
    } else if (canon) {  // the region in place in global memory (a part beyond the LDS stage)
        __threadfence_block();
        __syncthreads();
        canon_sort<SORT_THREADS>(ob, nrows);
    }
}

// User order (ncf_user_order): one workgroup per rank slice of a batch, counting
// sort by user in LDS (histogram, exclusive scan, placement by LDS atomics).  The
// slice's rows are read twice (the second pass from L2); the entries are written
// inside the slice's own 8-byte-per-row window.
constexpr int UO_THREADS = 1024, UO_UNROLL = 16;
__device__ __forceinline__ int uo_bin(uint64_t rw, int user_num) {
    const int u = (int)(uint32_t)rw;
    return (u < 0 || u >= user_num) ? user_num : u;  // padding rows (-1) last
}
__global__ __launch_bounds__(UO_THREADS) void user_order_kernel(const uint64_t* __restrict__ rows, int64_t n,
                                                                int64_t B, int world, int user_num,
                                                                int64_t* __restrict__ order) {
    extern __shared__ int uh[];  // [user_num + 1]
    __shared__ int wsum[UO_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / world;
    const int r = (int)(blockIdx.x - b * world);
    const int64_t b0 = b * B;
    if (b0 >= n) return;  // block-uniform
    const int64_t cnt = (n - b0) < B ? (n - b0) : B;
    const int64_t per = (cnt + world - 1) / world;
    const int64_t lo = (int64_t)r * per;
    if (lo >= cnt) return;
    const int len = (int)((cnt - lo) < per ? (cnt - lo) : per);
    const uint64_t* rb = rows + b0 + lo;
    int64_t* ob = order + b0 + lo;
    int32_t* ib = reinterpret_cast<int32_t*>(order + n) + b0 + lo;  // inverse: row offset -> position
    const int nbin = user_num + 1;
    for (int i = tid; i < nbin; i += UO_THREADS) uh[i] = 0;
    __syncthreads();
    // rows in batches of UO_UNROLL per thread, loads issued together ahead of the LDS
    // atomics (one dependent load -> atomic per row was latency-bound: 160 us/epoch)
    for (int k0 = 0; k0 < len; k0 += UO_THREADS * UO_UNROLL) {
        int bins[UO_UNROLL];
#pragma unroll
        for (int q = 0; q < UO_UNROLL; ++q) {
            const int k = k0 + q * UO_THREADS + tid;
            bins[q] = k < len ? uo_bin(rb[k], user_num) : -1;
        }
#pragma unroll
        for (int q = 0; q < UO_UNROLL; ++q)
            if (bins[q] >= 0) atomicAdd(&uh[bins[q]], 1);
    }
    __syncthreads();
    const int chunk = (nbin + UO_THREADS - 1) / UO_THREADS;
    const int i0 = min(nbin, tid * chunk), i1 = min(nbin, i0 + chunk);
    int tot = 0;
    for (int i = i0; i < i1; ++i) tot += uh[i];
    const int lane = tid & 63, wv = tid >> 6;
    int incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int q = 0; q < UO_THREADS / 64; ++q) {
            const int v = wsum[q];
            wsum[q] = acc;
            acc += v;
        }
    }
    __syncthreads();
    int s = wsum[wv] + incl - tot;
    for (int i = i0; i < i1; ++i) {
        const int c = uh[i];
        uh[i] = s;
        s += c;
    }
    __syncthreads();
    for (int k0 = 0; k0 < len; k0 += UO_THREADS * UO_UNROLL) {
        int bins[UO_UNROLL];
#pragma unroll
        for (int q = 0; q < UO_UNROLL; ++q) {
            const int k = k0 + q * UO_THREADS + tid;
            bins[q] = k < len ? uo_bin(rb[k], user_num) : -1;
        }
#pragma unroll
        for (int q = 0; q < UO_UNROLL; ++q) {
            const int k = k0 + q * UO_THREADS + tid;
            if (bins[q] >= 0) {
                const int pos = atomicAdd(&uh[bins[q]], 1);
                ob[pos] = (int64_t)(((uint64_t)(uint32_t)(bins[q] < user_num ? bins[q] : -1) << 32) | (uint32_t)k);
                ib[k] = pos;
            }
        }
    }
}

static int prep_parts(int64_t B) {
    if (B <= PART_ROWS) return 1;
    const int64_t need = (B + PART_ROWS - 1) / PART_ROWS;
    int P = 1;
    while (P < need) P <<= 1;
    return P;
}

static int64_t al256(int64_t x) { return (x + 255) & ~(int64_t)255; }

}  // namespace ncf

using namespace ncf;

extern "C" {

int ncf_pack_rows(const int32_t* users, const int32_t* items, const float* labels, int64_t n, uint64_t* rows_out,
                  void* stream) {
    if (!users || !items || !rows_out || n < 0) return NCF_E_ARG;
    if (n == 0) return NCF_OK;
    int64_t grid = (n + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(pack_rows_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, users, items, labels, n,
                       rows_out);
    return launch_status();
}

int ncf_gather_epoch(const uint64_t* rows, const int64_t* perm, int64_t n, uint64_t* rows_out, void* stream) {
    if (!rows || !perm || !rows_out || n < 0) return NCF_E_ARG;
    if (n == 0) return NCF_OK;
    int64_t grid = (n + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(gather_epoch_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, rows, perm, n,
                       rows_out);
    return launch_status();
}

int64_t ncf_prepare_epoch_workspace(int64_t n, int64_t batch_global, int item_num) {
    if (n < 0 || batch_global <= 0 || item_num <= 0) return -1;
    if (batch_global < PREP_GROUP_MIN) return al256(8);  // plain shuffle: no histogram, no parts
    const int64_t nb = (n + batch_global - 1) / batch_global;
    const int P = prep_parts(batch_global);
    return al256(n * 8) + al256(nb * item_num * 4) + al256(nb * (P + 1) * 2 * 4);
}

int ncf_prepare_epoch(const uint64_t* rows, const int64_t* perm, int64_t n, int64_t batch_global, int item_num,
                      uint64_t* rows_out, void* workspace, int64_t workspace_bytes, void* stream) {
    return ncf_prepare_epoch2(rows, perm, n, batch_global, item_num, 0, rows_out, workspace, workspace_bytes, stream);
}

int ncf_prepare_epoch2(const uint64_t* rows, const int64_t* perm, int64_t n, int64_t batch_global, int item_num,
                       int flags, uint64_t* rows_out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!rows || !perm || !rows_out || !workspace || n < 0 || batch_global <= 0 || item_num <= 0) return NCF_E_ARG;
    if (flags & ~NCF_PREP_CANONICAL) return NCF_E_ARG;
    if (batch_global > 0x7fffffff) return NCF_E_ARG;
    if (workspace_bytes < ncf_prepare_epoch_workspace(n, batch_global, item_num)) return NCF_E_ARG;
    if (n == 0) return NCF_OK;
    hipStream_t st = (hipStream_t)stream;
    if (batch_global < PREP_GROUP_MIN) {  // small batches: item runs ~1 row, grouping buys nothing
        int64_t grid = (n + 255) / 256;
        if (grid > 8192) grid = 8192;
        hipLaunchKernelGGL(gather_epoch_kernel, dim3((int)grid), dim3(256), 0, st, rows, perm, n, rows_out);
        return launch_status();
    }
    const int64_t nb = (n + batch_global - 1) / batch_global;
    const int P = prep_parts(batch_global);
    char* ws = static_cast<char*>(workspace);
    uint64_t* shuf = reinterpret_cast<uint64_t*>(ws);
    int* hist = reinterpret_cast<int*>(ws + al256(n * 8));
    int* parts = reinterpret_cast<int*>(ws + al256(n * 8) + al256(nb * item_num * 4));
    if (hipMemsetAsync(hist, 0, (size_t)(nb * item_num * 4), st) != hipSuccess) return NCF_E_LAUNCH;
    if (item_num <= SH2_MAX_ITEMS && !(diag_flags() & DIAG_PREP_DIRECT)) {
        const int chunks = (int)((batch_global + SH_CHUNK - 1) / SH_CHUNK);
        const int64_t lds = (int64_t)item_num * 4;
        if (ensure_lds(reinterpret_cast<const void*>(&shuffle_hist_lds_kernel), lds) != NCF_OK) return NCF_E_LAUNCH;
        hipLaunchKernelGGL(shuffle_hist_lds_kernel, dim3((unsigned)(nb * chunks)), dim3(SH2_THREADS), (size_t)lds, st,
                           rows, perm, n, batch_global, item_num, chunks, shuf, hist);
    } else {
        const int64_t g1 = (n + SH_THREADS * SH_UNROLL - 1) / (SH_THREADS * SH_UNROLL);
        hipLaunchKernelGGL(shuffle_hist_kernel, dim3((unsigned)g1), dim3(SH_THREADS), 0, st, rows, perm, n,
                           batch_global, item_num, shuf, hist);
    }
    hipLaunchKernelGGL(scan_parts_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, st, hist, n, batch_global,
                       item_num, P, parts);
    if (ensure_lds(reinterpret_cast<const void*>(&sort_part_kernel), SORT_LDS) != NCF_OK) return NCF_E_LAUNCH;
    const int64_t g3 = P >= 8 ? ((nb + 7) / 8) * 8 * P : nb * P;
    hipLaunchKernelGGL(sort_part_kernel, dim3((unsigned)g3), dim3(SORT_THREADS), (size_t)SORT_LDS, st, shuf, hist,
                       parts, n, batch_global, item_num, P, nb, rows_out, (flags & NCF_PREP_CANONICAL) ? 1 : 0);
    return launch_status();
}

int ncf_user_order(const uint64_t* rows, int64_t n, int64_t batch_global, int world, int user_num, int64_t* order,
                   void* stream) {
    if (!rows || !order || n < 0 || batch_global <= 0 || world < 1 || user_num <= 0) return NCF_E_ARG;
    if (user_num > UO_MAX_USERS) return NCF_E_UNSUPPORTED;
    if (n == 0) return NCF_OK;
    const int64_t nb = (n + batch_global - 1) / batch_global;
    if (nb * world > 0x7fffffff) return NCF_E_ARG;
    const int64_t lds = (int64_t)(user_num + 1) * 4;
    if (ensure_lds(reinterpret_cast<const void*>(&user_order_kernel), lds) != NCF_OK) return NCF_E_LAUNCH;
    hipLaunchKernelGGL(user_order_kernel, dim3((unsigned)(nb * world)), dim3(UO_THREADS), (size_t)lds,
                       (hipStream_t)stream, rows, n, batch_global, world, user_num, order);
    return launch_status();
}

int ncf_uses_user_order(const ncf_layout* lay) {
    if (!lay) return 0;
    return ((fact_mode(lay) && !train_fused(lay) && lay->user_num <= UO_MAX_USERS) || us_on(lay)) ? 1 : 0;
}

}  // extern "C"
