// The block-tile GEMM cores of the layered kernels (ncf_layered.hip, ncf_chain_wide.inc)
// and nothing else: 256 threads = 4 waves, each wave a quadrant of the block tile, K
// through double-buffered LDS.
//
//   gemm_block_f32<Stage>  64 x 64, v_mfma_f32_16x16x4f32 (exact fp32), K in steps of 16;
//                          Stage = F32Scalar (any factor_num) or F32Vec4 (16-byte loads)
//   gemm_block_x6<TB>      64 x 64 or 128 x 128, fp32 on the bf16 matrix cores (three-plane
//                          split, six products), 16-byte loads, K in steps of 32
//   gemm_block_x6b         gemm_block_x6<64> with the B operand already split in memory
//   gemm_tile<TB>          what the 16-byte kernels call: the split core, or
//                          (-DNCF_GEMM_F32, the A/B library variant) the f32 core at TB 64
//
// Operand loaders: ga(mn, k) / gb(k, mn) return one element (F32Scalar) or four along the
// operand's contiguous dimension (KC: K, else M/N; a multiple of 4 with 16-byte aligned
// rows, factor_num % 4 == 0).  Every core ends in tile_each(acc, ..., ep).
#pragma once
#include <type_traits>

#include "ncf_common.h"

namespace ncf {

constexpr int GBM = 64, GBN = 64, GBK = 16, GNT = 256, GPAD = 4;

__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ f4 zero4() { return f4{0.f, 0.f, 0.f, 0.f}; }

// Store-time hook on the A operand (sa(value) once per loaded element or f4, when it is
// written to LDS -- the load has landed by then, so no extra wait): the weight
// gradient sums dY's columns through it for db_k.
struct NoHook {
    template <class T>
    __device__ __forceinline__ void operator()(const T&) const {}
};

// B-operand loaders take (k, mn): adapt to the A form (mn, k)
template <class G>
struct X6Swap {
    G g;
    __device__ __forceinline__ auto operator()(int mn, int64_t k) const { return g(k, mn); }
};

// The wave's accumulators, element by element.  A wave owns the NT x NT 16 x 16 MFMA
// tiles at (wm, wn) of the block tile; lane l's register r of acc[ti][tj] is row
// wm + 16 ti + 4 (l >> 4) + r, column wn + 16 tj + (l & 15) (C/D of the f32 16x16x4 and
// of the bf16 16x16x32 MFMA alike).  f(row, col, value) is called per element; or, where
// the epilogue hoists a per-column load (bias[n]), f(col) returns the per-row
// g(row, value).
template <int NT, class F>
__device__ __forceinline__ void tile_each(const f4 (&acc)[NT][NT], int wm, int wn, int l, F f) {
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
            const int col = wn + 16 * tj + (l & 15), row = wm + 16 * ti + 4 * (l >> 4);
            if constexpr (std::is_invocable_v<F, int, int, float>) {
#pragma unroll
                for (int r = 0; r < 4; ++r) f(row + r, col, lane_get(acc[ti][tj], r));
            } else {
                auto g = f(col);
#pragma unroll
                for (int r = 0; r < 4; ++r) g(row + r, lane_get(acc[ti][tj], r));
            }
        }
}

// ---------------------------------------------------------------------------
// The f32 core.  LDS tiles [2][16 k][64 + 4]; a Stage<KC> holds one thread's share of
// one operand's next K step between its load and its LDS store.
//
// F32Scalar: one element per pass.  KC: the operand is contiguous along K (16 lanes per
// row, 4 passes of 16 rows); otherwise contiguous along M/N (64 lanes per k, 4 passes of
// 4 k).
template <bool KC>
__device__ __forceinline__ int map_mn(int t, int p) { return KC ? (t >> 4) + 16 * p : (t & 63); }
template <bool KC>
__device__ __forceinline__ int map_k(int t, int p) { return KC ? (t & 15) : (t >> 6) + 4 * p; }

template <bool KC>
struct F32Scalar {
    float r[4];
    template <class G>
    __device__ __forceinline__ void load(G& g, int64_t k0, int t) {
#pragma unroll
        for (int p = 0; p < 4; ++p) r[p] = g(map_mn<KC>(t, p), k0 + map_k<KC>(t, p));
    }
    template <class SA>
    __device__ __forceinline__ void hook(SA& sa) const {
#pragma unroll
        for (int p = 0; p < 4; ++p) sa(r[p]);
    }
    __device__ __forceinline__ void store(float (*S)[GBM + GPAD], int t) const {
#pragma unroll
        for (int p = 0; p < 4; ++p) S[map_k<KC>(t, p)][map_mn<KC>(t, p)] = r[p];
    }
};
// F32Vec4: one 16-byte load per thread per K step.  KC tile [64][16]: thread t loads row
// t / 4, k 4 (t % 4) .. + 3; otherwise [16][64]: k t / 16, columns 4 (t % 16) .. + 3 (one
// LDS f4 store).
template <bool KC>
struct F32Vec4 {
    f4 r;
    __device__ __forceinline__ static int mn(int t) { return KC ? (t >> 2) : 4 * (t & 15); }
    __device__ __forceinline__ static int k(int t) { return KC ? 4 * (t & 3) : (t >> 4); }
    template <class G>
    __device__ __forceinline__ void load(G& g, int64_t k0, int t) { r = g(mn(t), k0 + k(t)); }
    template <class SA>
    __device__ __forceinline__ void hook(SA& sa) const { sa(r); }
    __device__ __forceinline__ void store(float (*S)[GBM + GPAD], int t) const {
        if constexpr (KC) {
#pragma unroll
            for (int i = 0; i < 4; ++i) S[k(t) + i][mn(t)] = lane_get(r, i);
        } else {
            *reinterpret_cast<f4*>(&S[k(t)][mn(t)]) = r;
        }
    }
};

template <template <bool> class Stage, bool AKC, bool BKC, class GA, class GB, class EP, class SA = NoHook>
__device__ __forceinline__ void gemm_block_f32(int64_t kbeg, int64_t kend, GA ga, GB gb, EP ep, SA sa = SA{}) {
    __shared__ __attribute__((aligned(16))) float As[2][GBK][GBM + GPAD];
    __shared__ __attribute__((aligned(16))) float Bs[2][GBK][GBN + GPAD];
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int wm = (w >> 1) * 32, wn = (w & 1) * 32;
    X6Swap<GB> gbs{gb};
    Stage<AKC> ra;
    Stage<BKC> rb;
    auto load = [&](int64_t k0) {
        ra.load(ga, k0, t);
        rb.load(gbs, k0, t);
    };
    auto store = [&](int buf) {
        ra.hook(sa);
        ra.store(As[buf], t);
        rb.store(Bs[buf], t);
    };
    f4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = zero4();
    load(kbeg);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int64_t k0 = kbeg; k0 < kend; k0 += GBK) {
        const bool more = k0 + GBK < kend;
        if (more) load(k0 + GBK);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int kk = 4 * s + (l >> 4);
            const float a0 = As[buf][kk][wm + (l & 15)], a1 = As[buf][kk][wm + 16 + (l & 15)];
            const float b0 = Bs[buf][kk][wn + (l & 15)], b1 = Bs[buf][kk][wn + 16 + (l & 15)];
            acc[0][0] = MFMA4(a0, b0, acc[0][0]);
            acc[0][1] = MFMA4(a0, b1, acc[0][1]);
            acc[1][0] = MFMA4(a1, b0, acc[1][0]);
            acc[1][1] = MFMA4(a1, b1, acc[1][1]);
        }
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    tile_each(acc, wm, wn, l, ep);
}

// ---------------------------------------------------------------------------
// fp32 GEMM on the bf16 matrix cores (three-plane split, six products).
//
// gfx950 runs v_mfma_f32_16x16x4_f32 at 1/16 of the bf16 rate and has no xf32.
// Every fp32 operand element is split exactly into three bf16 planes by
// round-to-nearest, x = h + m + l (h = bf16(x), m = bf16(x - h), l = x - h - m; each
// remainder is exact in fp32 and the last fits bf16, so the sum is exact), and
//   x * y ~= h h' + (h m' + m h') + (h l' + m m' + l h')
// drops only m l', l m', l l': |m| <= 2^-8 |x|, |l| <= 2^-16 |x|, so each is
// <= 2^-24 |x y| and, the residuals being signed, unbiased -- about one fp32
// rounding per product (a truncating split leaves 8x larger, same-sign terms:
// max 4.7e-7 against 5.9e-8 relative over 2M random pairs).
// Accumulated in fp32 by v_mfma_f32_16x16x32_bf16 (exact bf16 x bf16 products).
// Per K = 32: 6 bf16 MFMAs of 16 cycles against 8 f32 MFMAs of 32.
typedef short bf16x8 __attribute__((ext_vector_type(8)));
constexpr int XBK = 32;

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float bitsf(uint32_t u) { return __builtin_bit_cast(float, u); }
// (a, b) -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32), a in the low half
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
    const f2_t v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
// (x0, x1) -> three packed bf16 pairs (x0 in the low half): h, m, l with x = h + m + l
__device__ __forceinline__ void split3(float x0, float x1, uint32_t& h, uint32_t& m, uint32_t& l) {
    h = pk_bf16(x0, x1);
    const float r0 = x0 - bitsf(h << 16), r1 = x1 - bitsf(h & 0xffff0000u);
    m = pk_bf16(r0, r1);
    const float s0 = r0 - bitsf(m << 16), s1 = r1 - bitsf(m & 0xffff0000u);
    l = pk_bf16(s0, s1);
}
// eight values along K (x: the first four, y: the next four) -> the three bf16 planes of
// one MFMA operand fragment
__device__ __forceinline__ void x6_frag(const f4& x, const f4& y, bf16x8 (&f)[3]) {
    uint4 h, m, lo;
    split3(x.x, x.y, h.x, m.x, lo.x);
    split3(x.z, x.w, h.y, m.y, lo.y);
    split3(y.x, y.y, h.z, m.z, lo.z);
    split3(y.z, y.w, h.w, m.w, lo.w);
    f[0] = __builtin_bit_cast(bf16x8, h);
    f[1] = __builtin_bit_cast(bf16x8, m);
    f[2] = __builtin_bit_cast(bf16x8, lo);
}
// c += a b: the six products, smallest terms first
__device__ __forceinline__ f4 x6_mma(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
}

// The split happens in registers: the LDS holds the fp32 tiles ([mn][k], 32 k per row,
// 4-float chunks XOR-swizzled by (r ^ r >> 3) & 7: conflict-free ds_read_b128 operand
// reads and 16-byte stores, 2-way dword stores); each wave reads its fragments (two
// ds_read_b128 per 16-row tile) and splits them before its MFMAs.  (A variant that split
// once per block into three bf16 plane images in LDS -- 48 KB per block, 3 blocks per
// CU -- measured slower: stress 1304 against 1093 us per step.)
__device__ __forceinline__ int x6s_addr(int r, int k) { return r * XBK + 4 * ((k >> 2) ^ ((r ^ (r >> 3)) & 7)) + (k & 3); }

// One operand's TB x 32 tile of a K step: TB / 32 16-byte loads per thread, then its LDS
// stores.  (A register-transposed store for !KC -- four consecutive k rows per thread
// stored as f4 along k -- removed the weight-gradient launch's 17M LDS bank-conflict
// cycles but ran 164.5 -> 194.8 us: profiles/r06_evidence/gemm_tile_ab/.)
template <bool KC, int TB, class G>
__device__ __forceinline__ void x6_load(G g, int64_t k0, int t, f4 (&v)[TB / 32]) {
#pragma unroll
    for (int h = 0; h < TB / 32; ++h) {
        const int q = t + 256 * h;
        v[h] = KC ? g(q >> 3, k0 + 4 * (q & 7)) : g(4 * (q % (TB / 4)), k0 + q / (TB / 4));
    }
}
template <bool KC, int TB>
__device__ __forceinline__ void x6_store(float* S, int t, const f4 (&v)[TB / 32]) {
#pragma unroll
    for (int h = 0; h < TB / 32; ++h) {
        const int q = t + 256 * h;
        if constexpr (KC) {
            *reinterpret_cast<f4*>(S + x6s_addr(q >> 3, 4 * (q & 7))) = v[h];
        } else {
            const int k = q / (TB / 4), mn = 4 * (q % (TB / 4));
#pragma unroll
            for (int i = 0; i < 4; ++i) S[x6s_addr(mn + i, k)] = lane_get(v[h], i);
        }
    }
}
// lane l's 8 k of row r (k 8 (l >> 4) .. + 7) -> the three bf16 planes of its fragment
__device__ __forceinline__ void x6s_frag(const float* S, int r, int l, bf16x8 (&f)[3]) {
    const int k = 8 * (l >> 4);
    x6_frag(ld4(S + x6s_addr(r, k)), ld4(S + x6s_addr(r, k + 4)), f);
}

// gemm_block_x6<TB>: the split core on a TB x TB block tile, each of the 4 waves a
// TB / 2 quadrant (NT x NT MFMA tiles, NT = TB / 32), with gemm_block_f32<F32Vec4>'s
// contract (loaders, store hook, tile_each).  TB = 64 was the first form; per K step
// its waves split 4 fragments (three bf16 planes each, ~40 VALU per fragment) for 24
// MFMAs, and a wave64 VALU instruction occupies the SIMD 4 cycles -- ~960 VALU cycles
// against 384 MFMA cycles, so the split sets the time (SQ: 10 VALU per MFMA instruction
// in the weight-gradient launch, MFMA busy 0.21).  At TB = 128 a wave splits 8 fragments
// for 96 MFMAs.  Each output element has the same planes, products, product order and
// K order at either TB (bitwise the same outputs for the same K range).
// LDS: 2 x (TB + TB) x 32 fp32 -- 32 KB static at TB = 64; 64 KB at TB = X6W_TB, dynamic
// (X6W_LDS bytes; launchers set the attribute, x6w_ready).
constexpr int X6W_TB = 128;
constexpr int X6W_LDS = 2 * 2 * X6W_TB * XBK * 4;

template <int TB>
__device__ __forceinline__ float* x6_lds() {
    if constexpr (TB == X6W_TB) {
        extern __shared__ __attribute__((aligned(16))) float x6w_sm[];
        return x6w_sm;
    } else {
        __shared__ __attribute__((aligned(16))) float x6_sm[2 * 2 * TB * XBK];
        return x6_sm;
    }
}

template <int TB, bool AKC, bool BKC, class GA, class GB, class EP, class SA = NoHook>
__device__ __forceinline__ void gemm_block_x6(int64_t kbeg, int64_t kend, GA ga4, GB gb4, EP ep, SA sa = SA{}) {
    static_assert(TB == 64 || TB == X6W_TB, "block tile");
    constexpr int NT = TB / 32;
    float* As = x6_lds<TB>();           // [2][TB * XBK]
    float* Bs = As + 2 * TB * XBK;      // [2][TB * XBK]
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int wm = (w >> 1) * (TB / 2), wn = (w & 1) * (TB / 2);
    const X6Swap<GB> gbs{gb4};
    f4 ra[NT], rb[NT];
    auto load = [&](int64_t k0) {
        x6_load<AKC, TB>(ga4, k0, t, ra);
        x6_load<BKC, TB>(gbs, k0, t, rb);
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int h = 0; h < NT; ++h) sa(ra[h]);
        x6_store<AKC, TB>(As + buf * TB * XBK, t, ra);
        x6_store<BKC, TB>(Bs + buf * TB * XBK, t, rb);
    };
    f4 acc[NT][NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = zero4();
    load(kbeg);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int64_t k0 = kbeg; k0 < kend; k0 += XBK) {
        const bool more = k0 + XBK < kend;
        if (more) load(k0 + XBK);
        bf16x8 fa[NT][3];
#pragma unroll
        for (int i = 0; i < NT; ++i) x6s_frag(As + buf * TB * XBK, wm + 16 * i + (l & 15), l, fa[i]);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            bf16x8 fb[3];
            x6s_frag(Bs + buf * TB * XBK, wn + 16 * j + (l & 15), l, fb);
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i][j] = x6_mma(fa[i], fb, acc[i][j]);
        }
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    tile_each(acc, wm, wn, l, ep);
}

// gemm_block_x6b: gemm_block_x6<64> with the B operand already split: bimg is the
// block's first 16-column group of a fragment-major image (lyr_wc_prep_kernel's W0
// images: per 16-column group ngs bytes, per K step of 32 three planes x 64 lanes x
// 16 B), read straight from memory (L2-resident, 1.5 MB per image) one K step ahead.
// Only A passes through LDS and the split, so a wave splits 2 fragments per 24 MFMAs
// instead of 4 (the weight operand is split once per step instead of once per block).
// Same planes, products and K order per element as gemm_block_x6.
template <bool AKC, class GA, class EP>
__device__ __forceinline__ void gemm_block_x6b(int64_t kbeg, int64_t kend, GA ga4, const char* __restrict__ bimg,
                                               int64_t ngs, EP ep) {
    constexpr int TB = 64, NT = TB / 32;
    __shared__ __attribute__((aligned(16))) float As[2 * TB * XBK];
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int wm = (w >> 1) * (TB / 2), wn = (w & 1) * (TB / 2);
    f4 ra[NT];
    bf16x8 fb[NT][3], fn[NT][3];  // this K step's B fragments, the next one's
    auto load = [&](int64_t k0) {
        x6_load<AKC, TB>(ga4, k0, t, ra);
        const char* p = bimg + (k0 / XBK) * 3072 + l * 16;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 3; ++q)
                fn[j][q] = *reinterpret_cast<const bf16x8*>(p + (int64_t)(wn / 16 + j) * ngs + q * 1024);
    };
    auto store = [&](int buf) {
        x6_store<AKC, TB>(As + buf * TB * XBK, t, ra);
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 3; ++q) fb[j][q] = fn[j][q];
    };
    f4 acc[NT][NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = zero4();
    load(kbeg);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int64_t k0 = kbeg; k0 < kend; k0 += XBK) {
        const bool more = k0 + XBK < kend;
        if (more) load(k0 + XBK);
        bf16x8 fa[NT][3];
#pragma unroll
        for (int i = 0; i < NT; ++i) x6s_frag(As + buf * TB * XBK, wm + 16 * i + (l & 15), l, fa[i]);
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i][j] = x6_mma(fa[i], fb[j], acc[i][j]);
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    tile_each(acc, wm, wn, l, ep);
}

// The GEMM core of the layered kernels' 16-byte loader path
template <int TB, bool AKC, bool BKC, class GA, class GB, class EP, class SA = NoHook>
__device__ __forceinline__ void gemm_tile(int64_t kbeg, int64_t kend, GA ga4, GB gb4, EP ep, SA sa = SA{}) {
#if defined(NCF_GEMM_F32)
    constexpr bool F32 = TB == 64;
#else
    constexpr bool F32 = false;
#endif
    if constexpr (F32)
        gemm_block_f32<F32Vec4, AKC, BKC>(kbeg, kend, ga4, gb4, ep, sa);
    else
        gemm_block_x6<TB, AKC, BKC>(kbeg, kend, ga4, gb4, ep, sa);
}

}  // namespace ncf
