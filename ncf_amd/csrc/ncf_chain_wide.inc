// Wide step chain (training, factored layer 0, dm = 512 with L = 4: NCF(64,4), the
// stress shape of SURVEY.md §8 / BASELINE.json configs[...]): the tower's forward,
// predict, BCE and data gradients for a tile of 128 rows in ONE launch, with every
// activation and data gradient kept in registers and the tower weights streamed
// through LDS.  Included by ncf_layered.hip (inside its anonymous namespace, after
// the predict kernel): it replaces lyr_fwd0_fact_kernel, the three lyr_fwd_kernel,
// lyr_predict_kernel and the three lyr_bwd_data_kernel launches of the per-layer
// path (reference: src/ncf/models.py:97-118 forward, scripts/train_neumf.py:112-114
// loss and backward) and writes exactly what the per-layer path leaves for the
// weight gradients and the layer-0 scatter (ChainBufs: H_1 .. H_{L-1}, D_0 .. D_{L-1}).
//
// Orientation.  Every layer is computed transposed, Out^T = W In^T, on
// v_mfma_f32_16x16x32_bf16: the A operand is the weight tile (16 output features x
// 32 K), the B operand the wave's 16 rows (32 K x 16 rows), so a lane (row c = l&15,
// group g = l>>4) ends a layer holding features 16 mt + 4 g .. + 3 of its row for each
// output tile mt -- which is directly the next layer's B operand once the K order of a
// 32-wide K step s is taken as {32 s + 4 g .. + 3, 32 s + 16 + 4 g .. + 3} for lane
// group g (tiles 2 s and 2 s + 1).  The weights are staged in that permuted order, so
// no activation ever goes through LDS.
//
// Precision.  fp32 products on the bf16 cores by the exact three-plane split of
// ncf_gemm.h (x6_frag, x6_mma): x = h + m + l, six products per pair, smallest
// terms first.  The weights are split once per staged chunk (per tile), the
// activations once per K step (per wave) and reused across the K step's 16 tiles.
//
// Staging.  The weight stream of a tile is a fixed sequence of 42 chunks of 48 KB: a
// chunk is nks K steps (32 wide) x mt output tiles with nks mt = 16, as three bf16
// planes [K step][plane][tile][lane] x 16 B, so each operand read is one conflict-free
// ds_read_b128 per plane:
//   fwd L1 16 x (1, 16), fwd L2 4 x (2, 8), fwd L3 (4, 4), bwd L3 (2, 8), bwd L2 4 x
//   (1, 16), bwd L1 2 x 8 x (1, 16)   (dm 512, L 4).
// lyr_wc_prep_kernel writes the 42 images once per step (2 MB, split and permuted
// from the current W_1 .. W_3); the chain copies chunk i + 1 into the other LDS buffer
// by global_load_lds (lane-linear, no registers, no split work) while it multiplies
// chunk i, one workgroup barrier per chunk.  The sequence runs on across the block's
// tiles.
namespace wc {

constexpr int NT = 512;                 // 8 waves
constexpr int ROWS = 128;               // 16 rows per wave
constexpr int CHUNK = 48 * 1024;        // bytes per chunk image / LDS buffer
constexpr int DM = 512, L = 4, F = DM >> (L - 1), TF = F / 16;
constexpr int S(int k) { return (2 * DM) >> k; }  // S(1) = DM .. S(L) = F

// the per-tile chunk schedule: phase i = (bwd, layer k, first output feature m0,
// tiles mt, K steps per chunk nks, chunks n); nks mt = 16 for every chunk
struct Phase { int bwd, k, m0, mt, nks, n; };
constexpr int NPH = 7, NCH = 16 + 4 + 1 + 1 + 4 + 8 + 8;  // 42 chunks per tile
__host__ __device__ constexpr Phase phase(int i) {
    return i == 0 ? Phase{0, 1, 0, 16, 1, 16}
         : i == 1 ? Phase{0, 2, 0, 8, 2, 4}
         : i == 2 ? Phase{0, 3, 0, 4, 4, 1}
         : i == 3 ? Phase{1, 3, 0, 8, 2, 1}
         : i == 4 ? Phase{1, 2, 0, 16, 1, 4}
         : i == 5 ? Phase{1, 1, 0, 16, 1, 8}
                  : Phase{1, 1, 256, 16, 1, 8};
}
constexpr int PREP_THREADS = NCH * 16 * 64;  // one thread per (chunk, K step x tile, lane)
// W0 as the pre-split B operand of the projection and the dX expansion (gemm_block_x6b):
// four images (projection users / items, dX users / items), each [n group of 16][K step
// of 32][plane][lane] x 16 B -- lane l of (ng, ks) holds B[32 ks + 8 (l >> 4) .. + 7]
// [16 ng + (l & 15)] (x6s_frag's K order, ncf_gemm.h)
constexpr int W0_NG = DM / 16, W0_KS = DM / 32;
constexpr int64_t W0_NG_BYTES = (int64_t)W0_KS * 3 * 1024;          // one n group
constexpr int64_t W0_IMG_BYTES = (int64_t)W0_NG * W0_NG_BYTES;      // one image (1.5 MB)
constexpr int W0_PREP_THREADS = 4 * W0_NG * W0_KS * 64;

// byte offset of (K step ksl, plane p, tile t) inside a chunk of mt tiles
__host__ __device__ constexpr int img_off(int mt, int ksl, int p, int t) { return ((ksl * 3 + p) * mt + t) * 1024; }

// copy stream chunk `local`'s image into an LDS buffer: 48 slices of 1 KB, six per
// wave, lane-linear (global_load_lds_dwordx4: base + lane x 16 B)
__device__ __forceinline__ void stage(const char* img, int local, char* lds, int w, int l) {
    const char* src = img + (int64_t)local * CHUNK + l * 16;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int j = w * 6 + i;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + j * 1024),
                                         (__attribute__((address_space(3))) void*)(lds + j * 1024), 16, 0, 0);
    }
}

// acc[mt] += A(tile mt of the K step at `buf`) B for the wave's 16 rows, six products
// smallest first
template <int MT>
__device__ __forceinline__ void kstep(const char* buf, int l, const bf16x8 (&b)[3], f4 (&acc)[MT]) {
    const char* p = buf + l * 16;
    // tile mt + 1's three planes are requested ahead of tile mt's six products; the
    // scheduling barrier keeps the compiler from hoisting every tile's reads (registers)
    bf16x8 fa[2][3];
    auto rd = [&](int mt, bf16x8 (&f)[3]) {
#pragma unroll
        for (int q = 0; q < 3; ++q) f[q] = *reinterpret_cast<const bf16x8*>(p + (q * MT + mt) * 1024);
    };
    rd(0, fa[0]);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (mt + 1 < MT) rd(mt + 1, fa[(mt + 1) & 1]);
        acc[mt] = x6_mma(fa[mt & 1], b, acc[mt]);
        if (mt + 1 < MT) __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// a[i] = a[i + 2] (cyclic): the next K step's two tiles to the front
template <int N>
__device__ __forceinline__ void rotate2(f4 (&v)[N]) {
    const f4 t0 = v[0], t1 = v[1];
#pragma unroll
    for (int i = 0; i + 2 < N; ++i) v[i] = v[i + 2];
    v[N - 2] = t0;
    v[N - 1] = t1;
}

__device__ __forceinline__ f4 relu_bias(const f4& v, const float* b) {
    const f4 bb = *reinterpret_cast<const f4*>(b);
    return f4{fmaxf(v.x + bb.x, 0.f), fmaxf(v.y + bb.y, 0.f), fmaxf(v.z + bb.z, 0.f), fmaxf(v.w + bb.w, 0.f)};
}
__device__ __forceinline__ uint32_t pos_bits(const f4& v) {
    return (v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u);
}
__device__ __forceinline__ f4 masked(const f4& v, uint32_t bits4) {
    return f4{(bits4 & 1u) ? v.x : 0.f, (bits4 & 2u) ? v.y : 0.f, (bits4 & 4u) ? v.z : 0.f, (bits4 & 8u) ? v.w : 0.f};
}

}  // namespace wc

// The step's 42 weight chunk images from the current W_1 .. W_3 (after the previous
// step's Adam): thread = (chunk, K step x tile pair, lane); its 8 permuted-K values of
// output row m split into the three bf16 planes, one 16-byte store per plane.
// Threads past PREP_THREADS write the four W0 images (w0img, may be null) in the same pass.
__global__ __launch_bounds__(256) void lyr_wc_prep_kernel(const float* __restrict__ prm, ncf_layout lay,
                                                          char* __restrict__ img, char* __restrict__ w0img) {
    using namespace wc;
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= PREP_THREADS) {
        const int q = gid - PREP_THREADS;
        if (w0img == nullptr || q >= W0_PREP_THREADS) return;
        const int lane = q & 63, ks = (q >> 6) % W0_KS, ng = (q >> 6) / W0_KS % W0_NG, use = (q >> 6) / (W0_KS * W0_NG);
        const int n = 16 * ng + (lane & 15), k0 = 32 * ks + 8 * (lane >> 4);
        const float* W0 = prm + lay.w[0];  // [DM][2 DM]
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + e;
            v[e] = use == 0 ? W0[(int64_t)n * 2 * DM + k]          // projection, users: W0[n][k]
                 : use == 1 ? W0[(int64_t)n * 2 * DM + DM + k]     // items: W0[n][DM + k]
                 : use == 2 ? W0[(int64_t)k * 2 * DM + n]          // dX, users: W0[k][n]
                            : W0[(int64_t)k * 2 * DM + DM + n];    // items: W0[k][DM + n]
        }
        uint4 h, mm, lo;
        split3(v[0], v[1], h.x, mm.x, lo.x);
        split3(v[2], v[3], h.y, mm.y, lo.y);
        split3(v[4], v[5], h.z, mm.z, lo.z);
        split3(v[6], v[7], h.w, mm.w, lo.w);
        char* dst = w0img + use * W0_IMG_BYTES + ng * W0_NG_BYTES + (int64_t)ks * 3072 + lane * 16;
        *reinterpret_cast<uint4*>(dst) = h;
        *reinterpret_cast<uint4*>(dst + 1024) = mm;
        *reinterpret_cast<uint4*>(dst + 2048) = lo;
        return;
    }
    const int lane = gid & 63, pi = (gid >> 6) & 15, chunk = gid >> 10;
    int loc = chunk, ip = 0;
    while (ip + 1 < NPH && loc >= phase(ip).n) loc -= phase(ip++).n;
    const Phase ph = phase(ip);
    const int ksl = pi / ph.mt, t = pi - ksl * ph.mt;
    const int s = loc * ph.nks + ksl;  // K step within the layer
    const int r = lane & 15, g = lane >> 4;
    const int m = ph.m0 + 16 * t + r, in = S(ph.k);
    const float* W = prm + lay.w[ph.k];  // [S(k+1)][S(k)]
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int kk = 32 * s + (e < 4 ? 4 * g + e : 12 + 4 * g + e);
        v[e] = ph.bwd ? W[(int64_t)kk * in + m] : W[(int64_t)m * in + kk];
    }
    uint4 h, mm, lo;
    split3(v[0], v[1], h.x, mm.x, lo.x);
    split3(v[2], v[3], h.y, mm.y, lo.y);
    split3(v[4], v[5], h.z, mm.z, lo.z);
    split3(v[6], v[7], h.w, mm.w, lo.w);
    char* dst = img + (int64_t)chunk * CHUNK + lane * 16;
    *reinterpret_cast<uint4*>(dst + img_off(ph.mt, ksl, 0, t)) = h;
    *reinterpret_cast<uint4*>(dst + img_off(ph.mt, ksl, 1, t)) = mm;
    *reinterpret_cast<uint4*>(dst + img_off(ph.mt, ksl, 2, t)) = lo;
}

template <bool BPR = false>  // BPR: the pairwise (NCF_DZ_BPR) instantiation
__global__ __launch_bounds__(wc::NT) void lyr_wide_chain_kernel(LyrArgs a, const float* __restrict__ P, ChainBufs o,
                                                                const char* __restrict__ img, int64_t R) {
    using namespace wc;
    extern __shared__ __attribute__((aligned(16))) char wsm[];  // two chunk buffers
    __shared__ __attribute__((aligned(16))) float sBias[DM + DM / 2 + DM / 4 + DM / 8];  // b_0 .. b_3
    __shared__ __attribute__((aligned(16))) float sWP[2][F];  // wp: GMF part, tower part
    __shared__ float sIg[8][16][F + 1];  // per wave: GMF item-gradient rows
    __shared__ int sIt[8][16];           // per wave: item id per row (-1: none)
    __shared__ float sred[2 * F + 2];    // block sums: dwp GMF | dwp tower | dbp | loss
    constexpr int BO1 = DM, BO2 = DM + DM / 2, BO3 = DM + DM / 2 + DM / 4;  // b_1 .. b_3 in sBias
    const Sel s = select_rows(a);
    const ncf_layout& lay = a.lay;
    const float* prm = a.params;
    const bool gmf = lay.model_type != NCF_MODEL_MLP;
    const int Pg = gmf ? F : 0;
    const int t = threadIdx.x, l = t & 63, w = t >> 6, c = l & 15, g = l >> 4;
    if (blockIdx.x == 0 && t == 0) {  // step snapshot for ncf_reduce_adam_step
        a.ctl->snap_batch = a.ctl->batch;
        a.ctl->snap_t = a.ctl->adam_t + 1;
    }
    const int64_t ntile = (R + ROWS - 1) / ROWS;
    const int64_t my_tiles = (int64_t)blockIdx.x < ntile ? (ntile - 1 - blockIdx.x) / gridDim.x + 1 : 0;
    const int64_t total = my_tiles * NCH;
    auto buf = [&](int64_t i) -> char* { return wsm + (int)(i & 1) * CHUNK; };  // chunk buffer of stream chunk i
    // stream prologue: chunk 0 into buffer 0 (waited for at the barrier below)
    if (total > 0) stage(img, 0, buf(0), w, l);
    for (int e = t; e < DM + DM / 2 + DM / 4 + DM / 8; e += NT) {
        sBias[e] = e < BO1 ? prm[lay.b[0] + e]
                 : e < BO2 ? prm[lay.b[1] + (e - BO1)]
                 : e < BO3 ? prm[lay.b[2] + (e - BO2)] : prm[lay.b[3] + (e - BO3)];
    }
    for (int e = t; e < F; e += NT) {
        sWP[0][e] = gmf ? prm[lay.wp + e] : 0.f;
        sWP[1][e] = prm[lay.wp + Pg + e];
    }
    for (int e = t; e < 2 * F + 2; e += NT) sred[e] = 0.f;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const float bp = prm[lay.bp];
    int64_t cid = 0;  // chunk of the block's stream being multiplied
    // a chunk: WC_BEGIN copies the next chunk into the other buffer (global_load_lds),
    // the phase multiplies this one, WC_END waits for the copy and joins the workgroup
#define WC_BEGIN() \
    do { if (cid + 1 < total) stage(img, (int)((cid + 1) % NCH), buf(cid + 1), w, l); } while (0)
#define WC_END()                                          \
    do {                                                  \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  \
        __syncthreads();                                  \
        ++cid;                                            \
    } while (0)
    float aB = 0.f, aL = 0.f;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t m = tile * ROWS + 16 * w + c;  // this lane's row
        const uint64_t rw = m < s.nloc ? a.rows[s.base + m] : ~0ull;
        int u = (int)(uint32_t)rw, it = (int)((rw >> 32) & 0x7fffffffu);
        const bool valid = u >= 0 && m < R;  // padding rows gather id 0 and get dz = 0
        if (u < 0) u = it = 0;
        const bool st = m < R;
        const float* pu = P + (int64_t)u * DM;
        const float* pi = P + ((int64_t)lay.user_num + it) * DM;
        // ---- fwd layer 1 (512 -> 256): H_1 = ReLU(P[u] + P[U + i] + b_0) built per K step.
        // The K-step loops stay rolled (one body per phase keeps the code in the
        // instruction cache); register arrays are consumed from the front and rotated.
        // H_1 > 0 bits shift in 8 per K step: K step s, half h, value r at bit
        // 8 (15 - s) + 4 h + r of mb[0..3] (mb[0] lowest).
        uint32_t mb0 = 0u, mb1 = 0u, mb2 = 0u, mb3 = 0u;
        f4 h2[16];
        {
            f4 acc[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = zero4();
            f4 nx0 = ld4(pu + 4 * g), nx1 = ld4(pu + 16 + 4 * g), nx2 = ld4(pi + 4 * g), nx3 = ld4(pi + 16 + 4 * g);
#pragma unroll 1
            for (int ks = 0; ks < DM / 32; ++ks) {
                WC_BEGIN();
                const f4 cu0 = nx0, cu1 = nx1, ci0 = nx2, ci1 = nx3;
                if (ks + 1 < DM / 32) {  // the next K step's operands
                    const int j = 32 * (ks + 1) + 4 * g;
                    nx0 = ld4(pu + j);
                    nx1 = ld4(pu + j + 16);
                    nx2 = ld4(pi + j);
                    nx3 = ld4(pi + j + 16);
                }
                const int j0 = 32 * ks + 4 * g, j1 = j0 + 16;
                const f4 x = relu_bias(f4{cu0.x + ci0.x, cu0.y + ci0.y, cu0.z + ci0.z, cu0.w + ci0.w}, sBias + j0);
                const f4 y = relu_bias(f4{cu1.x + ci1.x, cu1.y + ci1.y, cu1.z + ci1.z, cu1.w + ci1.w}, sBias + j1);
                if (st) {
                    *reinterpret_cast<f4*>(o.H[1] + m * DM + j0) = x;
                    *reinterpret_cast<f4*>(o.H[1] + m * DM + j1) = y;
                }
                mb3 = (mb3 << 8) | (mb2 >> 24);
                mb2 = (mb2 << 8) | (mb1 >> 24);
                mb1 = (mb1 << 8) | (mb0 >> 24);
                mb0 = (mb0 << 8) | pos_bits(x) | (pos_bits(y) << 4);
                bf16x8 bf[3];
                x6_frag(x, y, bf);
                kstep<16>(buf(cid), l, bf, acc);
                WC_END();
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) h2[q] = relu_bias(acc[q], sBias + BO1 + 16 * q + 4 * g);
        }
        uint32_t m2lo = 0u, m2hi = 0u;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (st) *reinterpret_cast<f4*>(o.H[2] + m * S(2) + 16 * q + 4 * g) = h2[q];
            if (q < 8) m2lo |= pos_bits(h2[q]) << (4 * q);
            else m2hi |= pos_bits(h2[q]) << (4 * (q - 8));
        }
        // ---- fwd layer 2 (256 -> 128)
        f4 h3[8];
        {
            f4 acc[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = zero4();
#pragma unroll 1
            for (int ch = 0; ch < 4; ++ch) {
                WC_BEGIN();
#pragma unroll 1
                for (int ksl = 0; ksl < 2; ++ksl) {
                    bf16x8 bf[3];
                    x6_frag(h2[0], h2[1], bf);
                    rotate2(h2);
                    kstep<8>(buf(cid) + img_off(8, ksl, 0, 0), l, bf, acc);
                }
                WC_END();
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) h3[q] = relu_bias(acc[q], sBias + BO2 + 16 * q + 4 * g);
        }
        uint32_t m3 = 0u;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (st) *reinterpret_cast<f4*>(o.H[3] + m * S(3) + 16 * q + 4 * g) = h3[q];
            m3 |= pos_bits(h3[q]) << (4 * q);
        }
        // ---- fwd layer 3 (128 -> 64); the GMF rows requested first
        f4 ug[TF], ig[TF];
#pragma unroll
        for (int q = 0; q < TF; ++q) {
            const int j0 = 16 * q + 4 * g;
            ug[q] = gmf ? ld4(prm + lay.ug + (int64_t)u * F + j0) : zero4();
            ig[q] = gmf ? ld4(prm + lay.ig + (int64_t)it * F + j0) : zero4();
        }
        f4 h4[TF];
        {
            f4 acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = zero4();
WC_BEGIN();
#pragma unroll 1
            for (int ksl = 0; ksl < 4; ++ksl) {
                bf16x8 bf[3];
                x6_frag(h3[0], h3[1], bf);
                rotate2(h3);
                kstep<4>(buf(cid) + img_off(4, ksl, 0, 0), l, bf, acc);
            }
            WC_END();
#pragma unroll
            for (int q = 0; q < 4; ++q) h4[q] = relu_bias(acc[q], sBias + BO3 + 16 * q + 4 * g);
        }
        // ---- predict, loss, dz (the fused chain's epilogue, lyr_step_chain_kernel)
        float zp = 0.f;
#pragma unroll
        for (int q = 0; q < TF; ++q) {
            const f4 wm = ld4(&sWP[1][16 * q + 4 * g]);
            zp += wm.x * h4[q].x + wm.y * h4[q].y + wm.z * h4[q].z + wm.w * h4[q].w;
            if (gmf) {
                const f4 wg = ld4(&sWP[0][16 * q + 4 * g]);
                zp += wg.x * (ug[q].x * ig[q].x) + wg.y * (ug[q].y * ig[q].y) + wg.z * (ug[q].z * ig[q].z) +
                      wg.w * (ug[q].w * ig[q].w);
            }
        }
        zp += __shfl_xor(zp, 16, 64);
        zp += __shfl_xor(zp, 32, 64);
        const float z = zp + bp;
        if (valid && g == 0 && a.logits_out != nullptr) a.logits_out[m] = z;
        float dz = 0.f;
        if constexpr (BPR) {
            // pairwise (BPR), as in lyr_step_chain_kernel: ROWS (128) and each wave's 16-row
            // slice are even, so a pair never straddles a tile and the partner's z is in
            // lane l ^ 1; both rows of a pair are valid or both padding (stream contract).
            static_assert(ROWS % 2 == 0, "a BPR pair must not straddle a row tile");
            dz = bpr_dz(z, __shfl_xor(z, 1, 64), rw, valid, g == 0, s.gb, aL);
        } else if (valid) {
            if (a.dz_mode == NCF_DZ_BCE) {
                const float y = (float)(uint32_t)(rw >> 63);
                dz = (sigmoidf_(z) - y) / s.gb;
                if (g == 0) aL += bce_loss(z, y) / s.gb;
            } else if (a.dz_mode == NCF_DZ_KD) {
                const float y = (float)(uint32_t)(rw >> 63);
                float rl;
                const float rg = kd_response(z, a.dlogit[s.base + m], a.kd_temp, &rl);
                dz = (a.kd_wt * (sigmoidf_(z) - y) + a.kd_wr * rg) / s.gb;
                if (g == 0) aL += (a.kd_wt * bce_loss(z, y) + a.kd_wr * rl) / s.gb;
            } else {
                dz = a.dlogit[s.base + m];
            }
        }
        if (g == 0) aB += dz;
        // dwp partials of this tile: sums over the wave's 16 rows -> LDS
#pragma unroll
        for (int q = 0; q < TF; ++q) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float vg = gmf ? dz * (lane_get(ug[q], r) * lane_get(ig[q], r)) : 0.f;
                float vm = dz * lane_get(h4[q], r);
#pragma unroll
                for (int o2 = 1; o2 < 16; o2 <<= 1) {
                    vg += __shfl_xor(vg, o2, 64);
                    vm += __shfl_xor(vm, o2, 64);
                }
                if (c == 0) {
                    if (gmf) atomicAdd(&sred[16 * q + 4 * g + r], vg);
                    atomicAdd(&sred[F + 16 * q + 4 * g + r], vm);
                }
            }
        }
        // ---- GMF backward: user rows per row, item rows staged for the run walk
        if (g == 0) sIt[w][c] = valid ? it : -1;
        if (gmf) {
#pragma unroll
            for (int q = 0; q < TF; ++q) {
                const int j0 = 16 * q + 4 * g;
                const f4 wg = ld4(&sWP[0][j0]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dg = dz * lane_get(wg, r);
                    if (valid) atomicAdd(a.grads + lay.ug + (int64_t)u * F + j0 + r, dg * lane_get(ig[q], r));
                    sIg[w][c][j0 + r] = dg * lane_get(ug[q], r);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same-wave LDS hand-off
            int ids[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) ids[r] = __builtin_amdgcn_readfirstlane(sIt[w][r]);
            {
                const int f = l;  // F = 64: one feature per lane
                float v[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = sIg[w][r][f];
                float run = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    run += v[r];
                    if (r == 15 || ids[r + 1] != ids[r]) {
                        if (ids[r] >= 0) atomicAdd(a.grads + lay.ig + (int64_t)ids[r] * F + f, run);
                        run = 0.f;
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next tile's writes
        }
        // ---- D_3 = dz wp_mlp [H_4 > 0]
        f4 d3[TF];
#pragma unroll
        for (int q = 0; q < TF; ++q) {
            const f4 wm = ld4(&sWP[1][16 * q + 4 * g]);
            d3[q] = masked(f4{dz * wm.x, dz * wm.y, dz * wm.z, dz * wm.w}, pos_bits(h4[q]));
            if (st) *reinterpret_cast<f4*>(o.D[3] + m * S(4) + 16 * q + 4 * g) = d3[q];
        }
        // ---- bwd layer 3: dH_3 = D_3 W_3 (M = 128, K = 64), D_2 = dH_3 [H_3 > 0]
        f4 d2[8];
        {
            f4 acc[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = zero4();
WC_BEGIN();
#pragma unroll 1
            for (int ksl = 0; ksl < 2; ++ksl) {
                bf16x8 bf[3];
                x6_frag(d3[0], d3[1], bf);
                rotate2(d3);
                kstep<8>(buf(cid) + img_off(8, ksl, 0, 0), l, bf, acc);
            }
            WC_END();
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                d2[q] = masked(acc[q], m3 >> (4 * q));
                if (st) *reinterpret_cast<f4*>(o.D[2] + m * S(3) + 16 * q + 4 * g) = d2[q];
            }
        }
        // ---- bwd layer 2: dH_2 = D_2 W_2 (M = 256, K = 128), D_1 = dH_2 [H_2 > 0]
        f4 d1[16];
        {
            f4 acc[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = zero4();
#pragma unroll 1
            for (int ks = 0; ks < 4; ++ks) {
                WC_BEGIN();
                bf16x8 bf[3];
                x6_frag(d2[0], d2[1], bf);
                rotate2(d2);
                kstep<16>(buf(cid), l, bf, acc);
                WC_END();
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                d1[q] = masked(acc[q], (q < 8 ? m2lo : m2hi) >> (4 * (q & 7)));
                if (st) *reinterpret_cast<f4*>(o.D[1] + m * S(2) + 16 * q + 4 * g) = d1[q];
            }
        }
        // ---- bwd layer 1: dH_1 = D_1 W_1 (M = 512 in two groups of 256, K = 256),
        //      D_0 = dH_1 [H_1 > 0] (row order: lyr_scatter0_kernel and the expansion read it)
#pragma unroll 1
        for (int gq = 0; gq < 2; ++gq) {
            f4 acc[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = zero4();
#pragma unroll 1
            for (int ks = 0; ks < 8; ++ks) {
                WC_BEGIN();
                bf16x8 bf[3];
                x6_frag(d1[0], d1[1], bf);
                rotate2(d1);  // cyclic: both groups read D_1 from the front
                kstep<16>(buf(cid), l, bf, acc);
                WC_END();
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                // feature 256 gq + 16 q + 4 g + r: H_1 K step s = 8 gq + q / 2, half q & 1
                // -> bit 8 (15 - s) + 4 (q & 1) + r of mb
                const int b = 8 * (15 - (8 * gq + (q >> 1))) + 4 * (q & 1);
                const int wd = b >> 5;
                const uint32_t word = wd == 0 ? mb0 : (wd == 1 ? mb1 : (wd == 2 ? mb2 : mb3));
                const f4 d0 = masked(acc[q], word >> (b & 31));
                if (st) *reinterpret_cast<f4*>(o.D[0] + m * DM + 256 * gq + 16 * q + 4 * g) = d0;
            }
        }
    }
    // ---- block tail: dbp, loss -> LDS; dwp / dbp / loss -> slab
#pragma unroll
    for (int o2 = 1; o2 < 64; o2 <<= 1) {
        aB += __shfl_xor(aB, o2, 64);
        aL += __shfl_xor(aL, o2, 64);
    }
    if (l == 0) {
        atomicAdd(&sred[2 * F], aB);
        atomicAdd(&sred[2 * F + 1], aL);
    }
    __syncthreads();
    const int64_t tb = lay.tower_begin;
    float* slab = a.slab + (int64_t)(blockIdx.x % lyr_slab_rows(&lay)) * (lay.tower_len + 64);
    for (int e = t; e < 2 * F + 2; e += NT) {
        int64_t off;
        if (e < F) {
            if (!gmf) continue;
            off = (lay.wp - tb) + e;
        } else if (e < 2 * F) {
            off = (lay.wp - tb) + Pg + (e - F);
        } else {
            off = e == 2 * F ? (lay.bp - tb) : lay.tower_len;
        }
        const float v = sred[e];
        if (v != 0.f) atomicAdd(slab + off, v);
    }
}

// NCF_WIDE_CHAIN=0 (environment) keeps the per-layer kernels for A/B runs.
static bool wide_chain_enabled() {
    static int on = -1;
    if (on < 0) {
        const char* e = getenv("NCF_WIDE_CHAIN");
        on = (e != nullptr && e[0] == '0') ? 0 : 1;
    }
    return on == 1;
}

// The wide chain for (DM, L) = (512, 4) with factor 64: the chunk images (prep) then
// the chain; false where it does not apply (the caller runs the per-layer kernels).
// img: wc::NCH * wc::CHUNK bytes of the workspace (lyr_workspace_floats).
// The weight images of the step (W_1..W_3 chunks and, with w0img, the W0 images of the
// projection and the expansion): one launch, before the projection.
static bool wide_chain_applies(const ncf_layout& lay) {
    return (lay.factor_num << (lay.num_layers - 1)) == wc::DM && lay.num_layers == wc::L && wide_chain_enabled();
}
static void launch_wc_prep(const LyrArgs& a, char* img, char* w0img, hipStream_t st) {
    const int threads = wc::PREP_THREADS + (w0img ? wc::W0_PREP_THREADS : 0);
    hipLaunchKernelGGL(lyr_wc_prep_kernel, dim3((threads + 255) / 256), dim3(256), 0, st, a.params, a.lay, img, w0img);
}
static bool launch_wide_chain(const LyrArgs& a, const float* P, const ChainBufs& o, char* img, int64_t R,
                              hipStream_t st, bool prepped = false) {
    const ncf_layout& lay = a.lay;
    const int L = lay.num_layers, DM = lay.factor_num << (L - 1);
    if (DM != wc::DM || L != wc::L || img == nullptr || !wide_chain_enabled()) return false;
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&lyr_wide_chain_kernel<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 2 * wc::CHUNK) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(&lyr_wide_chain_kernel<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, 2 * wc::CHUNK) != hipSuccess)
            return false;
        attr = true;
    }
    if (!prepped) launch_wc_prep(a, img, nullptr, st);
    int64_t grid = (R + wc::ROWS - 1) / wc::ROWS;
    if (grid > 256) grid = 256;  // one 8-wave block per CU, persistent over the tiles
    if (grid < 1) grid = 1;
    if (a.dz_mode == NCF_DZ_BPR)
        hipLaunchKernelGGL(lyr_wide_chain_kernel<true>, dim3((unsigned)grid), dim3(wc::NT), 2 * wc::CHUNK, st, a, P, o,
                           (const char*)img, R);
    else
        hipLaunchKernelGGL(lyr_wide_chain_kernel<false>, dim3((unsigned)grid), dim3(wc::NT), 2 * wc::CHUNK, st, a, P,
                           o, (const char*)img, R);
    return true;
}
