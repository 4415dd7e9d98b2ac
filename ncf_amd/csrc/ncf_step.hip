// The train step and what every entry point derives from a layout: ncf_layout_init /
// ncf_layout_tune, the debug switches, the layout geometry helpers (ncf_host.h), workspace
// sizes, ncf_train_step[_kd] with the user store-and-sum, ncf_forward, and the in-step
// Adam protocol (ncf_ais_*, ncf_train_step_ais).  gfx950 only.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ncf_host.h"

namespace ncf {

// User store-and-sum (NCF_LAYOUT_USER_STORE).  Float atomics run at the memory side at
// ~1.3 TB/s of added bytes (MI355X_MICROARCH.md, Global float atomics), plain stores at
// ~6 TB/s: at C3 the user half of the step's scatter (65,536 rows x (64 + 16) floats,
// ~10.8 rows per user per batch, rows in item order so nothing merges in a tile) was
// the largest single atomic stream of the step.  The step stores each row's user-side
// gradient into ustore[row][uw] ([Um part][Ug part], row = slice offset); this launch
// walks the slice's user order (ncf_user_order: entries user << 32 | offset, users
// ascending, padding last) in pieces of US_SPAN positions, one wave per piece: the
// piece's rows are loaded together, summed per run of equal users in order, and each
// run's sum is added to its user's Um / Ug rows by one float atomic per column -- every
// wave the same work whatever the user skew, and ~US_SPAN / (runs + 1) times fewer
// atomic bytes than per row.  Lane = column (uw <= 64 * US_NCH).
constexpr int US_SPAN = 32, US_WAVES = 4, US_NCH = 4;
struct UsArgs {
    const float* ustore;
    const int64_t* order;
    float* grads;
    const ncf_step_ctl* ctl;
    int64_t batch_global, um, ug;
    int world, rank, dmu, f, uw;
};
template <int NCH>
__global__ __launch_bounds__(US_WAVES * 64) void user_sum_kernel(UsArgs A) {
    // this rank's slice of the current batch (ncf_train.hip: the step's own rows)
    const int64_t ntot = A.ctl->n_total;
    const int64_t nbatch = (ntot + A.batch_global - 1) / A.batch_global;
    const int64_t b = nbatch > 0 ? A.ctl->batch % nbatch : 0;
    const int64_t b0 = b * A.batch_global;
    int64_t gb = ntot - b0;
    if (gb > A.batch_global) gb = A.batch_global;
    if (gb < 0) gb = 0;
    const int64_t per = (gb + A.world - 1) / A.world;
    int64_t lo = (int64_t)A.rank * per, hi = lo + per;
    if (lo > gb) lo = gb;
    if (hi > gb) hi = gb;
    const int64_t base = b0 + lo, nloc = hi - lo;
    const int lane = threadIdx.x & 63;
    const int64_t p0 = ((int64_t)blockIdx.x * US_WAVES + (threadIdx.x >> 6)) * US_SPAN;
    if (p0 >= nloc) return;  // wave-uniform
    const int64_t e = lane < US_SPAN && p0 + lane < nloc ? A.order[base + p0 + lane] : -1;
    const int eu = (int)(e >> 32), eo = (int)(uint32_t)e;  // past the slice: user -1 (stop)
    float v[US_SPAN][NCH];
#pragma unroll
    for (int t = 0; t < US_SPAN; ++t) {
        const int ut = __builtin_amdgcn_readlane(eu, t), ot = __builtin_amdgcn_readlane(eo, t);
        const float* src = A.ustore + (int64_t)ot * A.uw;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
            v[t][ch] = (ut >= 0 && ch * 64 + lane < A.uw) ? src[ch * 64 + lane] : 0.f;
    }
    float acc[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) acc[ch] = 0.f;
#pragma unroll
    for (int t = 0; t < US_SPAN; ++t) {
        const int ut = __builtin_amdgcn_readlane(eu, t);
        if (ut < 0) break;  // padding rows sort last
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) acc[ch] += v[t][ch];
        const int un = t + 1 < US_SPAN ? __builtin_amdgcn_readlane(eu, t + 1) : -1;
        if (un != ut) {  // the run (or this piece of it) ends: one atomic per column
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const int col = ch * 64 + lane;
                if (col < A.dmu)
                    atomicAdd(A.grads + A.um + (int64_t)ut * A.dmu + col, acc[ch]);
                else if (col < A.uw)
                    atomicAdd(A.grads + A.ug + (int64_t)ut * A.f + (col - A.dmu), acc[ch]);
                acc[ch] = 0.f;
            }
        }
    }
}

static const KernelEntry* find_entry(int mode, int F, int L) {
    int n = 0;
    const KernelEntry* t = kernel_table(&n);
    const int Lk = (mode == NCF_MODEL_GMF) ? 1 : L;
    for (int i = 0; i < n; ++i)
        if (t[i].mode == mode && t[i].F == F && t[i].L == Lk) return &t[i];
    return nullptr;
}

static int64_t train_lds_floats(const KernelEntry* e, const ncf_layout* lay, int geo = GEO_8) {
    const int64_t img = lay->tower_len + 1;
    return e->w_total + e->misc[geo] + (e->stage[geo] > img ? e->stage[geo] : img);
}

Ranges make_ranges(const int64_t* ranges, int nranges, int* err) {
    Ranges R;
    memset(&R, 0, sizeof(R));
    *err = 0;
    if (nranges < 1 || nranges > 8) {
        *err = 1;
        return R;
    }
    R.n = nranges;
    R.prefix[0] = 0;
    for (int i = 0; i < nranges; ++i) {
        const int64_t b = ranges[2 * i], e = ranges[2 * i + 1];
        if (b < 0 || e < b || (b & 3) || ((e - b) & 3)) *err = 1;
        R.begin[i] = b;
        R.prefix[i + 1] = R.prefix[i] + (e - b) / 4;
    }
    for (int i = nranges + 1; i < 9; ++i) R.prefix[i] = R.prefix[nranges];
    return R;
}

static int g_diag = 0;
int diag_flags() { return g_diag; }
static unsigned long long* g_stamps = nullptr;
// ncf_debug_set_geometry: 0 = ncf_layout_tune decides, 4 / NWAVES = forced (A/B, tests)
static int g_geo_waves = 0;
// ncf_debug_set_per_row: -1 = ncf_layout_tune's rule (2 rows < U + I), 0 / 1 forced (A/B)
static int g_per_row = -1;
// ncf_debug_set_user_store: 0 = off (the default: measured slower),
// -1 = ncf_layout_tune decides by the per-rank batch, 1 = wherever it applies
static int g_user_store = 0;
// ncf_layout_tune: user store-and-sum from this many rows per launch up
#ifndef NCF_US_MIN_ROWS
#define NCF_US_MIN_ROWS 16384
#endif
// ncf_layout_tune: 8-wave workgroups from this many 128-row tiles up, else 4-wave
#ifndef NCF_GEO_MIN_WGS
#define NCF_GEO_MIN_WGS 256
#endif
constexpr int64_t GEO_MIN_WGS = NCF_GEO_MIN_WGS;

int launch_status() { return hipGetLastError() == hipSuccess ? NCF_OK : NCF_E_LAUNCH; }

// hipFuncSetAttribute once per (kernel, size): nothing but launches happen on
// the hot path, so a step can be captured into a hipGraph.  Every kernel of the library
// with dynamic LDS comes through here (training, preparation and serving), so the pool
// grows: a kernel is never dropped, and it is appended on its first call only.
int ensure_lds(const void* fn, int64_t bytes) {
    struct Slot { const void* fn; int64_t bytes; };
    static std::vector<Slot> slots;
    if (slots.capacity() == 0) slots.reserve(256);
    for (const Slot& s : slots)
        if (s.fn == fn && s.bytes >= bytes) return NCF_OK;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        return NCF_E_LAUNCH;
    for (Slot& s : slots)
        if (s.fn == fn) { s.bytes = bytes; return NCF_OK; }
    slots.push_back(Slot{fn, bytes});
    return NCF_OK;
}

// Factored layer 0 for this layout?  MLP shapes whose two embedding tables have
// fewer rows than FACT_MAX_ROWS (the expand pass works on U + I rows per step, the
// per-row layer-0 gradients on B rows: at ml-1m 9.7K vs 65K; at ml-20m the tables
// have 165K rows and the per-row form stays), on the fused path or, for DM up to
// 128, the layered one (there the layer-0 forward is a per-step projection of the
// tables too, ncf_layered.hip).
#ifndef NCF_FACT_MAX_ROWS
#define NCF_FACT_MAX_ROWS 32768
#endif
constexpr int64_t FACT_MAX_ROWS = NCF_FACT_MAX_ROWS;
// Fused kernel for this layout, or nullptr (then the layered path runs).
static const KernelEntry* fused_entry(const ncf_layout* lay) {
    const KernelEntry* e = find_entry(lay->model_type, lay->factor_num, lay->num_layers);
    if (!e) return nullptr;
    return train_lds_floats(e, lay) * 4 <= LDS_LIMIT_BYTES ? e : nullptr;
}
// Fused kernel of a training step: none with dropout (the layered path applies it).
const KernelEntry* train_fused(const ncf_layout* lay) {
    if (lay->flags & NCF_LAYOUT_LAYERED) return nullptr;
    return lay->dropout > 0.f ? nullptr : fused_entry(lay);
}
int fact_dm(const ncf_layout* lay) { return lay->factor_num << (lay->num_layers - 1); }
bool fact_mode(const ncf_layout* lay) {
    if (lay->model_type == NCF_MODEL_GMF || (lay->flags & NCF_LAYOUT_PER_ROW_L0)) return false;
    if (lay->dropout > 0.f) return false;  // masks per row: layer 0 does not factor per entity
    if ((int64_t)lay->user_num + lay->item_num > FACT_MAX_ROWS) return false;
    const int dm = fact_dm(lay);
    const bool lds_dm = dm == 8 || dm == 16 || dm == 32 || dm == 64 || dm == 128;  // fact_expand_kernel<DM>
    const KernelEntry* e = train_fused(lay);
    if (e) return lds_dm && e->train_fact[GEO_8] != nullptr;
    // layered path: wider dm (256, 512) expanded with GEMMs (ncf_layered.hip lyr_fact_dx / dw0)
    return (lds_dm || dm == 256 || dm == FACT_MAX_DM) && lay->factor_num <= LYR_MAX_FACTOR;
}

// Launch geometry of the fused training step: 4-wave workgroups where
// ncf_layout_tune asked for them (the NCF_LAYOUT_GEO field) and the kernel exists.
static int train_geo(const KernelEntry* e, const ncf_layout* lay) {
    const int g = (lay->flags >> NCF_LAYOUT_GEO_SHIFT) & NCF_LAYOUT_GEO_MASK;
    if (g == GEO_8) return GEO_8;
    const void* fn = fact_mode(lay) ? e->train_fact[g] : e->train[g];
    return fn != nullptr ? g : GEO_8;
}

// Workgroups of the fused step = rows of the slab the reductions read.
static int slab_rows_of(const ncf_layout* lay) {
    const int w = (lay->flags >> NCF_LAYOUT_WG_SHIFT) & NCF_LAYOUT_WG_MASK;
    return (w > 0 && w < SLAB_ROWS) ? w : SLAB_ROWS;
}

// First tower column (relative to tower_begin) the reductions produce: GMF models
// have no tower.
int slab_lo(const ncf_layout* lay) {
    if (lay->model_type == NCF_MODEL_GMF) return (int)(lay->wp - lay->tower_begin);
    return 0;
}

// NCF_LAYOUT_USER_STORE: user-side gradient row width ([Um part][Ug part]) and
// whether the fused step can run it (user_order_kernel's user bound, the sum
// kernel's columns, vector-aligned parts).
static int us_uw(const ncf_layout* lay) {
    const bool mlp = lay->model_type != NCF_MODEL_GMF, gmf = lay->model_type != NCF_MODEL_MLP;
    return (mlp ? (lay->factor_num << (lay->num_layers - 1)) : 0) + (gmf ? lay->factor_num : 0);
}
static bool us_applies(const ncf_layout* lay) {
    return train_fused(lay) != nullptr && lay->user_num <= UO_MAX_USERS && lay->factor_num % 4 == 0 &&
           us_uw(lay) <= 64 * US_NCH;
}
bool us_on(const ncf_layout* lay) { return (lay->flags & NCF_LAYOUT_USER_STORE) && us_applies(lay); }
static int64_t us_floats(const ncf_layout* lay, int64_t rows) {
    return us_on(lay) ? ((rows + TILE_ROWS + 63) & ~(int64_t)63) * us_uw(lay) : 0;
}

// The dW0 partials in the train workspace: after the fused path's slab rows, or
// after the layered path's single slab row (ncf_layered.hip).
static float* fact_partials(const ncf_layout* lay, void* workspace) {
    const int64_t stride = lay->tower_len + 64;
    return static_cast<float*>(workspace) +
           (train_fused(lay) ? (int64_t)SLAB_ROWS * stride : rup64((int64_t)lyr_slab_rows(lay) * stride));
}

// Rows of the partial slab the reductions sum: the fused step's workgroups, or the
// layered path's lyr_slab_rows.
int reduce_rows(const ncf_layout* lay) { return train_fused(lay) ? slab_rows_of(lay) : lyr_slab_rows(lay); }

// NCF_LAYOUT_FACT_DEFER_DX: the W0 the step ran with ([DM][2 DM]), saved by the
// expansion after the dW0 partials; ncf_adam_step_fact forms dX = G W0 half from it
// while the same launch updates W0 itself (fused path, dm <= FACT_LDS_DM).
static int64_t fact_w0_snap_floats(const ncf_layout* lay) {
    const int64_t DM = fact_dm(lay);
    return DM <= FACT_LDS_DM ? 2 * DM * DM : 0;
}
float* fact_w0_snap(const ncf_layout* lay, void* workspace) {
    return fact_partials(lay, workspace) + fact_partials_floats(lay);
}

W0Part w0_part(const ncf_layout* lay, const void* workspace) {
    W0Part wp;
    memset(&wp, 0, sizeof(wp));
    if (!fact_mode(lay) || fact_dm(lay) > FACT_LDS_DM) return wp;  // W0 from the slab
    wp.p = fact_partials(lay, const_cast<void*>(workspace));
    wp.nblk = fact_blocks(lay, &wp.nbu);
    wp.dm = lay->factor_num << (lay->num_layers - 1);
    wp.cols = (int)(lay->b[0] - lay->w[0]);
    return wp;
}

}  // namespace ncf

using namespace ncf;

extern "C" {

int ncf_abi_version(void) { return NCF_ABI_VERSION; }

int ncf_debug_set_diag(int flags) {
    g_diag = flags;
    return NCF_OK;
}

int ncf_debug_set_stamps(unsigned long long* dev_buf) {
    g_stamps = dev_buf;
    return NCF_OK;
}

int ncf_slab_rows(void) { return SLAB_ROWS; }

int ncf_fact_mode(const ncf_layout* lay) { return lay && fact_mode(lay) ? 1 : 0; }

int ncf_reduce_rows(const ncf_layout* lay) { return lay ? reduce_rows(lay) : -1; }

uint32_t ncf_dropout_hash(uint32_t seed, uint32_t t, uint32_t layer, int64_t row, uint32_t col) {
    return dropout_hash(seed, t, layer, row, col);
}

int ncf_layout_tune(ncf_layout* lay, int64_t rows) {
    if (!lay || rows <= 0) return NCF_E_ARG;
    int32_t f = lay->flags & ~(NCF_LAYOUT_PER_ROW_L0 | (NCF_LAYOUT_GEO_MASK << NCF_LAYOUT_GEO_SHIFT) |
                               (NCF_LAYOUT_WG_MASK << NCF_LAYOUT_WG_SHIFT) | NCF_LAYOUT_USER_STORE);
    if (g_per_row == 1 || (g_per_row < 0 && 2 * rows < (int64_t)lay->user_num + lay->item_num))
        f |= NCF_LAYOUT_PER_ROW_L0;
    lay->flags = f;
    // geometry: forced (ncf_debug_set_geometry), else 8-wave workgroups where the
    // batch has GEO_MIN_WGS 128-row tiles and 4-wave ones below (twice the workgroups,
    // one wave per SIMD).  Measured on the MI355X (profiles/r04_evidence/geometry_*):
    // C2 (1,024 rows) 22.3 / 19.1 / 19.8 / 20.8 us per step at 8 / 4 / 2 / 1 waves,
    // C5 (256) 13.3 / 12.4 / 12.8 / 13.2, the C3 step at 8,192 rows per rank 31.0 /
    // 27.5 (train launch); the 2- and 1-wave kernels stay for A/B.
    const KernelEntry* e = train_fused(lay);
    int g = GEO_8;
    if (e) {
        auto avail = [&](int gg) {
            lay->flags = f | (gg << NCF_LAYOUT_GEO_SHIFT);
            return train_geo(e, lay) == gg;
        };
        if (g_geo_waves != 0) {
            for (int gg = 0; gg < NGEO; ++gg)
                if (geo_waves(gg) == g_geo_waves && avail(gg)) g = gg;
        } else if ((rows + 127) / 128 < GEO_MIN_WGS && avail(GEO_4)) {
            g = GEO_4;
        }
    }
    f |= g << NCF_LAYOUT_GEO_SHIFT;
    // user store-and-sum (user_sum_kernel), when enabled: forced, or by the per-rank
    // batch (-1).  Off by default: at C3 the step kernel went 41.1 -> 39.2 us without
    // its user atomics but the sum launch took 11.0 us (and the user order 1.7 us per
    // step), 65.4 -> 75.6 us per step (profiles/r04_evidence/user_store_ab.json)
    lay->flags = f;
    if (us_applies(lay) && (g_user_store == 1 || (g_user_store < 0 && rows >= NCF_US_MIN_ROWS)))
        f |= NCF_LAYOUT_USER_STORE;
    const int tr = 16 * geo_waves(g);
    const int64_t tiles = (rows + tr - 1) / tr;
    if (tiles < SLAB_ROWS) f |= (int32_t)tiles << NCF_LAYOUT_WG_SHIFT;
    lay->flags = f;
    return NCF_OK;
}

int ncf_debug_set_per_row(int mode) {
    if (mode < -1 || mode > 1) return NCF_E_ARG;
    g_per_row = mode;
    return NCF_OK;
}

int ncf_debug_set_user_store(int mode) {
    if (mode < -1 || mode > 1) return NCF_E_ARG;
    g_user_store = mode;
    return NCF_OK;
}

int ncf_debug_set_geometry(int waves) {
    if (waves != 0 && waves != 1 && waves != 2 && waves != 4 && waves != NWAVES) return NCF_E_ARG;
    g_geo_waves = waves;
    return NCF_OK;
}

int ncf_layout_init(int U, int I, int F, int L, int mode, ncf_layout* o) {
    if (!o || U <= 0 || I <= 0 || F <= 0 || L < 1 || L > 4 || mode < 0 || mode > 2) return NCF_E_ARG;
    memset(o, 0, sizeof(*o));
    const int64_t DM = (int64_t)F << (L - 1);
    const int64_t P = mode == NCF_MODEL_NEUMF ? 2 * F : F;
    int64_t off = 0;
    o->ug = off; off += rup64((int64_t)U * F);
    o->ig = off; off += rup64((int64_t)I * F);
    o->um = off; off += rup64((int64_t)U * DM);
    o->im = off; off += rup64((int64_t)I * DM);
    o->tower_begin = off;
    for (int k = 0; k < 4; ++k) {
        if (k < L) {
            const int64_t si = (2 * DM) >> k, so = si / 2;
            o->w[k] = off; off += rup64(so * si);
            o->b[k] = off; off += rup64(so);
        } else {
            o->w[k] = -1;
            o->b[k] = -1;
        }
    }
    o->wp = off; off += rup64(P);
    o->bp = off; off += 64;
    o->tower_len = off - o->tower_begin;
    off += 64;  // loss slot + pad
    o->total = off;
    o->user_num = U; o->item_num = I; o->factor_num = F; o->num_layers = L; o->model_type = mode;
    return NCF_OK;
}

int ncf_supported(int mode, int F, int L) {
    ncf_layout lay;
    if (ncf_layout_init(1, 1, F, L, mode, &lay) != NCF_OK) return 0;
    if (fused_entry(&lay)) return NCF_PATH_FUSED;
    return F <= LYR_MAX_FACTOR ? NCF_PATH_LAYERED : 0;
}

// fused-path workspace: slab rows, [factored: dW0 partials, W0 snapshot], [user store]
static int64_t us_base_floats(const ncf_layout* lay) {
    return (int64_t)SLAB_ROWS * ncf_slab_stride(lay) +
           (fact_mode(lay) ? fact_partials_floats(lay) + fact_w0_snap_floats(lay) : 0);
}

int64_t ncf_workspace_bytes(const ncf_layout* lay, int64_t rows) {
    if (!lay || rows < 0) return -1;
    if (train_fused(lay))
        return (us_base_floats(lay) + us_floats(lay, rows)) * 4;
    return lyr_workspace_floats(lay, rows, true, fact_mode(lay) ? fact_partials_floats(lay) : -1) * 4;
}

int64_t ncf_forward_workspace_bytes(const ncf_layout* lay, int64_t n) {
    if (!lay || n < 0) return -1;
    if (fused_entry(lay)) return 0;
    return lyr_workspace_floats(lay, n, false, -1) * 4;
}

static int train_step_impl(const ncf_layout* lay, const float* params, float* grads, const uint64_t* rows,
                           const int64_t* user_order, const float* dlogit, ncf_step_ctl* ctl, int64_t batch_global,
                           int world, int rank,
                           int dz_mode, float kd_wt, float kd_wr, float kd_temp, void* workspace,
                           int64_t workspace_bytes,
                           float* logits_out, void* stream) {
    if (!lay || !params || !grads || !rows || !ctl || !workspace) return NCF_E_ARG;
    if (batch_global <= 0 || world < 1 || rank < 0 || rank >= world) return NCF_E_ARG;
    if (dz_mode != NCF_DZ_BCE && dz_mode != NCF_DZ_DLOGIT && dz_mode != NCF_DZ_KD && dz_mode != NCF_DZ_BPR)
        return NCF_E_ARG;
    // pairwise: rows 2k / 2k + 1 are one triple -- a rank slice (ceil(gb / world)) or an odd
    // batch could split a pair; dlogit is ignored (labels ride in the rows, as for BCE)
    if (dz_mode == NCF_DZ_BPR && (world != 1 || (batch_global & 1))) return NCF_E_ARG;
    const bool has_dl = dz_mode == NCF_DZ_DLOGIT || dz_mode == NCF_DZ_KD;
    if (has_dl && !dlogit) return NCF_E_ARG;
    const int64_t rows_max = (batch_global + world - 1) / world;
    if (workspace_bytes < ncf_workspace_bytes(lay, rows_max)) return NCF_E_ARG;
    float* slab = static_cast<float*>(workspace);
    const KernelEntry* e = train_fused(lay);
    if (!e) {
        LyrArgs la;
        memset(&la, 0, sizeof(la));
        la.lay = *lay;
        la.params = params;
        la.grads = grads;
        la.rows = rows;
        // (the pairwise kernels take rows in stream order: a pair stream is not item-grouped,
        // and its user runs are the pairs themselves)
        la.uorder = ncf_uses_user_order(lay) && dz_mode != NCF_DZ_BPR ? user_order : nullptr;
        la.dlogit = dlogit;
        la.ctl = ctl;
        la.batch_global = batch_global;
        la.world = world;
        la.rank = rank;
        la.dz_mode = dz_mode;
        la.kd_wt = kd_wt;
        la.kd_wr = kd_wr;
        la.kd_temp = kd_temp;
        la.logits_out = logits_out;
        la.fact_part_floats = fact_mode(lay) ? fact_partials_floats(lay) : -1;
        const int rc = lyr_run(la, slab, rows_max, true, (hipStream_t)stream);
        if (rc != NCF_OK || la.fact_part_floats < 0) return rc;
        return launch_fact_expand(lay, params, grads, fact_partials(lay, workspace), nullptr, (hipStream_t)stream);
    }
    const int geo = train_geo(e, lay);
    const int64_t lds = train_lds_floats(e, lay, geo) * 4;
    if (lds > LDS_LIMIT_BYTES) return NCF_E_UNSUPPORTED;
    const void* fn = fact_mode(lay) ? e->train_fact[geo] : e->train[geo];
    if (dz_mode == NCF_DZ_BPR) {  // the pairwise instantiation of the same (shape, path, geometry)
        int nt = 0, nb = 0;
        const KernelEntry* t0 = kernel_table(&nt);
        const BprEntry* b = kernel_table_bpr(&nb) + (e - t0);
        if (nb != nt || e < t0 || e >= t0 + nt) return NCF_E_UNSUPPORTED;
        fn = fact_mode(lay) ? b->train_fact[geo] : b->train[geo];
        if (!fn) return NCF_E_UNSUPPORTED;
    }
    if (ensure_lds(fn, lds) != NCF_OK) return NCF_E_LAUNCH;
    TrainArgs a;
    memset(&a, 0, sizeof(a));
    a.lay = *lay;
    a.params = params;
    a.grads = grads;
    a.rows = rows;
    // BCE mode: point dlogit at the rows so the per-row load stays unconditional
    a.dlogit = has_dl ? dlogit : reinterpret_cast<const float*>(rows);
    a.ctl = ctl;
    a.batch_global = batch_global;
    a.world = world;
    a.rank = rank;
    a.dz_mode = dz_mode;
    a.kd_wt = kd_wt;
    a.kd_wr = kd_wr;
    a.kd_temp = kd_temp;
    a.diag = g_diag;
    a.stamps = g_stamps;
    a.slab = slab;
    a.logits_out = logits_out;
    const bool us = us_on(lay) && user_order != nullptr;
    if (us) {
        a.ustore = slab + us_base_floats(lay);
        a.uw = us_uw(lay);
    }
    void* args[] = {&a};
    if (hipLaunchKernel(fn, dim3(slab_rows_of(lay)), dim3(geo_waves(geo) * WAVE), args, (size_t)lds,
                        (hipStream_t)stream) != hipSuccess)
        return NCF_E_LAUNCH;
    int rc = launch_status();
    if (rc != NCF_OK) return rc;
    if (us) {  // the stored user-side rows summed per user (before the factored expansion reads G)
        UsArgs ua;
        memset(&ua, 0, sizeof(ua));
        ua.ustore = a.ustore;
        ua.order = user_order;
        ua.grads = grads;
        ua.ctl = ctl;
        ua.batch_global = batch_global;
        ua.um = lay->um;
        ua.ug = lay->ug;
        ua.world = world;
        ua.rank = rank;
        ua.uw = a.uw;
        ua.dmu = lay->model_type != NCF_MODEL_GMF ? (lay->factor_num << (lay->num_layers - 1)) : 0;
        ua.f = lay->factor_num;
        const int64_t waves = (rows_max + US_SPAN - 1) / US_SPAN;
        const dim3 grid((unsigned)((waves + US_WAVES - 1) / US_WAVES)), blk(US_WAVES * 64);
        const hipStream_t st = (hipStream_t)stream;
        switch ((a.uw + 63) / 64) {
            case 1: hipLaunchKernelGGL(user_sum_kernel<1>, grid, blk, 0, st, ua); break;
            case 2: hipLaunchKernelGGL(user_sum_kernel<2>, grid, blk, 0, st, ua); break;
            case 3: hipLaunchKernelGGL(user_sum_kernel<3>, grid, blk, 0, st, ua); break;
            default: hipLaunchKernelGGL(user_sum_kernel<US_NCH>, grid, blk, 0, st, ua); break;
        }
        rc = launch_status();
        if (rc != NCF_OK) return rc;
    }
    if (!fact_mode(lay)) return rc;
    // factored layer 0: the per-user / per-item D0 sums -> dUm, dIm, dW0 partials
    return launch_fact_expand(lay, params, grads, fact_partials(lay, workspace), fact_w0_snap(lay, workspace),
                              (hipStream_t)stream);
}

int ncf_train_step(const ncf_layout* lay, const float* params, float* grads, const uint64_t* rows,
                   const int64_t* user_order, const float* dlogit, ncf_step_ctl* ctl, int64_t batch_global,
                   int world, int rank,
                   int dz_mode, void* workspace, int64_t workspace_bytes, float* logits_out, void* stream) {
    if (dz_mode == NCF_DZ_KD) return NCF_E_ARG;  // ncf_train_step_kd carries the weights
    return train_step_impl(lay, params, grads, rows, user_order, dlogit, ctl, batch_global, world, rank, dz_mode, 0.f,
                           0.f, 0.f,
                           workspace, workspace_bytes, logits_out, stream);
}

int ncf_train_step_kd(const ncf_layout* lay, const float* params, float* grads, const uint64_t* rows,
                      const int64_t* user_order, const float* teacher_logits, ncf_step_ctl* ctl,
                      int64_t batch_global, int world, int rank,
                      float w_task, float w_resp, float temperature, void* workspace, int64_t workspace_bytes,
                      float* logits_out, void* stream) {
    if (!teacher_logits) return NCF_E_ARG;
    return train_step_impl(lay, params, grads, rows, user_order, teacher_logits, ctl, batch_global, world, rank, NCF_DZ_KD,
                           w_task, w_resp, temperature, workspace, workspace_bytes, logits_out, stream);
}

// ---- the previous step's Adam inside the training launch (ABI 18, NCF_LAYOUT_ADAM_IN_STEP)
}  // extern "C"

namespace ncf {

// The fused kernel with the in-step optimizer for this layout and its geometry, or null.
static const void* ais_kernel(const ncf_layout* lay, int* geo) {
    const KernelEntry* e = train_fused(lay);
    if (!e || fact_mode(lay) || us_on(lay)) return nullptr;
    const int g = train_geo(e, lay);
    *geo = g;
    return e->train_ais[g];
}

// ncf_ais_begin: no update pending, S_{adam_t} in buffer 0; the three gradient buffers
// cleared over the active ranges and the loss slot.
__global__ __launch_bounds__(256) void ais_begin_kernel(ncf_step_ctl* ctl, int64_t* st, float* g0, float* g1, float* g2,
                                                        Ranges R, int64_t loss_i) {
    const int64_t total = R.prefix[R.n];
    const f4 z = f4{0.f, 0.f, 0.f, 0.f};
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        int which;
        const int64_t i = range_locate(R, q, &which);
        *reinterpret_cast<f4*>(g0 + i) = z;
        *reinterpret_cast<f4*>(g1 + i) = z;
        *reinterpret_cast<f4*>(g2 + i) = z;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        g0[loss_i] = g1[loss_i] = g2[loss_i] = 0.f;
        st[0] = 0;
        st[1] = ctl->adam_t & 1;
    }
}

// ncf_ais_bump: a chunk of k launches done -- k batches, k - 1 + pending updates applied,
// one pending for the next launch.
__global__ void ais_bump_kernel(ncf_step_ctl* ctl, int64_t* st, int64_t k) {
    if (threadIdx.x == 0) {
        const int64_t pend0 = st[0];
        ctl->adam_t = ctl->adam_t + k - 1 + pend0;
        ctl->batch = ctl->batch + k;
        st[0] = 1;
    }
}

// ncf_ais_flush, first launch: the pending update written into buffer 0 (or, with
// none pending, S_{adam_t} copied there from buffer 1), its loss recorded, its gradient
// cleared; reads ctl / st only (the second launch advances them).
__global__ __launch_bounds__(256) void ais_flush_kernel(AisArgs x, ncf_step_ctl* ctl, int64_t loss_i) {
#pragma clang fp contract(off)
    __shared__ float sc[2];
    const int64_t pend = x.st[0], par = x.st[1];
    const int64_t n = ctl->adam_t + 1;
    const int rb = (int)((pend ? n - 1 + par : ctl->adam_t + par) & 1);
    const ScCache sce = sc_peek(x.scc, n);
    float* gr = x.g[n % 3];
    if (pend) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && x.loss_hist != nullptr && x.hist_len > 0) {
            const int64_t b = ctl->batch - 1;
            x.loss_hist[((b % x.hist_len) + x.hist_len) % x.hist_len] = gr[loss_i];
        }
        sc_resolve(sce, n, x.lr, x.beta1, x.beta2, sc);
        step_scalars_ahead(x.scc, n, x.lr, x.beta1, x.beta2);
    }
    __syncthreads();
    if (!pend && rb == 0) return;  // block-uniform: already in buffer 0
    const float neg_step = sc[0], bc2s = sc[1];
    const float w1 = (float)(1.0 - x.beta1), b2 = (float)x.beta2, omb2 = (float)(1.0 - x.beta2);
    const int64_t total = x.R.prefix[x.R.n];
    const f4 z = f4{0.f, 0.f, 0.f, 0.f};
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        int which;
        const int64_t i = range_locate(x.R, q, &which);
        f4 pp = *reinterpret_cast<const f4*>(x.p[rb] + i), mm = *reinterpret_cast<const f4*>(x.m[rb] + i),
           vv = *reinterpret_cast<const f4*>(x.v[rb] + i);
        if (pend) {
            const f4 gg = *reinterpret_cast<const f4*>(gr + i);
            adam_f4(pp, mm, vv, gg, w1, b2, omb2, bc2s, x.eps, neg_step);
            *reinterpret_cast<f4*>(gr + i) = z;
        }
        *reinterpret_cast<f4*>(x.p[0] + i) = pp;
        *reinterpret_cast<f4*>(x.m[0] + i) = mm;
        *reinterpret_cast<f4*>(x.v[0] + i) = vv;
    }
    if (pend && blockIdx.x == 0 && threadIdx.x == 0) gr[loss_i] = 0.f;
}

__global__ void ais_flush_done_kernel(ncf_step_ctl* ctl, int64_t* st) {
    if (threadIdx.x == 0) {
        const int64_t t = ctl->adam_t + st[0];
        ctl->adam_t = t;
        st[0] = 0;
        st[1] = t & 1;
    }
}

static int ais_args(const ncf_layout* lay, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                    const ncf_ais_bufs* b, const int64_t* ranges, int nranges, AisArgs* x) {
    if (!lay || !params || !grads || !exp_avg || !exp_avg_sq || !b || !ranges) return NCF_E_ARG;
    if (!b->params_b || !b->exp_avg_b || !b->exp_avg_sq_b || !b->grads_1 || !b->grads_2 || !b->state) return NCF_E_ARG;
    memset(x, 0, sizeof(*x));
    int err = 0;
    x->R = make_ranges(ranges, nranges, &err);
    if (err) return NCF_E_ARG;
    for (int i = 0; i < nranges; ++i)  // every active float inside the flat buffers
        if (ranges[2 * i + 1] > lay->total) return NCF_E_ARG;
    x->p[0] = params;
    x->p[1] = b->params_b;
    x->m[0] = exp_avg;
    x->m[1] = b->exp_avg_b;
    x->v[0] = exp_avg_sq;
    x->v[1] = b->exp_avg_sq_b;
    x->g[0] = grads;
    x->g[1] = b->grads_1;
    x->g[2] = b->grads_2;
    x->st = b->state;
    return NCF_OK;
}

static unsigned ais_grid(const Ranges& R, int64_t cap) {
    int64_t g = (R.prefix[R.n] + 255) / 256;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace ncf

extern "C" {

int ncf_ais_supported(const ncf_layout* lay) {
    int geo = 0;
    return (lay && ais_kernel(lay, &geo) != nullptr) ? 1 : 0;
}

int ncf_ais_begin(const ncf_layout* lay, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                  const ncf_ais_bufs* b, const int64_t* ranges, int nranges, ncf_step_ctl* ctl, void* stream) {
    AisArgs x;
    const int rc = ais_args(lay, params, grads, exp_avg, exp_avg_sq, b, ranges, nranges, &x);
    if (rc != NCF_OK) return rc;
    if (!ctl) return NCF_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    const size_t bytes = (size_t)lay->total * 4;  // buffer 1 = buffer 0 (inactive floats stay equal)
    if (hipMemcpyAsync(b->params_b, params, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(b->exp_avg_b, exp_avg, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(b->exp_avg_sq_b, exp_avg_sq, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return NCF_E_LAUNCH;
    hipLaunchKernelGGL(ais_begin_kernel, dim3(ais_grid(x.R, 1024)), dim3(256), 0, st, ctl, b->state, grads, b->grads_1,
                       b->grads_2, x.R, lay->tower_begin + lay->tower_len);
    return launch_status();
}

int ncf_train_step_ais(const ncf_layout* lay, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                       const ncf_ais_bufs* b, const int64_t* ranges, int nranges, const uint64_t* rows,
                       const float* dlogit, ncf_step_ctl* ctl, int64_t batch_global, int dz_mode, float kd_wt,
                       float kd_wr, float kd_temp, double lr, double beta1, double beta2, double eps,
                       float* loss_hist, int64_t hist_len, int64_t step_i, void* stream) {
    AisArgs x;
    int rc = ais_args(lay, params, grads, exp_avg, exp_avg_sq, b, ranges, nranges, &x);
    if (rc != NCF_OK) return rc;
    if (!rows || !ctl || batch_global <= 0 || step_i < 0) return NCF_E_ARG;
    // (NCF_DZ_BPR is refused here: the pairwise mode runs the two-launch step only)
    if (dz_mode != NCF_DZ_BCE && dz_mode != NCF_DZ_DLOGIT && dz_mode != NCF_DZ_KD) return NCF_E_ARG;
    if (dz_mode != NCF_DZ_BCE && !dlogit) return NCF_E_ARG;
    int geo = 0;
    const void* fn = ais_kernel(lay, &geo);
    if (!fn) return NCF_E_UNSUPPORTED;
    const KernelEntry* e = train_fused(lay);
    const int64_t lds = train_lds_floats(e, lay, geo) * 4;
    if (lds > LDS_LIMIT_BYTES) return NCF_E_UNSUPPORTED;
    if (ensure_lds(fn, lds) != NCF_OK) return NCF_E_LAUNCH;
    x.lr = lr;
    x.beta1 = beta1;
    x.beta2 = beta2;
    x.eps = (float)eps;
    x.loss_hist = loss_hist;
    x.hist_len = hist_len;
    x.scc = sc_cache_for(ctl, stream);
    x.step_i = step_i;
    x.ntrain = slab_rows_of(lay);
    TrainArgs a;
    memset(&a, 0, sizeof(a));
    a.lay = *lay;
    a.params = params;
    a.grads = grads;
    a.rows = rows;
    a.dlogit = dz_mode != NCF_DZ_BCE ? dlogit : reinterpret_cast<const float*>(rows);
    a.ctl = ctl;
    a.batch_global = batch_global;
    a.world = 1;
    a.rank = 0;
    a.dz_mode = dz_mode;
    a.kd_wt = kd_wt;
    a.kd_wr = kd_wr;
    a.kd_temp = kd_temp;
    a.diag = g_diag;
    a.stamps = g_stamps;
    a.ais = x;
    // the dense update over every active float by the workgroups past the training ones:
    // a few, so their bursts of loads do not queue ahead of the training workgroups'
    // dependent round trips (NCF_AIS_EXTRA, default 192)
    static const int extra_cap = [] {
        const char* e = getenv("NCF_AIS_EXTRA");
        const int v = e ? atoi(e) : 192;
        return v < 1 ? 1 : (v > 1024 ? 1024 : v);
    }();
    const int64_t t4 = x.R.prefix[x.R.n];  // float4 of the update; two per thread
    int64_t extra = (t4 + 2 * 256 - 1) / (2 * 256);
    if (extra > extra_cap) extra = extra_cap;
    if (extra < 1) extra = 1;
    void* args[] = {&a};  // + 1: the step-scalar workgroup (ais_dense_block)
    if (hipLaunchKernel(fn, dim3((unsigned)(x.ntrain + extra + 1)), dim3(geo_waves(geo) * WAVE), args,
                        (size_t)lds, (hipStream_t)stream) != hipSuccess)
        return NCF_E_LAUNCH;
    return launch_status();
}

int ncf_ais_bump(ncf_step_ctl* ctl, const ncf_ais_bufs* b, int64_t k, void* stream) {
    if (!ctl || !b || !b->state || k < 1) return NCF_E_ARG;
    hipLaunchKernelGGL(ais_bump_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ctl, b->state, k);
    return launch_status();
}

int ncf_ais_flush(const ncf_layout* lay, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                  const ncf_ais_bufs* b, const int64_t* ranges, int nranges, ncf_step_ctl* ctl, double lr,
                  double beta1, double beta2, double eps, float* loss_hist, int64_t hist_len, void* stream) {
    AisArgs x;
    const int rc = ais_args(lay, params, grads, exp_avg, exp_avg_sq, b, ranges, nranges, &x);
    if (rc != NCF_OK) return rc;
    if (!ctl) return NCF_E_ARG;
    x.lr = lr;
    x.beta1 = beta1;
    x.beta2 = beta2;
    x.eps = (float)eps;
    x.loss_hist = loss_hist;
    x.hist_len = hist_len;
    x.scc = sc_cache_for(ctl, stream);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ais_flush_kernel, dim3(ais_grid(x.R, 1024)), dim3(256), 0, st, x, ctl,
                       lay->tower_begin + lay->tower_len);
    if (launch_status() != NCF_OK) return NCF_E_LAUNCH;
    hipLaunchKernelGGL(ais_flush_done_kernel, dim3(1), dim3(64), 0, st, ctl, b->state);
    return launch_status();
}

int ncf_forward(const ncf_layout* lay, const float* params, const uint64_t* rows, int64_t n, float* logits,
                void* workspace, int64_t workspace_bytes, void* stream) {
    if (!lay || !params || !rows || !logits || n < 0) return NCF_E_ARG;
    if (n == 0) return NCF_OK;
    const KernelEntry* e = find_entry(lay->model_type, lay->factor_num, lay->num_layers);
    if (!fused_entry(lay)) {
        if (!workspace || workspace_bytes < ncf_forward_workspace_bytes(lay, n)) return NCF_E_ARG;
        LyrArgs la;
        memset(&la, 0, sizeof(la));
        la.lay = *lay;
        la.params = params;
        la.rows = rows;
        la.fwd_n = n;
        la.world = 1;
        la.logits_out = logits;
        la.fact_part_floats = -1;
        return lyr_run(la, static_cast<float*>(workspace), n, false, (hipStream_t)stream);
    }
    const int64_t lds = (int64_t)(e->w_total + e->misc[GEO_8]) * 4;
    if (lds > LDS_LIMIT_BYTES) return NCF_E_UNSUPPORTED;
    if (ensure_lds(e->fwd, lds) != NCF_OK) return NCF_E_LAUNCH;
    TrainArgs a;
    memset(&a, 0, sizeof(a));
    a.lay = *lay;
    a.params = params;
    a.rows = rows;
    a.logits_out = logits;
    a.fwd_n = n;
    a.world = 1;
    const int64_t ntiles = (n + TILE_ROWS - 1) / TILE_ROWS;
    const int grid = (int)(ntiles < 2 * SLAB_ROWS ? ntiles : 2 * SLAB_ROWS);
    void* args[] = {&a};
    if (hipLaunchKernel(e->fwd, dim3(grid), dim3(NTHREADS), args, (size_t)lds, (hipStream_t)stream) != hipSuccess)
        return NCF_E_LAUNCH;
    return launch_status();
}

int64_t ncf_slab_stride(const ncf_layout* lay) { return lay ? lay->tower_len + 64 : -1; }

}  // extern "C"
