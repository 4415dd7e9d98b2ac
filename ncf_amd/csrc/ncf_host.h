// Host helpers shared by the translation units behind the C ABI (include/ncf_hip.h):
// launch plumbing and the layout geometry every entry point has to agree on.  Each is
// defined once, in the file named here, next to the process-wide state it owns (the
// ensure_lds slots, the step-scalar cache map, the ncf_debug_set_* values).
#pragma once
#include "ncf_adam.h"
#include "ncf_kernels.h"
#include "ncf_layered.h"

namespace ncf {

constexpr int UO_MAX_USERS = 32767;  // user_order_kernel's LDS histogram (ncf_prep.hip)

// ncf_step.hip: launch plumbing and the debug switches
int launch_status();
int ensure_lds(const void* fn, int64_t bytes);  // hipFuncSetAttribute once per (kernel, size)
Ranges make_ranges(const int64_t* ranges, int nranges, int* err);
int diag_flags();  // ncf_debug_set_diag's value

// Workspace layouts: every piece starts on a 256-byte boundary
inline int64_t ws_align(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }

// Materialised paths (ncf_recommend, ncf_select_negatives): packed rows, their logits and
// ncf_forward's own workspace for chunks of at most `pairs` (user, item) pairs.
struct MatWs {
    int64_t rows, logits, fwd, fwd_bytes, total;
};
inline MatWs mat_ws(const ncf_layout* lay, int64_t pairs) {
    MatWs w;
    w.rows = 0;
    w.logits = ws_align(pairs * 8);
    w.fwd = w.logits + ws_align(pairs * 4);
    w.fwd_bytes = ncf_forward_workspace_bytes(lay, pairs);
    w.total = w.fwd + ws_align(w.fwd_bytes);
    return w;
}

// Fused paths: the layer-0 projections Pi [item_num][kp0], Pu [user_rows][kp0] and
// Ag [user_rows][fp] (rc_proj_kernel, ncf_tower_tile.h); total = the first byte after them.
struct ProjWs {
    int64_t pi, pu, ag, total;
};
inline ProjWs proj_ws(const ncf_layout* lay, int64_t user_rows, int kp0, int fp) {
    ProjWs w;
    w.pi = 0;
    w.pu = ws_align((int64_t)lay->item_num * kp0 * 4);
    w.ag = w.pu + ws_align(user_rows * kp0 * 4);
    w.total = w.ag + ws_align(user_rows * fp * 4);
    return w;
}

// ncf_step.hip: layout geometry
const KernelEntry* train_fused(const ncf_layout* lay);  // fused kernel of a training step, or null (layered)
int fact_dm(const ncf_layout* lay);
bool fact_mode(const ncf_layout* lay);
int slab_lo(const ncf_layout* lay);
int reduce_rows(const ncf_layout* lay);
bool us_on(const ncf_layout* lay);
float* fact_w0_snap(const ncf_layout* lay, void* workspace);
W0Part w0_part(const ncf_layout* lay, const void* workspace);

// ncf_fact.hip: the factored layer-0 expansion
int fact_blocks(const ncf_layout* lay, int* nbu);
int64_t fact_partials_floats(const ncf_layout* lay);
int launch_fact_expand(const ncf_layout* lay, const float* params, float* grads, float* partials, float* w0snap,
                       hipStream_t st);

// ncf_optim.hip: the step-scalar cache entry pair of a control block (g_sc_cache); the slab
// reduction into out[slab_lo .. stride) (launch only: the caller checks launch_status)
ScCache* sc_cache_for(const void* ctl, void* stream);
void launch_reduce_slab(const ncf_layout* lay, const void* workspace, float* out, ncf_step_ctl* ctl, hipStream_t st);

}  // namespace ncf
