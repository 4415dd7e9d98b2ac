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

// ncf_debug_set_*_path of a serving entry point: *g = 0 (by shape) or NCF_PATH_LAYERED
inline int set_debug_path(int* g, int path) {
    if (path != 0 && path != NCF_PATH_LAYERED) return NCF_E_ARG;
    *g = path;
    return NCF_OK;
}

// Rows of Pu / Ag where a fused kernel gathers them per pair: the call's n rows when they are
// fewer than the users (by_row: row = the call's row), else the user table (row = user id).
struct UserRows {
    int64_t R;
    int by_row;
};
inline UserRows serve_user_rows(const ncf_layout* lay, int64_t n) {
    return n < lay->user_num ? UserRows{n, 1} : UserRows{(int64_t)lay->user_num, 0};
}

// Materialised paths (ncf_recommend, ncf_select_negatives, ncf_rank_candidates,
// ncf_target_ranks): packed rows, their logits and ncf_forward's own workspace for chunks of at most `pairs` (user, item)
// pairs.  (ws_align is in ncf_common.h, the fused paths' proj_ws in ncf_tower_tile.h.)
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

// The materialised loop over [0, total) in chunks [b, b + c) of at most `chunk` units:
// make_rows(b, c, rows) launches the rows kernel and returns its pair count, ncf_forward scores
// them -- into the workspace's logit buffer, reused, or with all_logits (units = pairs) into
// all_logits + b -- and consume(b, c, those logits) launches their reader.  The first
// ncf_forward failure, else NCF_OK (the caller ends with launch_status).
template <class MakeRows, class Consume>
int mat_run(const ncf_layout* lay, const float* params, const MatWs& W, char* ws, float* all_logits, int64_t total,
            int64_t chunk, void* stream, MakeRows make_rows, Consume consume) {
    uint64_t* rows = reinterpret_cast<uint64_t*>(ws + W.rows);
    void* fws = W.fwd_bytes ? ws + W.fwd : nullptr;
    for (int64_t b = 0; b < total; b += chunk) {
        const int64_t c = total - b < chunk ? total - b : chunk;
        const int64_t pairs = make_rows(b, c, rows);
        float* lg = all_logits ? all_logits + b : reinterpret_cast<float*>(ws + W.logits);
        const int rc = ncf_forward(lay, params, rows, pairs, lg, fws, W.fwd_bytes, stream);
        if (rc != NCF_OK) return rc;
        consume(b, c, lg);
    }
    return NCF_OK;
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
