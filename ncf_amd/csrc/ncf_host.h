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
