// The pairwise (NCF_DZ_BPR) instantiations of the fused step kernel: ncf_train.hip compiled
// a second time with only ncf_step_kernel<..., BPR = true> instantiated and
// kernel_table_bpr() in place of kernel_table().  A translation unit of its own, so the
// two compile side by side and the kernels of the other modes are built from exactly
// the code they were built from before.
#define NCF_TRAIN_BPR_TU
#include "ncf_train.hip"
