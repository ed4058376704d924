// Data-gradient kernels of the bf16x3 mode, 4 waves / 128-row workgroup tiles: the geometry the plan (pass_plan.h plan_dgrad) picks for launches
// whose row count leaves the 256-row kernel's last round of tiles mostly empty (small passes: a 512-ray step, i.e. a 4096-ray batch strong-scaled over
// 8 GPUs).  Same arithmetic, same tile-block areas, bit-identical results (tests/test_hip_gpu.py); 12-17 % slower per row than the
// 8-wave kernel at full occupancy (mlp_bwd_impl.h), which is why it is not the only one.
#include "mlp_bwd_impl.h"

template int sparf::launch_mlp_bwd_t<sparf::PREC_X3, true, 4, sparf::FWD_SAVE_PLANES>(const sparf::MlpBwdArgs&, int, hipStream_t);
template int sparf::launch_mlp_bwd_t<sparf::PREC_X3, false, 4, sparf::FWD_SAVE_PLANES>(const sparf::MlpBwdArgs&, int, hipStream_t);
