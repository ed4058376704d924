// Data-gradient kernels over 8-bit save / gradient areas (layout.h AREA_Q8; the code is mlp_bwd_impl.h): the bf16-operand modes
// (bf16x3: weights head + tail, propagated gradient in bf16, 256-row tiles, as in mlp_bwd_x3.hip).
#include "mlp_bwd_impl.h"

template int sparf::launch_mlp_bwd_t<sparf::PREC_BF16, true, 8, sparf::FWD_SAVE_Q8>(const sparf::MlpBwdArgs&, int, hipStream_t);
template int sparf::launch_mlp_bwd_t<sparf::PREC_BF16, false, 8, sparf::FWD_SAVE_Q8>(const sparf::MlpBwdArgs&, int, hipStream_t);
template int sparf::launch_mlp_bwd_t<sparf::PREC_X3, true, 8, sparf::FWD_SAVE_Q8>(const sparf::MlpBwdArgs&, int, hipStream_t);
template int sparf::launch_mlp_bwd_t<sparf::PREC_X3, false, 8, sparf::FWD_SAVE_Q8>(const sparf::MlpBwdArgs&, int, hipStream_t);
