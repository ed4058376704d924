// Data-gradient kernels of the fp32 mode (the code is mlp_bwd_impl.h).
#include "mlp_bwd_impl.h"

template int sparf::launch_mlp_bwd_t<sparf::PREC_FP32, true, 4, sparf::FWD_SAVE_PLANES>(const sparf::MlpBwdArgs&, int, hipStream_t);
template int sparf::launch_mlp_bwd_t<sparf::PREC_FP32, false, 4, sparf::FWD_SAVE_PLANES>(const sparf::MlpBwdArgs&, int, hipStream_t);
