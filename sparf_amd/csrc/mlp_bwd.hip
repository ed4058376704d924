// Data-gradient kernels of the bf16 mode over plane save / gradient areas (the code is mlp_bwd_impl.h).
#include "mlp_bwd_impl.h"

template int sparf::launch_mlp_bwd_t<sparf::PREC_BF16, true, 8, sparf::FWD_SAVE_PLANES>(const sparf::MlpBwdArgs&, int, hipStream_t);
template int sparf::launch_mlp_bwd_t<sparf::PREC_BF16, false, 8, sparf::FWD_SAVE_PLANES>(const sparf::MlpBwdArgs&, int, hipStream_t);
