// Data-gradient kernel of ray-gradient-only passes, fp32 mode (the code is mlp_bwd_impl.h).
#include "mlp_bwd_impl.h"

template int sparf::launch_mlp_bwd_t<sparf::PREC_FP32, true, 4, sparf::FWD_SAVE_MASKS>(const sparf::MlpBwdArgs&, int, hipStream_t);
