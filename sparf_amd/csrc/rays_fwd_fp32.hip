// Fused NeRF MLP forward, fp32 kernel of a ray-gradient-only pass: leaves the ReLU mask words only (layout.h AREA_MASKS); the code is mlp_fwd_impl.h.
#include "mlp_fwd_impl.h"

template int sparf::launch_mlp_fwd_t<sparf::PREC_FP32, sparf::FWD_SAVE_MASKS>(const sparf::MlpFwdArgs&, int, hipStream_t);
