// Fused NeRF MLP forward, bf16x3 training kernel with 8-bit saves (layout.h AREA_Q8); the code is mlp_fwd_impl.h.
#include "mlp_fwd_impl.h"

template int sparf::launch_mlp_fwd_t<sparf::PREC_X3, sparf::FWD_SAVE_Q8>(const sparf::MlpFwdArgs&, int, hipStream_t);
