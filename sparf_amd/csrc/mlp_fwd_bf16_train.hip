// Fused NeRF MLP forward, bf16 training (activation-saving) kernel; the code is mlp_fwd_impl.h.
#include "mlp_fwd_impl.h"

template int sparf::launch_mlp_fwd_t<sparf::PREC_BF16, sparf::FWD_SAVE_PLANES>(const sparf::MlpFwdArgs&, int, hipStream_t);
