// Fused NeRF MLP forward, x3 inference kernel; the code is mlp_fwd_impl.h.
#include "mlp_fwd_impl.h"

template int sparf::launch_mlp_fwd_t<sparf::PREC_X3, sparf::FWD_INFER>(const sparf::MlpFwdArgs&, int, hipStream_t);
