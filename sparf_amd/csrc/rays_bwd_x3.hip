// Data-gradient kernel of ray-gradient-only passes, bf16x3 mode, 8 waves / 256-row workgroup tiles (the code is mlp_bwd_impl.h).
#include "mlp_bwd_impl.h"

template int sparf::launch_mlp_bwd_t<sparf::PREC_X3, true, 8, sparf::FWD_SAVE_MASKS>(const sparf::MlpBwdArgs&, int, hipStream_t);
