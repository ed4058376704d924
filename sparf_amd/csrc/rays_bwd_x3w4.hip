// Data-gradient kernel of ray-gradient-only passes, bf16x3 mode, 4 waves / 128-row workgroup tiles: the geometry the plan picks for launches
// whose row count leaves the 256-row kernel's last round mostly empty (the code is mlp_bwd_impl.h).
#include "mlp_bwd_impl.h"

template int sparf::launch_mlp_bwd_t<sparf::PREC_X3, true, 4, sparf::FWD_SAVE_MASKS>(const sparf::MlpBwdArgs&, int, hipStream_t);
