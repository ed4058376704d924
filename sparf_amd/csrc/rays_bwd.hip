// Data-gradient kernel of ray-gradient-only passes (sparf_hip.h SPARF_SAVE_MASKS), bf16 mode.  The code is mlp_bwd_impl.h with
// P = RaysOnly<...> (mlp_dev.h): the pose variant of the precision's kernel over a masks-only save area, without the dY stores (a.grad is not read).
#include "mlp_bwd_impl.h"

template int sparf::launch_mlp_bwd_t<sparf::PREC_BF16, true, 8, sparf::FWD_SAVE_MASKS>(const sparf::MlpBwdArgs&, int, hipStream_t);
