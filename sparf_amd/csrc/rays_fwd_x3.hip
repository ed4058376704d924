// Fused NeRF MLP forward, x3 kernel of a ray-gradient-only pass: leaves the ReLU mask words only (layout.h AREA_MASKS); the code is mlp_fwd_impl.h.
#define SP_FWD_PREC sparf::PREC_X3
#define SP_FWD_SAVE sparf::FWD_SAVE_MASKS
#define SP_FWD_LAUNCHER launch_mlp_fwd_x3_masks
#define SP_FWD_PROF_EXPORT 0
#include "mlp_fwd_impl.h"
