// Fused NeRF MLP kernels: the dispatch.  Host code only: this unit must not see mlp_fwd_impl.h / mlp_bwd_impl.h (it would
// instantiate every kernel of kernels.h' lists a second time); the launchers it looks up live in the units that instantiate them.
#include "kernels.h"

namespace sparf {

// save: FWD_INFER (nothing saved), FWD_SAVE_PLANES, FWD_SAVE_Q8, FWD_SAVE_MASKS (kernels.h)
int launch_mlp_fwd(int prec, int save, const MlpFwdArgs& a, int grid, hipStream_t stream) {
    const MlpFwdKernel* k = find_mlp_fwd(prec, save);
    return k ? k->launch(a, grid, stream) : 1;
}

// save: what the forward of the pass left; waves: the kernel's workgroup geometry (kernels.h MlpBwdKernel)
int launch_mlp_bwd(int prec, bool pose, int save, int waves, const MlpBwdArgs& a, int grid, hipStream_t stream) {
    const MlpBwdKernel* k = find_mlp_bwd(prec, pose, waves, save);
    return k ? k->launch(a, grid, stream) : 1;
}

}  // namespace sparf
