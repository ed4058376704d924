// Data-gradient kernel of ray-gradient-only passes, bf16x3 mode, 8 waves / 256-row workgroup tiles (the code is mlp_bwd_impl.h; dispatch: rays_bwd.hip).
#include "mlp_bwd_impl.h"

namespace sparf {

int launch_rays_bwd_x3(const MlpBwdArgs& a, int grid, hipStream_t stream) {
    typedef RaysOnly<PolicyX3Dgrad> P;
    hipLaunchKernelGGL((mlp_bwd_kernel<PREC_X3, true, P>), dim3(grid), dim3(P::NWAVES * 64), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace sparf
