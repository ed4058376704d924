// Data-gradient kernel of ray-gradient-only passes, fp32 mode (the code is mlp_bwd_impl.h; dispatch: rays_bwd.hip).
#include "mlp_bwd_impl.h"

namespace sparf {

int launch_rays_bwd_fp32(const MlpBwdArgs& a, int grid, hipStream_t stream) {
    typedef RaysOnly<Policy<PREC_FP32>> P;
    hipLaunchKernelGGL((mlp_bwd_kernel<PREC_FP32, true, P>), dim3(grid), dim3(P::NWAVES * 64), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace sparf
