// Data-gradient kernel of ray-gradient-only passes, bf16x3 mode, 4 waves / 128-row workgroup tiles: the geometry api.hip picks for launches
// whose row count leaves the 256-row kernel's last round mostly empty (the code is mlp_bwd_impl.h; dispatch: rays_bwd.hip).
#include "mlp_bwd_impl.h"

namespace sparf {

int launch_rays_bwd_x3w4(const MlpBwdArgs& a, int grid, hipStream_t stream) {
    typedef RaysOnly<PolicyX3DgradW4> P;
    hipLaunchKernelGGL((mlp_bwd_kernel<PREC_X3, true, P>), dim3(grid), dim3(P::NWAVES * 64), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace sparf
