// Data-gradient kernels of ray-gradient-only passes (sparf_hip.h SPARF_SAVE_MASKS): the launch dispatch, and the bf16 kernel.  The code is
// mlp_bwd_impl.h with P = RaysOnly<...> (mlp_dev.h): the pose variant of each precision's kernel over a masks-only save area, without the
// dY stores.  The other precisions are their own translation units (rays_bwd_fp32.hip, rays_bwd_x3.hip, rays_bwd_x3w4.hip), compiled in parallel.
#include "mlp_bwd_impl.h"

namespace sparf {

int launch_rays_bwd_fp32(const MlpBwdArgs& a, int grid, hipStream_t stream);             // rays_bwd_fp32.hip
int launch_rays_bwd_x3(const MlpBwdArgs& a, int grid, hipStream_t stream);               // rays_bwd_x3.hip   (8 waves, 256-row tiles)
int launch_rays_bwd_x3w4(const MlpBwdArgs& a, int grid, hipStream_t stream);             // rays_bwd_x3w4.hip (4 waves, 128-row tiles)

// waves: geometry of the bf16x3 kernel (8 | 4; kernels.h) -- ignored by the other precisions
int launch_mlp_bwd_rays(int prec, const MlpBwdArgs& a, int grid, hipStream_t stream, int waves) {
    if (a.rows <= 0) return 0;
    if (prec == PREC_FP32) return launch_rays_bwd_fp32(a, grid, stream);
    if (prec == PREC_X3) return waves == 4 ? launch_rays_bwd_x3w4(a, grid, stream) : launch_rays_bwd_x3(a, grid, stream);
    if (prec != PREC_BF16) return 1;
    typedef RaysOnly<Policy<PREC_BF16>> P;
    hipLaunchKernelGGL((mlp_bwd_kernel<PREC_BF16, true, P>), dim3(grid), dim3(P::NWAVES * 64), 0, stream, a);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace sparf
