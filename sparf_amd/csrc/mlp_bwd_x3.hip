// Data-gradient kernels of the bf16x3 mode, 8 waves / 256-row workgroup tiles (the code is mlp_bwd_impl.h):
// weights head + tail, propagated gradient in bf16 (mlp_dev.h PolicyX3DgradT).  The full head + tail backward of round 2: code retired, last in ebe6c54.
#include "mlp_bwd_impl.h"

template int sparf::launch_mlp_bwd_t<sparf::PREC_X3, true, 8, sparf::FWD_SAVE_PLANES>(const sparf::MlpBwdArgs&, int, hipStream_t);
template int sparf::launch_mlp_bwd_t<sparf::PREC_X3, false, 8, sparf::FWD_SAVE_PLANES>(const sparf::MlpBwdArgs&, int, hipStream_t);

#ifdef SP_PROF      // wave-time accounting of THIS unit's kernels (each translation unit has its own g_prof_bwd): tools/kernel_bench.py bf16x3
extern "C" int sparf_debug_prof_bwd(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(sparf::g_prof_bwd), 10 * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
#endif
