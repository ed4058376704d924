// Fused NeRF MLP forward, x3 training (activation-saving) kernel; the code is mlp_fwd_impl.h.
#include "mlp_fwd_impl.h"

template int sparf::launch_mlp_fwd_t<sparf::PREC_X3, sparf::FWD_SAVE_PLANES>(const sparf::MlpFwdArgs&, int, hipStream_t);

#ifdef SP_PROF      // wave-time accounting of THIS unit's kernel (each translation unit has its own g_prof): tools/kernel_bench.py bf16x3
extern "C" int sparf_debug_prof(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(sparf::g_prof), 10 * sizeof(unsigned long long)) == hipSuccess ? 0 : 1;
}
#endif
