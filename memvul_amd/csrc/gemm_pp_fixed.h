// The two functions libmemvul_pp_fixed.so exports (gemm_pp_fixed.hip): the fixed-form persistent GEMMs of MV_F16X8.  libmemvul_hip.so links against that
// library and calls them from launch_pp (encoder_pass.h) and mv_create (engine.hip).
#pragma once
#include <hip/hip_runtime.h>

struct GemmArgs;

extern "C" {
// One launch of the fixed-form kernel of kind PP_QK / PP_GELU / PP_RESLN3 at padded length a->S (256 or 512) on `stream`: grid workgroups of 512 threads, lds
// bytes of dynamic LDS.  The caller has checked that the launch IS of the fixed form (encoder_pass.h pp_fixed_form): the kernel does not read the fields the
// form fixes.  Returns hipGetLastError() of the launch, or -1 when there is no kernel of that kind and length.
int pp_fixed_launch(int kind, const GemmArgs* a, int grid, int lds, hipStream_t stream);
// The dynamic-LDS opt-in of every kernel of the library on the current device (mv_create, next to GEMM_LDS_OPT_INS); returns the number of kernels.
int pp_fixed_lds_opt_in(void);
}
