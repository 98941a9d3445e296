// libmemvul_pp_fixed.so: the three MV_F16X8 persistent GEMMs (gemm_pp.h) in their FIXED form, in a code object of their own, and the function that launches them.
// libmemvul_hip.so links against this library; launch_pp (encoder_pass.h) comes here for the launches of a long pass in the [CLS]-row form and stays with its own
// kernels for every other launch.  The kernels live here, not in engine.hip, so that the kernels of libmemvul_hip.so — what build.kernel_fingerprints hashes
// and tests/golden/pass_fingerprints.json is keyed on — stay the bytes they were.
//
// What the form fixes.  The run-time kernels hold every form field of GemmArgs in SGPRs across the main loop and branch on it in the epilogues, and they are the only
// kernels of the project that spill.  In a pass of padded length 256 / 512 in the [CLS]-row form with no short sequence, one plane and MEMVUL_QKV_ASIDE=none the
// host knows all of these before the launch (encoder_pass.h pp_fixed_form), so here they are constants:
//   no row tile is short (tile_both is not read), x8_terms = 3 with an empty aside mask (PP_QK) / 1 (the others), out8_hi_only = 1 (PP_GELU) / 0 (PP_RESLN3),
//   no second planes (vt_lo, q_lo, k_lo), the grouped raster (raster_mode 0), S = the template value FS, and N = 3072 (PP_GELU) / 768 (PP_RESLN3).
// PP_QK keeps N and col0 at run time: one kernel serves the layer's QKV projection and the pruned last layer's K/V launch.  K stays at run time everywhere: as a
// constant it turns SGPR pressure into 150 - 230 bytes of VGPR scratch per lane (profiles/pp_fixed_form_kernel_resources.txt has every set that was compiled).
// Only where a value comes from changes: the statements of gemm_pp.h, their order and their roundings are the run-time kernels', token for token.
#include <hip/hip_runtime.h>

#define PP_KERNEL_NAME gemm_pp_fixed_kernel
#define PP_EXTRA_TPARAMS , int FS
#define PP_SHORT_TILE(a, tm) false
#define PP_X8_TERMS(a) (EPI == PP_QK ? 3 : 1)
#define PP_ASIDE_MASK(a) 0
#define PP_OUT8_HI_ONLY(a) (EPI == PP_GELU ? 1 : 0)
#define PP_VT_LO(a) ((half_t*)nullptr)
#define PP_Q_LO(a) ((half_t*)nullptr)
#define PP_K_LO(a) ((half_t*)nullptr)
#define PP_RASTER_MODE(a) 0
#define PP_S(a) FS
#define PP_N(a) (EPI == PP_GELU ? MV_INTER : EPI == PP_RESLN3 ? MV_HIDDEN : (a).N)
#include "gemm_pp.h"
#include "gemm_pp_fixed.h"

namespace {

template <int EPI, int FS>
constexpr auto fixed_kernel = gemm_pp_fixed_kernel<EPI, EPI != PP_RESLN3, 1, FS>;
template <int EPI>
constexpr int fixed_lds = EPI != PP_RESLN3 ? PP_LDS_BYTES_RAW : PP_LDS_BYTES;

struct FixedKernel { int kind, S; void (*kernel)(GemmArgs); int lds; };
constexpr FixedKernel FIXED_KERNELS[] = {
    {PP_QK, 256, fixed_kernel<PP_QK, 256>, fixed_lds<PP_QK>},             {PP_QK, 512, fixed_kernel<PP_QK, 512>, fixed_lds<PP_QK>},
    {PP_GELU, 256, fixed_kernel<PP_GELU, 256>, fixed_lds<PP_GELU>},       {PP_GELU, 512, fixed_kernel<PP_GELU, 512>, fixed_lds<PP_GELU>},
    {PP_RESLN3, 256, fixed_kernel<PP_RESLN3, 256>, fixed_lds<PP_RESLN3>}, {PP_RESLN3, 512, fixed_kernel<PP_RESLN3, 512>, fixed_lds<PP_RESLN3>},
};

}  // namespace

extern "C" int pp_fixed_launch(int kind, const GemmArgs* a, int grid, int lds, hipStream_t stream) {
  if (!a || grid <= 0) return -1;
  for (const FixedKernel& k : FIXED_KERNELS)
    if (k.kind == kind && k.S == a->S && k.lds == lds) {
      hipLaunchKernelGGL(k.kernel, dim3((unsigned)grid), dim3(512), (size_t)lds, stream, *a);
      return (int)hipGetLastError();
    }
  return -1;
}

extern "C" int pp_fixed_lds_opt_in(void) {
  int n = 0;
  for (const FixedKernel& k : FIXED_KERNELS) {
    hipFuncSetAttribute((const void*)k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds);
    ++n;
  }
  (void)hipGetLastError();
  return n;
}
