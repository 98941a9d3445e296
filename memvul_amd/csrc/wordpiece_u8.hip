// libmemvul_tok_u8.so: the UTF-8 tokenise kernel (wordpiece.h wp_encode_u8_kernel) in a code object of its own, and the one function that launches it.
// libmemvul_hip.so links against this library and calls wp_u8_launch from mv_tok_encode_u8 (tokenizer_object.h); nothing else is exported.  The kernel lives
// here, not in engine.hip, so that the set of kernels in libmemvul_hip.so — what build.kernel_fingerprints hashes and tests/golden/pass_fingerprints.json is
// keyed on — does not change with a kernel that no encoder pass launches.
#include <hip/hip_runtime.h>

#define WP_U8_KERNEL
#include "wordpiece.h"

// one chunk: m texts, one wave each, on `stream`; the tables and every buffer are device memory of the current device.  Returns hipGetLastError() of the launch.
extern "C" int wp_u8_launch(const WpTable* t, const WpU8* u, const uint8_t* text, const int64_t* off, int m, int max_length, int add_special, int32_t* ids,
                            int32_t* lens, uint8_t* status, hipStream_t stream) {
  hipLaunchKernelGGL(wp_encode_u8_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, stream, *t, *u, text, off, m, max_length, add_special ? 1 : 0, ids, lens, status);
  return (int)hipGetLastError();
}
