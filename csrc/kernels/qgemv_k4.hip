// Quantised GEMV/GEMM kernels of type-set 4 (ggml IQ4_NL / IQ4_XS as QT_IQ4, with the Q5_K, Q6_K and Q8_0 tensors
// their mixes carry; see qgemv_impl.h); one TU per set so the instantiations compile in parallel.
#include "qgemv_impl.h"

namespace nls_gemv {
int launch_k4(int mode, int waves, int rt, int mt, const SegList& sl, int tiles, int ks, float* ws,
               const GemvArgs& a, hipStream_t st, int nmb) {
  return launch_kset<4>(mode, waves, rt, mt, sl, tiles, ks, ws, a, st, nmb);
}
}  // namespace nls_gemv
