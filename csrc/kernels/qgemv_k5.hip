// Quantised GEMV/GEMM kernels of type-set 5 (ggml MXFP4 as QT_MXFP4, alone: the expert tensors of an MXFP4_MOE file
// share a launch with no other format; see gemv_args.h); one TU per set so the instantiations compile in parallel.
#include "qgemv_impl.h"

namespace nls_gemv {
int launch_k5(int mode, int waves, int rt, int mt, const SegList& sl, int tiles, int ks, float* ws,
               const GemvArgs& a, hipStream_t st, int nmb) {
  return launch_kset<5>(mode, waves, rt, mt, sl, tiles, ks, ws, a, st, nmb);
}
}  // namespace nls_gemv
