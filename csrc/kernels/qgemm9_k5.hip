// Mode-9 kernels of type-set 5 (MXFP4; see qgemm9_impl.h); one TU per set, as qgemv_k5.hip / qgemm_k5.hip.
#include "qgemm9_impl.h"

namespace nls_q9 {
int launch_q9_k5(int waves, int rt, int bm, const SegList& sl, int ntiles, int ks, float* ws, const GemvArgs& a,
                 hipStream_t st) {
  return launch_k<5>(waves, rt, bm, sl, ntiles, ks, ws, a, st);
}
}  // namespace nls_q9
