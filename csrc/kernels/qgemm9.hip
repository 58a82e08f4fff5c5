// Mode 9 (qgemm9_impl.h): the kernels of type-sets 0, 1, 3 and 4 and the entry the dispatcher calls; set 5's kernels are
// qgemm9_k5.hip.
#include "qgemm9_impl.h"

namespace nls_q9 {

// waves x rt weight tiles of 16 rows per workgroup: (4, 2) | (8, 2) | (8, 1) (4 x 4 spills: 256 accumulators
// plus the pipelined fragments exceed 512 registers) over 256 activation rows; kset as the dispatcher's
int launch_q9(int kset, int waves, int rt, const SegList& sl, int ntiles, int ks, float* ws, const GemvArgs& a,
              hipStream_t st, int bm) {
  if (kset == 0) return launch_k<0>(waves, rt, bm, sl, ntiles, ks, ws, a, st);
  if (kset == 1) return launch_k<1>(waves, rt, bm, sl, ntiles, ks, ws, a, st);
  if (kset == 3) return launch_k<3>(waves, rt, bm, sl, ntiles, ks, ws, a, st);
  if (kset == 4) return launch_k<4>(waves, rt, bm, sl, ntiles, ks, ws, a, st);
  if (kset == 5) return launch_q9_k5(waves, rt, bm, sl, ntiles, ks, ws, a, st);
  return (int)hipErrorInvalidValue;
}

}  // namespace nls_q9
