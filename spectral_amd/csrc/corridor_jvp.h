// corridor_jvp.h -- the launch arguments of corridor_jvp_kernel (corridor_jvp.hip), shared with the host entry point
// btrapz_corridor_batch_jvp_device (btrapz_host.hip).
#ifndef BTRAPZ_CORRIDOR_JVP_H
#define BTRAPZ_CORRIDOR_JVP_H

#include <hip/hip_runtime.h>

namespace btrapz {

// The forward-mode derivative of the wave-wide corridor stage.  The decision phases, the two passes and the LDS layout are
// the backward pass's (CorridorVjpArgs, corridor_vjp_lds: btrapz_device.h); corridor_decide.h reads the fields of the same
// names from either struct.
struct CorridorJvpArgs {
  int B, N, num_obs, variant, seg_stride, T;
  double delta;
  const double *s_bounds, *l_bounds, *ds_bounds, *s_ref, *l_ref;
  const double *s_dot, *l_dot, *ds_dot, *dl_knots_dot, *sref_dot, *lref_dot;   // tangents, leading axis T; any may be null
  double *seg_dot, *ref_end_dot, *dl10_dot;                                    // outputs, leading axis T; any may be null
  int cap_o, cap_sel, pass, staged;                                            // as CorridorVjpArgs
  int *retry_list, *retry_count;
};
__global__ void corridor_jvp_kernel(const CorridorJvpArgs a);

}  // namespace btrapz
#endif
