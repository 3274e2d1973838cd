// btrapz_long_grad.h -- what btrapz_long_grad.hip's kernels share with the host code that launches them
// (btrapz_solve_long_vjp_device, btrapz_solve_long_jvp_device: include/btrapz_hip_long_grad.h).
#ifndef BTRAPZ_LONG_GRAD_H
#define BTRAPZ_LONG_GRAD_H
#include <hip/hip_runtime.h>

#include "btrapz_device.h"

namespace btrapz {

// One axis problem per workgroup of W = ceil(seg_stride / 64) wavefronts, 2 B workgroups, axis = blockIdx.x & 1.
// The arguments are those of vjp_kernel / jvp_kernel with S = seg_stride (65 .. BTRAPZ_MAX_SEGMENTS_LONG).
__global__ void long_vjp_kernel(const VjpArgs a);
// cost_ws: [2][T][B], each axis' share of cost_dot (null when cost_dot is not wanted)
__global__ void long_jvp_kernel(const JvpArgs a, double *cost_ws);
// cost_dot[i] = cost_ws[i] + cost_ws[n + i], i < n = T B: the s axis' share plus the l axis', in that order
__global__ void long_cost_dot_kernel(const double *cost_ws, double *cost_dot, unsigned n);

}  // namespace btrapz
#endif
