// btrapz_grad_rule.h -- the constants and row macros of the kernels that differentiate a solve: vjp_kernel
// (btrapz_vjp.hip), jvp_kernel (btrapz_jvp.hip), long_vjp_kernel and long_jvp_kernel (btrapz_long_grad.hip).  The three
// files restate the method statement for statement (DESIGN 3.16 says why they are not one body); what they must agree
// on to the last digit stands here once.
#ifndef BTRAPZ_GRAD_RULE_H
#define BTRAPZ_GRAD_RULE_H
#include "btrapz_ipm.h"

// penalty of an active row: rho_r = GRAD_RHO times the lane's largest diagonal entry of P over |g_r|^2
#define GRAD_RHO 1e6
// passes of the method of multipliers on the one factorisation
#define GRAD_PASSES 3
// A multiplier that is no number classifies nothing.  The solve returns the control points of its BEST iterate and the
// multipliers of its LAST one, and the last one may be the non-finite iterate that ended the solve (a warm start
// sanitises such entries: btrapz_kernels.hip).  Such a row is classified by its slack alone, at the value the rule
// "multiplier above slack" takes on a solved candidate: lam s = mu <= 1e-7 (BTRAPZ_SOLVED), so lam > s where
// s < sqrt(1e-7).  Multipliers below 1e300 in size classify as before, bit for bit.
#define GRAD_SLACK_ACTIVE 3.1622776601683794e-4

#define HSYM(H, i, j) ((i) <= (j) ? H[SYM(i, j)] : H[SYM(j, i)])

// rows these kernels keep: those of the solve (rows_kept<false>: 1-5, 7-10, 12-17)
#define GRAD_ROWS(r) static_for<15>([&](auto r##_c) { constexpr int r = row_id<false>(decltype(r##_c)::value); constexpr int ri_ = state_index<false>(r); (void)ri_;
#define GRAD_END });

#endif
