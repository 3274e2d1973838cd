/* btrapz_hip_schedule.h -- test / analysis hooks of the schedule of the lean two-launch solve: a third
 * header beside btrapz_hip.h (which it includes), plain C99.
 *
 * A lean two-launch solve (btrapz_options.cap_iter, btrapz_last_solve_form() == 11) of a uniform batch in memory order
 * runs either as its two launches -- capped launch of both axes, resume launch of both axes -- or as three: the capped
 * launch of one axis, ONE grid of that axis's resume wavefronts and the other axis's capped launch, the other axis's
 * resume launch.  Both give the one-launch solve's results bit for bit; the schedule only moves time.  By default the
 * library chooses: three launches, with axis a first, when the context's last finished solve of the same shape
 * (segments, variant) handed over at least four times more problems of axis a than of the other one.  When it handed
 * over at least 256 times more, the other axis is QUIET: it is solved without the cap, by the one-launch body, in the
 * grid that carries axis a's resume wavefronts -- no lists, no bucketing and no resume launch for it.  Such a solve
 * remembers an estimate, from its iteration counts, of what the quiet axis would have handed over. */
#ifndef BTRAPZ_HIP_SCHEDULE_H
#define BTRAPZ_HIP_SCHEDULE_H
#include "btrapz_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The schedule of the lean two-launch solves that follow on this context -- 0 (default): chosen as above; -1: always the
 * two launches; 1 / 2: three launches with the s / l axis first; 3 / 4: the s / l axis first and the other axis quiet.
 * BTRAPZ_EINVAL for any other mode. */
int btrapz_debug_set_schedule(btrapz_ctx *ctx, int mode);
/* The number of solve-kernel launches the main step of the context's last batched solve made: 1, 2 or 3 (3 as well for
 * a quiet-axis schedule, whose third step is no launch: it tells the axis-first schedules from the two launches). */
int btrapz_debug_solve_launches(const btrapz_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
