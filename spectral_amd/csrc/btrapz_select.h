// btrapz_select.h -- library-internal: what btrapz_select.hip (the K-best selection) needs of a context.
#ifndef BTRAPZ_SELECT_H
#define BTRAPZ_SELECT_H
#include <cstddef>
#include <string>

#include "btrapz_device.h"
#include "../../include/btrapz_hip_select.h"

// The context's workspace for `entries` partial (cost, index) entries, opened for a launch sequence on `stream` (it waits
// for the sequence before it when that ran on another stream).  Grown on demand; the contents are not kept.
int btrapz_ctx_select_workspace(btrapz_ctx *ctx, size_t entries, void *stream, double **cost, long long **idx);
// ... and closed behind the sequence's last launch.
int btrapz_ctx_workspace_close(btrapz_ctx *ctx, void *stream);
#endif
