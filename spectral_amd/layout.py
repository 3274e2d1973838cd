"""HBM data layout of a candidate batch (mirrors include/btrapz_hip.h).

One candidate = S segment records (the reference's `Cube`, cube_type.h:2-24, plus the
per-segment quantities its assembly derives: ds bounds from solve_3d.cc:835-845 and the
piecewise-linear reference of solve_3d.cc:1159-1166).  Stored field-major (SoA):

    seg[f][b][k]   f = field, b = candidate, k = segment        float64

so that the lanes of a wavefront (lane = segment, consecutive candidates packed into
one wave) read consecutive addresses for every field.
"""
from dataclasses import dataclass, field

import numpy as np

(F_T, F_DOWN_BIAS, F_DOWN_SKEW, F_UPP_BIAS, F_UPP_SKEW, F_L_DOWN_BIAS, F_L_DOWN_SKEW,
 F_L_UPP_BIAS, F_L_UPP_SKEW, F_BEG_L, F_END_L, F_DS_LO, F_DS_HI, F_X_SKEW, F_X_BIAS,
 F_Y_SKEW, F_Y_BIAS) = range(17)
NUM_SEG_FIELDS = 17
MAX_SEGMENTS = 64

# OSQP status_val vocabulary (the reference accepts 1 and 2: solve_3d.cc:1253)
STATUS_SOLVED = 1
STATUS_SOLVED_INACCURATE = 2
STATUS_MAX_ITER = -2
STATUS_PRIMAL_INFEASIBLE = -3
FAIL_SENTINEL = 100000000000.0  # trp_wrapper.cpp:199


@dataclass
class Shared:
    """Weights and limits shared by every candidate of a batch (Params + file header)."""
    w_s: tuple  # weight_s_ref, weight_ds_ref, s_acc_weight, s_jerk_weight
    w_l: tuple
    weight_end_s: float
    weight_end_l: float
    ds_ref: float
    dl_ref: float
    dds: tuple
    ddds: tuple
    ddl: tuple
    dddl: tuple
    delta: float = 0.1
    variant: int = 0  # 0 trapezoid (solve_3d.cc), 1 cuboid (cuboid_3d.cc)

    def as_array(self):
        return np.array([*self.w_s, *self.w_l, self.weight_end_s, self.weight_end_l, self.ds_ref,
                         self.dl_ref, *self.dds, *self.ddds, *self.ddl, *self.dddl, self.delta],
                        dtype=np.float64)


@dataclass
class Batch:
    B: int
    S: int
    seg: np.ndarray       # [NUM_SEG_FIELDS][B][S]
    init: np.ndarray      # [B][6]  s0 ds0 dds0 l0 dl0 ddl0
    ref_end: np.ndarray   # [B][2]  x_ref[N-1], y_ref[N-1]   (solve_3d.cc:268,315)
    dl_bounds: np.ndarray  # [B][10] dy_bounds_[i], i=0..4 as lo,hi (solve_3d.cc:1003-1004)

    def slice(self, lo, hi):
        return Batch(B=hi - lo, S=self.S, seg=np.ascontiguousarray(self.seg[:, lo:hi]),
                     init=np.ascontiguousarray(self.init[lo:hi]),
                     ref_end=np.ascontiguousarray(self.ref_end[lo:hi]),
                     dl_bounds=np.ascontiguousarray(self.dl_bounds[lo:hi]))

    def algorithmic_bytes(self):
        """Bytes one solve must move: inputs + 12S control points + cost + status."""
        S = self.S
        return (NUM_SEG_FIELDS * S + 6 + 2 + 10) * 8 + 12 * S * 8 + 8 + 4


REFLINE_FIELDS = ("rs", "rx", "ry", "rtheta", "rkappa", "rdkappa")


class Obstacles:
    """The moving obstacles of the clearance stage (btrapz_obstacles, include/btrapz_hip_clearance.h): n_scenes scenes of up
    to O rectangles at n samples.  pose: [O, 3, n] (one scene) or [n_scenes, O, 3, n], rows (x, y, theta), column j being
    the obstacle at the time of sample j of the rows it is checked against (aligning the two is the caller's); a NaN in a
    column means the obstacle is absent there.  half: [O, 2] or [n_scenes, O, 2], (half_length, half_width).  obs_count:
    [n_scenes] or None (every scene has O).  Host arrays or device tensors.  The constructor checks the shapes and that
    every half extent is > 0 and finite (the device does not), on a host copy it keeps as .host; .on(device) uploads once
    per device and hands the same tensors out afterwards."""

    def __init__(self, pose, half, obs_count=None):
        self._given = dict(pose=pose, half=half, obs_count=obs_count)
        to_host = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else a
        p = np.ascontiguousarray(to_host(pose), dtype=np.float64)
        h = np.ascontiguousarray(to_host(half), dtype=np.float64)
        if p.ndim == 3:
            p = p[None]
        if h.ndim == 2:
            h = h[None]
        if p.ndim != 4 or p.shape[2] != 3 or min(p.shape) < 1:
            raise ValueError("Obstacles: pose is [O, 3, n] or [n_scenes, O, 3, n] with every extent >= 1, not %s" % (p.shape,))
        self.n_scenes, self.O, _, self.n = p.shape
        if h.shape != (self.n_scenes, self.O, 2):
            raise ValueError("Obstacles: half is %s for this pose, not %s" % ((self.n_scenes, self.O, 2), h.shape))
        if not bool((np.isfinite(h) & (h > 0)).all()):
            raise ValueError("Obstacles: every half extent must be > 0 and finite")
        c = None
        if obs_count is not None:
            c = np.ascontiguousarray(to_host(obs_count), dtype=np.int32)
            if c.shape != (self.n_scenes,):
                raise ValueError("Obstacles: obs_count is [n_scenes] = %s, not %s" % ((self.n_scenes,), c.shape))
        self.host = dict(pose=p, half=h, obs_count=c)
        self._device = {}

    def on(self, device):
        """(pose, half, obs_count or None) as contiguous tensors on `device`, uploaded the first time."""
        import torch
        device = torch.device(device)
        if device not in self._device:
            out = []
            for k, dtype in (("pose", torch.float64), ("half", torch.float64), ("obs_count", torch.int32)):
                a = self._given[k]
                if a is None:
                    out.append(None)
                elif torch.is_tensor(a) and a.device == device and a.dtype == dtype and a.is_contiguous():
                    out.append(a.detach().reshape(self.host[k].shape))
                else:
                    out.append(torch.from_numpy(self.host[k]).to(device))
            self._device[device] = tuple(out)
        return self._device[device]


class RefLine:
    """The reference-line table of the Cartesian stage (btrapz_refline, include/btrapz_hip_cartesian.h): n_lines tables
    of M >= 2 points each -- arc length rs (strictly increasing within a line), position rx, ry, heading rtheta,
    curvature rkappa and its derivative rdkappa.  Each array is [M] (one line) or [n_lines, M], a host array or a
    device tensor.  The constructor checks the shapes, M >= 2 and that rs increases (the device does not), on a host
    copy it keeps as .host; .on(device) uploads once per device and hands the same six tensors out afterwards."""

    def __init__(self, rs, rx, ry, rtheta, rkappa, rdkappa):
        given = dict(zip(REFLINE_FIELDS, (rs, rx, ry, rtheta, rkappa, rdkappa)))
        self._given = given
        host = {}
        for k, a in given.items():
            a = a.detach().cpu().numpy() if hasattr(a, "detach") else a
            a = np.ascontiguousarray(a, dtype=np.float64)
            host[k] = a[None, :] if a.ndim == 1 else a
            if host[k].ndim != 2 or host[k].shape != host["rs"].shape:
                raise ValueError("RefLine: %s has shape %s; every array is [M] or [n_lines, M] like rs %s"
                                 % (k, a.shape, host["rs"].shape))
        self.n_lines, self.M = host["rs"].shape
        if self.n_lines < 1 or self.M < 2:
            raise ValueError("RefLine: n_lines >= 1 and M >= 2 points per line, not %s" % (host["rs"].shape,))
        if not bool((np.diff(host["rs"], axis=1) > 0).all()):
            raise ValueError("RefLine: rs must be strictly increasing within every line")
        self.host = host
        self._device = {}

    def on(self, device):
        """The six arrays as contiguous float64 tensors [n_lines, M] on `device`, uploaded the first time."""
        import torch
        device = torch.device(device)
        if device not in self._device:
            out = []
            for k in REFLINE_FIELDS:
                a = self._given[k]
                if torch.is_tensor(a) and a.device == device and a.dtype == torch.float64 and a.is_contiguous():
                    out.append(a.detach().reshape(self.n_lines, self.M))
                else:
                    out.append(torch.from_numpy(self.host[k]).to(device))
            self._device[device] = tuple(out)
        return self._device[device]
