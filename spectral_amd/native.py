"""ctypes binding of libbtrapz_hip.so (include/btrapz_hip.h).

The library is the product; this module only marshals pointers.  There is no CPU or
PyTorch fallback: if the HIP library is missing, or no HIP device is visible, every
solve raises."""
import ctypes as C
import os
import subprocess

import numpy as np

from . import layout as L

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
CSRC_DIR = os.path.join(_HERE, "csrc")
# BTRAPZ_HIP_LIB: another build of the library (tools: A/B runs of kernel variants on one GPU box); default: the in-tree build
LIB_PATH = os.environ.get("BTRAPZ_HIP_LIB") or os.path.join(LIB_DIR, "libbtrapz_hip.so")


class BtrapzError(RuntimeError):
    pass


class CShared(C.Structure):
    _fields_ = [("w_s", C.c_double * 4), ("w_l", C.c_double * 4),
                ("weight_end_s", C.c_double), ("weight_end_l", C.c_double),
                ("ds_ref", C.c_double), ("dl_ref", C.c_double),
                ("dds", C.c_double * 2), ("ddds", C.c_double * 2),
                ("ddl", C.c_double * 2), ("dddl", C.c_double * 2),
                ("delta", C.c_double), ("variant", C.c_int), ("reserved", C.c_int)]

    @classmethod
    def from_shared(cls, sh):
        s = cls()
        s.w_s[:] = sh.w_s; s.w_l[:] = sh.w_l
        s.weight_end_s, s.weight_end_l = sh.weight_end_s, sh.weight_end_l
        s.ds_ref, s.dl_ref = sh.ds_ref, sh.dl_ref
        s.dds[:] = sh.dds; s.ddds[:] = sh.ddds; s.ddl[:] = sh.ddl; s.dddl[:] = sh.dddl
        s.delta, s.variant = sh.delta, sh.variant
        return s


class COptions(C.Structure):
    """btrapz_options; struct_size is what btrapz_options_init() sets (the library rejects other layouts)."""
    _fields_ = [("struct_size", C.c_int), ("max_iter", C.c_int), ("eps", C.c_double), ("step_fraction", C.c_double),
                ("step_threshold", C.c_double), ("elastic", C.c_int), ("elastic_tol", C.c_double),
                ("elastic_delta", C.c_double), ("queue", C.c_int), ("split", C.c_int), ("start", C.c_int), ("cap_iter", C.c_int), ("lean", C.c_int), ("compact", C.c_int)]


def _options(max_iter=0, eps=0.0, elastic=0, elastic_tol=0.0, elastic_delta=0.0, queue=0, split=0, start=0, cap_iter=0, lean=0, compact=0):
    return COptions(C.sizeof(COptions), int(max_iter), float(eps), float(os.environ.get("BTRAPZ_STEP_FRACTION", "0")),
                    float(os.environ.get("BTRAPZ_STEP_THRESHOLD", "0")), int(elastic), float(elastic_tol),
                    float(elastic_delta), int(queue), int(split), int(start), int(cap_iter), int(lean), int(compact))


class CGrads(C.Structure):
    """btrapz_grads (include/btrapz_hip.h): device pointers of the gradient arrays of btrapz_solve_vjp_device."""
    _fields_ = [("seg", C.c_void_p), ("init", C.c_void_p), ("ref_end", C.c_void_p), ("dl_bounds", C.c_void_p),
                ("shared", C.c_void_p)]


class CTangents(C.Structure):
    """btrapz_tangents (include/btrapz_hip.h): device pointers of the input tangents of btrapz_solve_jvp_device."""
    _fields_ = [("seg", C.c_void_p), ("init", C.c_void_p), ("ref_end", C.c_void_p), ("dl_bounds", C.c_void_p),
                ("shared", C.c_void_p)]


MAX_TANGENTS = 32   # BTRAPZ_MAX_TANGENTS


class CRowCheck(C.Structure):
    """btrapz_row_check (include/btrapz_hip_check.h): the unit and the output device pointers of btrapz_check_rows_device."""
    _fields_ = [("struct_size", C.c_size_t), ("unit", C.c_int), ("margin", C.c_void_p), ("worst", C.c_void_p),
                ("eq_res", C.c_void_p), ("obj", C.c_void_p)]


class CKnotGrads(C.Structure):
    """btrapz_knot_grads (include/btrapz_hip.h): pointers of the gradient arrays of btrapz_corridor_batch_vjp_device
    (device) / btrapz_corridor_vjp_host (host)."""
    _fields_ = [("s_bounds", C.c_void_p), ("l_bounds", C.c_void_p), ("ds_bounds", C.c_void_p),
                ("dl_bounds_knots", C.c_void_p), ("s_ref", C.c_void_p), ("l_ref", C.c_void_p)]


KNOT_GRADS = ("s_bounds", "l_bounds", "ds_bounds", "dl_bounds_knots", "s_ref", "l_ref")


class CKnotTangents(C.Structure):
    """btrapz_knot_tangents (include/btrapz_hip_stage_jvp.h): pointers of the input tangents of
    btrapz_corridor_batch_jvp_device (device) / btrapz_corridor_jvp_host (host), in KNOT_GRADS' order."""
    _fields_ = CKnotGrads._fields_


class CWarm(C.Structure):
    """btrapz_warm (include/btrapz_hip.h): optional warm start of a solve."""
    _fields_ = [("x0", C.c_void_p), ("lam0", C.c_void_p), ("lam_out", C.c_void_p),
                ("mu0", C.c_double), ("smin", C.c_double), ("hint", C.c_void_p)]


class CTrajInput(C.Structure):
    """btrapz_traj_input: the content of the corridor text file (trp_wrapper.cpp:39-144) as arrays."""
    _fields_ = [("N", C.c_int), ("num_obs", C.c_int), ("delta", C.c_double),
                ("init_s", C.c_double * 3), ("init_l", C.c_double * 3),
                ("ds_ref", C.c_double), ("dl_ref", C.c_double),
                ("dds", C.c_double * 2), ("ddds", C.c_double * 2), ("ddl", C.c_double * 2), ("dddl", C.c_double * 2),
                ("s_bounds", C.c_void_p), ("l_bounds", C.c_void_p), ("ds_bounds", C.c_void_p),
                ("dl_bounds", C.c_void_p), ("s_ref", C.c_void_p), ("l_ref", C.c_void_p)]


class CMultiShard(C.Structure):
    """btrapz_multi_shard: a shard that is on its device already."""
    _fields_ = [("B", C.c_int), ("index_base", C.c_longlong), ("seg", C.c_void_p), ("init", C.c_void_p),
                ("ref_end", C.c_void_p), ("dl_bounds", C.c_void_p)]


class CMultiView(C.Structure):
    """btrapz_multi_view: what lives on one device slot after a step (device pointers)."""
    _fields_ = [("device", C.c_int), ("B", C.c_int), ("index_base", C.c_longlong), ("stream", C.c_void_p), ("ctx", C.c_void_p),
                ("ctrl", C.c_void_p), ("cost", C.c_void_p), ("status", C.c_void_p), ("iters", C.c_void_p),
                ("best_idx", C.c_void_p), ("best_cost", C.c_void_p), ("best_ctrl", C.c_void_p)]


MULTI_AUTO, MULTI_COPIES, MULTI_RCCL = 0, 1, 2


class CParams(C.Structure):
    """include/btrapz/py_cpp_.h:6-21 == trp_wrapper.py:19-32."""
    _fields_ = [("s_acc_weight", C.c_double), ("s_jerk_weight", C.c_double),
                ("l_acc_weight", C.c_double), ("l_jerk_weight", C.c_double),
                ("weight_s_ref", C.c_double), ("weight_ds_ref", C.c_double),
                ("weight_l_ref", C.c_double), ("weight_dl_ref", C.c_double),
                ("weight_end_s", C.c_double), ("weight_end_l", C.c_double),
                ("iteration", C.c_int)]


class CSegment(C.Structure):
    """btrapz_segment == Cube (include/btrapz/cube_type.h:2-24)."""
    _fields_ = [("beg_t", C.c_int), ("end_t", C.c_int), ("t", C.c_double),
                ("beg_l", C.c_double), ("end_l", C.c_double),
                ("upp_skew", C.c_double), ("upp_bias", C.c_double),
                ("down_skew", C.c_double), ("down_bias", C.c_double),
                ("l_upp_skew", C.c_double), ("l_upp_bias", C.c_double),
                ("l_down_skew", C.c_double), ("l_down_bias", C.c_double),
                ("count", C.c_int)]


class CRoad(C.Structure):
    """btrapz_road: road limits and safety margins of the prism -> bounds stage (cart_frenet.py:54-58, 698-699)."""
    _fields_ = [("s_lo", C.c_double), ("s_hi", C.c_double), ("l_lo", C.c_double), ("l_hi", C.c_double),
                ("l_safe", C.c_double), ("w_safe", C.c_double), ("knots_per_second", C.c_double)]

    @classmethod
    def reference(cls):
        return cls(0.0, 50.0, -2.0, 8.0, 5.0 / 3 + 5.0 / 3, 2.0 / 3 + 2.0 / 3, 10.0)


_i, _d, _ll, _vp, _str = C.c_int, C.c_double, C.c_longlong, C.c_void_p, C.c_char_p
_ip, _sh, _opt, _par, _road = C.POINTER(C.c_int), C.POINTER(CShared), C.POINTER(COptions), C.POINTER(CParams), C.POINTER(CRoad)
_batch = [_vp] * 4          # seg, init, ref_end, dl_bounds of a uniform batch
_ragged = [_vp] * 5         # seg, seg_count, init, ref_end, dl_bounds
_result = [_vp] * 4         # ctrl, cost, status, iters
_knots = [_vp] * 6          # s_bounds, l_bounds, ds_bounds, dl_bounds_knots, s_ref, l_ref

# Every function of include/btrapz_hip.h: name -> (restype, argtypes), applied by lib().  tests/test_abi.py holds the
# argument counts and return types to the header's prototypes (a wrong count in ctypes is silent garbage, not an error).
PROTOTYPES = {
    "btrapz_find_traj": (_d, [_i, _str, _str, _par]),
    "btrapz_find_traj_mem": (_d, [_i, C.POINTER(CTrajInput), _par, _i, _vp, _ip, _vp, _ip]),
    "btrapz_find_traj_mem_cap": (_d, [_i, C.POINTER(CTrajInput), _par, _i, _vp, _ip, _vp, _i, _ip]),
    "btrapz_find_traj_last_iterations": (_i, []),
    "btrapz_find_traj_last_status": (_i, [_vp]),
    "btrapz_corridor_from_file": (_i, [_i, _str, C.POINTER(CSegment), _i]),
    "btrapz_options_init": (None, [_opt]),
    "btrapz_create": (_i, [C.POINTER(_vp), _i]),
    "btrapz_destroy": (_i, [_vp]),
    "btrapz_last_error": (_str, [_vp]),
    "btrapz_workspace_bytes": (_ll, [_vp]),
    "btrapz_device_count": (_i, []),
    "btrapz_build_has_experiments": (_i, []),
    "btrapz_solve_batch_device": (_i, [_vp, _sh, _opt, _i, _i] + _batch + _result + [_vp]),
    "btrapz_solve_batch_host": (_i, [_vp, _sh, _opt, _i, _i] + _batch + _result),
    "btrapz_rescue_violations_device": (_i, [_vp, _i, _vp, _vp]),
    "btrapz_last_solve_form": (_i, [_vp]),
    "btrapz_argmin_device": (_i, [_vp, _i, _i, _ll, _vp, _vp, _vp, _vp]),
    "btrapz_argmin_pairs_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp]),
    "btrapz_multi_create": (_i, [C.POINTER(_vp), _ip, _i, _i]),
    "btrapz_multi_destroy": (_i, [_vp]),
    "btrapz_multi_last_error": (_str, [_vp]),
    "btrapz_multi_transport": (_i, [_vp]),
    "btrapz_multi_transport_library": (_str, [_vp]),
    "btrapz_multi_device_count": (_i, [_vp]),
    "btrapz_multi_shard_bounds": (_i, [_i, _i, _i, _i, _ip, _ip]),
    "btrapz_multi_upload": (_i, [_vp, _i, _i, _i] + _batch),
    "btrapz_multi_set_shards": (_i, [_vp, _i, _i, _i, C.POINTER(CMultiShard)]),
    "btrapz_multi_solve_argmin": (_i, [_vp, _sh, _opt]),
    "btrapz_multi_result": (_i, [_vp, _i, _vp, _vp, _vp]),
    "btrapz_multi_wait": (_i, [_vp]),
    "btrapz_multi_shard_view": (_i, [_vp, _i, C.POINTER(CMultiView)]),
    "btrapz_multi_download": (_i, [_vp] + _result),
    "btrapz_sample_device": (_i, [_vp, _i, _i, _d, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "btrapz_sample_ragged_device": (_i, [_vp, _i, _i, _vp, _d, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "btrapz_solve_ragged_device": (_i, [_vp, _sh, _opt, _i, _i] + _ragged + _result + [_vp]),
    "btrapz_corridor_batch_device": (_i, [_vp, _i, _i, _i, _i, _d] + _knots + [_i, _vp, _vp, _vp, _vp, _vp]),
    "btrapz_corridor_batch_vjp_device": (_i, [_vp, _i, _i, _i, _i, _d] + _knots + [_i, _vp, _vp, _vp, C.POINTER(CKnotGrads), _vp]),
    "btrapz_corridor_vjp_host": (_i, [_i, _i, _i, _d] + _knots + [_i, _vp, _vp, _vp, C.POINTER(CKnotGrads), _ip]),
    "btrapz_prism_bounds_device": (_i, [_vp, _i, _i, _i, _road, _vp, _i, _vp, _vp, _vp, _vp]),
    "btrapz_prism_bounds_vjp_device": (_i, [_vp, _i, _i, _i, _road, _vp, _i, _vp, _vp, _vp, _vp]),
    "btrapz_prism_bounds_vjp_host": (_i, [_i, _i, _i, _road, _vp, _i, _vp, _vp, _vp]),
    "btrapz_prism_corridor_batch_device": (_i, [_vp, _i, _i, _i, _i, _road, _vp, _i, _d, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp,
                                                _vp, _vp, _vp]),
    "btrapz_solve_warm_device": (_i, [_vp, _sh, _opt, C.POINTER(CWarm), _i, _i] + _ragged + _result + [_vp]),
    "btrapz_solve_sets_device": (_i, [_vp, _sh, _i, _vp, _opt, C.POINTER(CWarm), _i, _i] + _ragged + _result + [_vp]),
    "btrapz_solve_vjp_device": (_i, [_vp, _sh, _i, _vp, _i, _i] + _ragged + [_vp, _vp, _vp, _vp, _vp, C.POINTER(CGrads), _vp]),
    "btrapz_solve_jvp_device": (_i, [_vp, _sh, _i, _vp, _i, _i] + _ragged + [_vp, _vp, _vp, _i, C.POINTER(CTangents), _vp, _vp,
                                     _vp]),
    "btrapz_traj_cost_device": (_i, [_vp, _sh, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "btrapz_traj_cost_vjp_device": (_i, [_vp, _sh, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i] + [_vp] * 7),
    "btrapz_eval_states_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "btrapz_sample_vjp_device": (_i, [_vp, _i, _i, _vp, _d, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "btrapz_eval_states_vjp_device": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "btrapz_debug_mqm_tables": (_i, [_vp, _sh, _vp, _vp]),
    "btrapz_debug_axis_records": (_i, [_vp, _i, _vp, _vp]),
    "btrapz_debug_resume_keys": (_i, [_vp, _i, _vp]),
    "btrapz_debug_parse_double": (_d, [_str, _ip]),
    "btrapz_debug_format_fixed": (_i, [_d, _str]),
}
EXPORTS = tuple(PROTOTYPES)

# Every function of include/btrapz_hip_stage_jvp.h, the same way (tests/test_abi_stage_jvp.py holds it to that header).
PROTOTYPES_STAGE_JVP = {
    "btrapz_prism_bounds_jvp_device": (_i, [_vp, _i, _i, _i, _road, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "btrapz_prism_bounds_jvp_host": (_i, [_i, _i, _i, _road, _vp, _i, _i, _vp, _vp, _vp]),
    "btrapz_corridor_batch_jvp_device": (_i, [_vp, _i, _i, _i, _i, _d] + _knots + [_i, _i, C.POINTER(CKnotTangents), _vp, _vp, _vp, _vp]),
    "btrapz_corridor_jvp_host": (_i, [_i, _i, _i, _d] + _knots + [_i, _i, C.POINTER(CKnotTangents), _vp, _vp, _vp, _ip]),
}
EXPORTS_STAGE_JVP = tuple(PROTOTYPES_STAGE_JVP)

# Every function of include/btrapz_hip_schedule.h, the same way (tests/test_abi_schedule.py holds it to that header).
PROTOTYPES_SCHEDULE = {
    "btrapz_debug_set_schedule": (_i, [_vp, _i]),
    "btrapz_debug_solve_launches": (_i, [_vp]),
}
EXPORTS_SCHEDULE = tuple(PROTOTYPES_SCHEDULE)

# Every function of include/btrapz_hip_select.h, the same way (tests/test_abi_select.py holds it to that header).
PROTOTYPES_SELECT = {
    "btrapz_topk_device": (_i, [_vp, _i, _i, _i, _ll, _vp, _vp, _vp, _vp]),
    "btrapz_topk_pairs_device": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "btrapz_gather_rows_device": (_i, [_vp, _i, _vp, _ll, _i, _i, _vp, _vp, _vp]),
}
EXPORTS_SELECT = tuple(PROTOTYPES_SELECT)

# Every function of include/btrapz_hip_check.h, the same way (tests/test_abi_check.py holds it to that header).
PROTOTYPES_CHECK = {
    "btrapz_check_rows_device": (_i, [_vp, _sh, _i, _vp, _i, _i] + _ragged + [_vp, C.POINTER(CRowCheck), _vp]),
}
EXPORTS_CHECK = tuple(PROTOTYPES_CHECK)

# Every function of include/btrapz_hip_long.h, the same way (tests/test_long_warm_abi.py holds it to that header).
PROTOTYPES_LONG = {
    "btrapz_solve_long_warm_device": (_i, [_vp, _sh, _opt, C.POINTER(CWarm), _i, _i] + _ragged + _result + [_vp]),
}
EXPORTS_LONG = tuple(PROTOTYPES_LONG)

# Every function of include/btrapz_hip_long_rescue.h, the same way (tests/test_long_rescue_goldens.py holds it to that header).
PROTOTYPES_LONG_RESCUE = {
    "btrapz_solve_long_rescue_device": PROTOTYPES_LONG["btrapz_solve_long_warm_device"],
}
EXPORTS_LONG_RESCUE = tuple(PROTOTYPES_LONG_RESCUE)

# Every function of include/btrapz_hip_long_grad.h, the same way (tests/test_long_grad_abi.py holds it to that header).
PROTOTYPES_LONG_GRAD = {
    "btrapz_solve_long_vjp_device": (_i, [_vp, _sh, _i, _vp, _i, _i] + _ragged + [_vp, _vp, _vp, _vp, _vp, C.POINTER(CGrads), _vp]),
    "btrapz_solve_long_jvp_device": (_i, [_vp, _sh, _i, _vp, _i, _i] + _ragged + [_vp, _vp, _vp, _i, C.POINTER(CTangents), _vp, _vp,
                                          _vp]),
}
EXPORTS_LONG_GRAD = tuple(PROTOTYPES_LONG_GRAD)

# Every function of include/btrapz_hip_long_sets.h, the same way (tests/test_long_sets_abi.py holds it to that header).
PROTOTYPES_LONG_SETS = {
    "btrapz_solve_long_sets_device": PROTOTYPES["btrapz_solve_sets_device"],
}
EXPORTS_LONG_SETS = tuple(PROTOTYPES_LONG_SETS)


class CRefLine(C.Structure):
    """btrapz_refline (include/btrapz_hip_cartesian.h): n_lines tables of M points, device or host pointers."""
    _fields_ = [("n_lines", C.c_int), ("M", C.c_int), ("rs", C.c_void_p), ("rx", C.c_void_p), ("ry", C.c_void_p),
                ("rtheta", C.c_void_p), ("rkappa", C.c_void_p), ("rdkappa", C.c_void_p)]


KIN_AUDIT = ("kappa_abs_max", "alat_abs_max", "a_min", "a_max", "v_max", "frame_min", "n_outside", "worst")


class CKinAudit(C.Structure):
    """btrapz_kin_audit (include/btrapz_hip_cartesian.h): the output pointers of the kinematic audit, in KIN_AUDIT's order."""
    _fields_ = [(k, C.c_void_p) for k in KIN_AUDIT]


FRENET_SAMPLES, FRENET_STATES = 0, 1   # BTRAPZ_FRENET_SAMPLES, BTRAPZ_FRENET_STATES
_ref, _aud = C.POINTER(CRefLine), C.POINTER(CKinAudit)

# Every function of include/btrapz_hip_cartesian.h, the same way (tests/test_abi_cartesian.py holds it to that header).
PROTOTYPES_CARTESIAN = {
    "btrapz_cartesian_device": (_i, [_vp, _ref, _vp, _i, _i, _i, _vp, _vp, _vp, _aud, _vp]),
    "btrapz_cartesian_vjp_device": (_i, [_vp, _ref, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "btrapz_cartesian_jvp_device": (_i, [_vp, _ref, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "btrapz_cartesian_host": (_i, [_ref, _vp, _i, _i, _i, _vp, _vp, _vp, _aud]),
    "btrapz_cartesian_vjp_host": (_i, [_ref, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "btrapz_cartesian_jvp_host": (_i, [_ref, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
}
EXPORTS_CARTESIAN = tuple(PROTOTYPES_CARTESIAN)

# Every function of include/btrapz_hip_frenet.h, the same way (tests/test_abi_frenet.py holds it to that header).
PROTOTYPES_FRENET = {
    "btrapz_frenet_device": (_i, [_vp, _ref, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "btrapz_frenet_vjp_device": (_i, [_vp, _ref, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "btrapz_frenet_jvp_device": (_i, [_vp, _ref, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "btrapz_frenet_host": (_i, [_ref, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "btrapz_frenet_vjp_host": (_i, [_ref, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "btrapz_frenet_jvp_host": (_i, [_ref, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
}
EXPORTS_FRENET = tuple(PROTOTYPES_FRENET)


class CFootprint(C.Structure):
    """btrapz_footprint (include/btrapz_hip_clearance.h): the ego's rectangle."""
    _fields_ = [("half_length", C.c_double), ("half_width", C.c_double), ("centre_offset", C.c_double)]


class CObstacles(C.Structure):
    """btrapz_obstacles (include/btrapz_hip_clearance.h): n_scenes scenes of up to O obstacles at n samples, device or host
    pointers."""
    _fields_ = [("n_scenes", C.c_int), ("O", C.c_int), ("n", C.c_int), ("pose", C.c_void_p), ("half", C.c_void_p),
                ("obs_count", C.c_void_p)]


CLEAR_AUDIT = ("clear_min", "worst", "n_below", "n_invalid")


class CClearAudit(C.Structure):
    """btrapz_clear_audit (include/btrapz_hip_clearance.h): the output pointers of the clearance audit, in CLEAR_AUDIT's order."""
    _fields_ = [(k, C.c_void_p) for k in CLEAR_AUDIT]


CLEAR_FEATURES = 12         # BTRAPZ_CLEAR_FEATURES
_d = C.c_double
_foot, _obs, _caud = C.POINTER(CFootprint), C.POINTER(CObstacles), C.POINTER(CClearAudit)

# Every function of include/btrapz_hip_clearance.h, the same way (tests/test_abi_clearance.py holds it to that header).
PROTOTYPES_CLEARANCE = {
    "btrapz_clearance_device": (_i, [_vp, _foot, _obs, _vp, _i, _i, _vp, _vp, _d, _vp, _vp, _caud, _vp]),
    "btrapz_clearance_vjp_device": (_i, [_vp, _foot, _obs, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "btrapz_clearance_jvp_device": (_i, [_vp, _foot, _obs, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "btrapz_clearance_host": (_i, [_foot, _obs, _vp, _i, _i, _vp, _vp, _d, _vp, _vp, _caud]),
    "btrapz_clearance_vjp_host": (_i, [_foot, _obs, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "btrapz_clearance_jvp_host": (_i, [_foot, _obs, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
}
EXPORTS_CLEARANCE = tuple(PROTOTYPES_CLEARANCE)
MAX_TOPK = 64               # BTRAPZ_MAX_TOPK


def _ptr(t):
    """Device tensor -> its address as a c_void_p; None -> None (a NULL argument or struct field), always.  Keeps nothing
    alive: the caller holds the tensor until the launch has run."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _np_ptr(a):
    """The same for a numpy array (host pointers)."""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _np_f64(a):
    """Array-like -> contiguous float64 numpy array (referenced, not copied, when it is one already); None -> None."""
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _stream(stream):
    """The hipStream_t argument: a stream's handle as an integer, None or 0 = the default stream."""
    return C.c_void_p(stream or 0)


def _sets_array(sets):
    """list of layout.Shared -> btrapz_shared[n_sets] (host array; at least one slot, so that an empty list has an address)."""
    return (CShared * max(len(sets), 1))(*[CShared.from_shared(sh) for sh in sets])


def _warm(x0, lam0, lam_out, mu0, smin, hint):
    return CWarm(_ptr(x0), _ptr(lam0), _ptr(lam_out), float(mu0), float(smin), _ptr(hint))


def build(verbose=False):
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-j4", "-C", CSRC_DIR, "all"], stdout=out)
    return LIB_PATH


def kernel_source_hash():
    """Identifies the kernel build a counter profile belongs to: sha256 over the sources and flags that determine
    the solve kernel's code (profiles/*.json carry it; bench.py refuses profiles of other kernel sources)."""
    import hashlib
    h = hashlib.sha256()
    for f in ("btrapz_kernels.hip", "btrapz_lean.hip", "btrapz_lean_warm.hip", "btrapz_lean_pipe.hip", "btrapz_lean_quiet.hip", "btrapz_lean_body.h", "btrapz_ipm.h", "btrapz_device.h", "Makefile",
              os.path.join("..", "..", "include", "btrapz_hip.h")):
        with open(os.path.join(CSRC_DIR, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


_lib = None
ROCM_HIP_RUNTIME = "/opt/rocm/lib/libamdhip64.so"


def _bind_hip_runtime():
    """libbtrapz_hip.so is linked without a HIP runtime of its own (csrc/Makefile): a process
    must hold exactly one libamdhip64.  If PyTorch-ROCm is already imported its bundled runtime
    is promoted to the global symbol scope and reused; otherwise the system runtime is loaded."""
    import sys
    path = ROCM_HIP_RUNTIME
    if "torch" in sys.modules:
        bundled = os.path.join(os.path.dirname(sys.modules["torch"].__file__), "lib", "libamdhip64.so")
        if os.path.exists(bundled):
            path = bundled
    try:
        C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError as e:
        raise BtrapzError("cannot load the HIP runtime %s: %s (there is no CPU path)" % (path, e))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BtrapzError("HIP library %s is missing: run spectral_amd.native.build() "
                              "(there is no CPU path)" % LIB_PATH)
        _bind_hip_runtime()
        l = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in list(PROTOTYPES.items()) + list(PROTOTYPES_STAGE_JVP.items()) + list(PROTOTYPES_SCHEDULE.items()) + list(PROTOTYPES_SELECT.items()) + list(PROTOTYPES_CHECK.items()) + list(PROTOTYPES_LONG.items()) + list(PROTOTYPES_LONG_RESCUE.items()) + list(PROTOTYPES_LONG_GRAD.items()) + list(PROTOTYPES_LONG_SETS.items()) + list(PROTOTYPES_CARTESIAN.items()) + list(PROTOTYPES_FRENET.items()) + list(PROTOTYPES_CLEARANCE.items()):
            fn = getattr(l, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = l
    return _lib


def multi_shard_bounds(B, G, g, group=0):
    """btrapz_multi_shard_bounds: [lo, hi) of device slot g."""
    lo, hi = C.c_int(0), C.c_int(0)
    rc = lib().btrapz_multi_shard_bounds(int(B), int(G), int(g), int(group), C.byref(lo), C.byref(hi))
    if rc != 0:
        raise BtrapzError("btrapz_multi_shard_bounds(%d, %d, %d, %d) -> %d" % (B, G, g, group, rc))
    return lo.value, hi.value


class MultiContext:
    """btrapz_multi: one host process, one context + stream per entry of `devices` (an ordinal may repeat: logical
    devices), candidates sharded contiguously, one gather of the local winners (include/btrapz_hip.h)."""

    def __init__(self, devices, transport=MULTI_AUTO):
        self._h = C.c_void_p()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        rc = lib().btrapz_multi_create(C.byref(self._h), devs, len(devices), int(transport))
        if rc != 0:
            raise BtrapzError("btrapz_multi_create(%s, transport=%d) failed with %d (no HIP device, or the transport "
                              "cannot be had: see stderr)" % (list(devices), transport, rc))
        self.G = len(devices); self.B = self.S = 0; self.group = 0

    def close(self):
        if self._h:
            lib().btrapz_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise BtrapzError("%s failed (%d): %s" % (what, rc, lib().btrapz_multi_last_error(self._h).decode()))

    def transport(self):
        return int(lib().btrapz_multi_transport(self._h))

    def transport_library(self):
        return lib().btrapz_multi_transport_library(self._h).decode()

    def fallback_reason(self):
        return lib().btrapz_multi_last_error(self._h).decode()

    def upload(self, batch, group=0):
        seg, init, ref_end, dlb = _np_f64(batch.seg), _np_f64(batch.init), _np_f64(batch.ref_end), _np_f64(batch.dl_bounds)
        assert seg.shape == (L.NUM_SEG_FIELDS, batch.B, batch.S)
        self._check(lib().btrapz_multi_upload(self._h, batch.B, batch.S, int(group), _np_ptr(seg), _np_ptr(init),
                                              _np_ptr(ref_end), _np_ptr(dlb)), "btrapz_multi_upload")
        self.B, self.S, self.group = batch.B, batch.S, int(group)

    def set_shards(self, B, S, shards, group=0):
        """shards: list of (B_g, index_base, seg, init, ref_end, dl_bounds) with torch tensors on the slot's device (or
        None for an empty shard); the tensors must stay alive while steps run."""
        arr = (CMultiShard * self.G)()
        for g, (Bg, base, seg, init, ref_end, dlb) in enumerate(shards):
            arr[g] = CMultiShard(int(Bg), int(base), _ptr(seg), _ptr(init), _ptr(ref_end), _ptr(dlb))
        self._check(lib().btrapz_multi_set_shards(self._h, int(B), int(S), int(group), arr), "btrapz_multi_set_shards")
        self.B, self.S, self.group = int(B), int(S), int(group)
        self._keep = shards

    def solve_argmin(self, shared, **options):
        self.prepared_step(shared, **options)()

    def prepared_step(self, shared, **options):
        """solve_argmin with its argument structs built once: returns a function of no arguments (timing loops)."""
        sh = CShared.from_shared(shared)
        opt = _options(**options)
        fn, check, h = lib().btrapz_multi_solve_argmin, self._check, self._h
        args = (h, C.byref(sh), C.byref(opt))

        def call(_keep=(sh, opt)):
            check(fn(*args), "btrapz_multi_solve_argmin")
        return call

    def result(self, device_slot=-1):
        """(best_idx, best_cost, best_ctrl): scalars + [12 S] for one arg-min group, arrays [n], [n], [n, 12 S] for n groups."""
        n = 1 if (self.group == 0 or self.group >= self.B) else self.B // self.group
        idx = np.zeros(n, dtype=np.int64); cost = np.zeros(n); ctrl = np.zeros((n, 12 * self.S))
        self._check(lib().btrapz_multi_result(self._h, int(device_slot), _np_ptr(idx), _np_ptr(cost), _np_ptr(ctrl)), "btrapz_multi_result")
        return (int(idx[0]), float(cost[0]), ctrl[0]) if n == 1 else (idx, cost, ctrl)

    def wait(self):
        self._check(lib().btrapz_multi_wait(self._h), "btrapz_multi_wait")

    def view(self, device_slot):
        v = CMultiView()
        self._check(lib().btrapz_multi_shard_view(self._h, int(device_slot), C.byref(v)), "btrapz_multi_shard_view")
        return v

    def download(self):
        ctrl = np.zeros((self.B, 12 * self.S)); cost = np.zeros(self.B)
        status = np.zeros(self.B, dtype=np.int32); iters = np.zeros(self.B, dtype=np.int32)
        self._check(lib().btrapz_multi_download(self._h, _np_ptr(ctrl), _np_ptr(cost), _np_ptr(status), _np_ptr(iters)), "btrapz_multi_download")
        return dict(ctrl=ctrl, cost=cost, status=status, iters=iters)


class Context:
    """Owns a btrapz_ctx on one HIP device."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib().btrapz_create(C.byref(self._h), int(device))
        if rc != 0:
            raise BtrapzError("btrapz_create(device=%d) failed with %d: no HIP device "
                              "(this library has no CPU path)" % (device, rc))
        self.device = device

    def close(self):
        if self._h:
            lib().btrapz_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise BtrapzError("%s failed (%d): %s" % (what, rc, lib().btrapz_last_error(self._h).decode()))

    # ---- host-pointer path (numpy in, numpy out) ------------------------------------------
    def solve_host(self, batch, shared, max_iter=0, eps=0.0, elastic=0, elastic_tol=0.0, split=0):
        B, S = batch.B, batch.S
        seg, init, ref_end, dlb = _np_f64(batch.seg), _np_f64(batch.init), _np_f64(batch.ref_end), _np_f64(batch.dl_bounds)
        assert seg.shape == (L.NUM_SEG_FIELDS, B, S)
        ctrl = np.empty((B, 12 * S)); cost = np.empty(B)
        status = np.empty(B, dtype=np.int32); iters = np.empty(B, dtype=np.int32)
        sh = CShared.from_shared(shared); opt = _options(max_iter, eps, elastic, elastic_tol, split=split)
        self._check(lib().btrapz_solve_batch_host(self._h, C.byref(sh), C.byref(opt), B, S, _np_ptr(seg), _np_ptr(init),
                                                  _np_ptr(ref_end), _np_ptr(dlb), _np_ptr(ctrl), _np_ptr(cost),
                                                  _np_ptr(status), _np_ptr(iters)), "btrapz_solve_batch_host")
        return ctrl, cost, status, iters

    # ---- device-pointer path (torch tensors only carry the memory) --------------------------
    def solve_device(self, B, S, shared, seg, init, ref_end, dl_bounds, ctrl, cost, status, iters=None,
                     stream=None, max_iter=0, eps=0.0, elastic=0, elastic_tol=0.0, queue=0, split=0, start=0, cap_iter=0, lean=0, compact=0):
        self.prepared_solve(B, S, shared, seg, init, ref_end, dl_bounds, ctrl, cost, status, iters, stream=stream,
                            max_iter=max_iter, eps=eps, elastic=elastic, elastic_tol=elastic_tol, queue=queue, split=split,
                            start=start, cap_iter=cap_iter, lean=lean, compact=compact)()

    def prepared_solve(self, B, S, shared, seg, init, ref_end, dl_bounds, ctrl, cost, status, iters=None, stream=None,
                       **options):
        """btrapz_solve_batch_device with its argument structs built ONCE: returns a function of no arguments that
        makes the call (a replanning loop or a latency measurement pays the C call, not the marshalling).  The tensors
        and `stream` must stay alive and unchanged in place; options as in solve_device."""
        sh = CShared.from_shared(shared); opt = _options(**options)
        fn, check = lib().btrapz_solve_batch_device, self._check
        args = (self._h, C.byref(sh), C.byref(opt), B, S, _ptr(seg), _ptr(init), _ptr(ref_end), _ptr(dl_bounds), _ptr(ctrl),
                _ptr(cost), _ptr(status), _ptr(iters), _stream(stream))
        keep = (sh, opt, seg, init, ref_end, dl_bounds, ctrl, cost, status, iters)

        def call(_keep=keep):
            check(fn(*args), "btrapz_solve_batch_device")
        return call

    def solve_ragged_device(self, B, seg_stride, shared, seg, seg_count, init, ref_end, dl_bounds, ctrl, cost,
                            status, iters=None, stream=None, max_iter=0, eps=0.0, elastic=0, elastic_tol=0.0, cap_iter=0, lean=0, compact=0):
        sh = CShared.from_shared(shared); opt = _options(max_iter, eps, elastic, elastic_tol, cap_iter=cap_iter, lean=lean, compact=compact)
        self._check(lib().btrapz_solve_ragged_device(self._h, C.byref(sh), C.byref(opt), B, seg_stride, _ptr(seg),
                                                     _ptr(seg_count), _ptr(init), _ptr(ref_end), _ptr(dl_bounds),
                                                     _ptr(ctrl), _ptr(cost), _ptr(status), _ptr(iters), _stream(stream)),
                    "btrapz_solve_ragged_device")

    def solve_warm_device(self, B, seg_stride, shared, seg, seg_count, init, ref_end, dl_bounds, ctrl, cost, status,
                          iters=None, x0=None, lam0=None, lam_out=None, mu0=0.0, smin=0.0, stream=None, max_iter=0,
                          eps=0.0, hint=None, elastic=0, elastic_tol=0.0, lean=0):
        """btrapz_solve_warm_device: seg_count None = uniform batch; x0 / lam0 / lam_out optional."""
        self._warm_call("btrapz_solve_warm_device", B, seg_stride, shared, seg, seg_count, init, ref_end, dl_bounds, ctrl, cost,
                        status, iters, _warm(x0, lam0, lam_out, mu0, smin, hint), stream,
                        _options(max_iter, eps, elastic, elastic_tol, lean=lean))

    def solve_long_warm_device(self, B, seg_stride, shared, seg, seg_count, init, ref_end, dl_bounds, ctrl, cost, status,
                               iters=None, x0=None, lam0=None, lam_out=None, mu0=0.0, smin=0.0, stream=None, max_iter=0,
                               eps=0.0, hint=None, elastic=0, elastic_tol=0.0, lean=0):
        """btrapz_solve_long_warm_device (include/btrapz_hip_long.h): solve_warm_device with seg_stride up to 256 -- the
        candidates of 65..256 segments are warm-started and keep their multipliers too.  elastic != 0 is refused."""
        self._warm_call("btrapz_solve_long_warm_device", B, seg_stride, shared, seg, seg_count, init, ref_end, dl_bounds, ctrl,
                        cost, status, iters, _warm(x0, lam0, lam_out, mu0, smin, hint), stream,
                        _options(max_iter, eps, elastic, elastic_tol, lean=lean))

    def solve_long_rescue_device(self, B, seg_stride, shared, seg, seg_count, init, ref_end, dl_bounds, ctrl, cost, status,
                                 iters=None, x0=None, lam0=None, lam_out=None, mu0=0.0, smin=0.0, stream=None, max_iter=0,
                                 eps=0.0, hint=None, elastic=1, elastic_tol=0.0, lean=0):
        """btrapz_solve_long_rescue_device (include/btrapz_hip_long_rescue.h): solve_long_warm_device with the rescue pass
        (elastic 0 or 1) -- uniform batches up to 256 segments and the long candidates of a ragged record too."""
        self._warm_call("btrapz_solve_long_rescue_device", B, seg_stride, shared, seg, seg_count, init, ref_end, dl_bounds, ctrl,
                        cost, status, iters, _warm(x0, lam0, lam_out, mu0, smin, hint), stream,
                        _options(max_iter, eps, elastic, elastic_tol, lean=lean))

    def _warm_call(self, name, B, seg_stride, shared, seg, seg_count, init, ref_end, dl_bounds, ctrl, cost, status, iters, warm,
                   stream, opt):
        """The two entry points that take (shared, options, btrapz_warm, a batch record, the result arrays)."""
        sh = CShared.from_shared(shared)
        self._check(getattr(lib(), name)(self._h, C.byref(sh), C.byref(opt), C.byref(warm), B, seg_stride, _ptr(seg),
                                         _ptr(seg_count), _ptr(init), _ptr(ref_end), _ptr(dl_bounds), _ptr(ctrl), _ptr(cost),
                                         _ptr(status), _ptr(iters), _stream(stream)), name)

    def solve_sets_device(self, B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl, cost, status,
                          iters=None, x0=None, lam0=None, lam_out=None, mu0=0.0, smin=0.0, hint=None, stream=None,
                          max_iter=0, eps=0.0, elastic=0, cap_iter=0, lean=0, compact=0, split=0):
        """btrapz_solve_sets_device: sets = list of layout.Shared (one per parameter set), set_index = [B] int32 device
        tensor (a value outside [0, len(sets)): that candidate is not solved, status NO_CORRIDOR); seg_count None =
        uniform batch.  Warm start as in solve_warm_device (hint is accepted and ignored by the library)."""
        opt = _options(max_iter, eps, elastic, split=split, cap_iter=cap_iter, lean=lean, compact=compact)
        use_warm = any(t is not None for t in (x0, lam0, lam_out, hint))
        warm = C.byref(_warm(x0, lam0, lam_out, mu0, smin, hint)) if use_warm else None
        self._check(lib().btrapz_solve_sets_device(self._h, _sets_array(sets), len(sets), _ptr(set_index), C.byref(opt),
                                                   warm, B, seg_stride, _ptr(seg), _ptr(seg_count), _ptr(init),
                                                   _ptr(ref_end), _ptr(dl_bounds), _ptr(ctrl), _ptr(cost), _ptr(status),
                                                   _ptr(iters), _stream(stream)), "btrapz_solve_sets_device")

    def solve_long_sets_device(self, B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl, cost, status,
                               iters=None, x0=None, lam0=None, lam_out=None, mu0=0.0, smin=0.0, hint=None, stream=None,
                               max_iter=0, eps=0.0, elastic=0, elastic_tol=0.0, cap_iter=0, lean=0, compact=0, split=0):
        """btrapz_solve_long_sets_device (include/btrapz_hip_long_sets.h): solve_sets_device with warm starts and kept
        multipliers up to 256 segments and with the rescue pass (elastic 0 or 1) at every width."""
        opt = _options(max_iter, eps, elastic, elastic_tol, split=split, cap_iter=cap_iter, lean=lean, compact=compact)
        use_warm = any(t is not None for t in (x0, lam0, lam_out, hint))
        warm = C.byref(_warm(x0, lam0, lam_out, mu0, smin, hint)) if use_warm else None
        self._check(lib().btrapz_solve_long_sets_device(self._h, _sets_array(sets), len(sets), _ptr(set_index), C.byref(opt),
                                                        warm, B, seg_stride, _ptr(seg), _ptr(seg_count), _ptr(init),
                                                        _ptr(ref_end), _ptr(dl_bounds), _ptr(ctrl), _ptr(cost), _ptr(status),
                                                        _ptr(iters), _stream(stream)), "btrapz_solve_long_sets_device")

    def solve_vjp_device(self, B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl, lam, status,
                         ctrl_bar, cost_bar, g_seg=None, g_init=None, g_ref_end=None, g_dl_bounds=None, g_shared=None,
                         stream=None):
        """btrapz_solve_vjp_device: gradients of a solve (elastic = 0, multipliers kept) w.r.t. its inputs.  sets = list of
        layout.Shared; set_index None = every candidate with sets[0]; seg_count None = uniform batch; ctrl_bar / cost_bar
        may be None (zero); the g_* device tensors are overwritten (None: not wanted)."""
        self._vjp_call("btrapz_solve_vjp_device", B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl, lam,
                       status, ctrl_bar, cost_bar, CGrads(_ptr(g_seg), _ptr(g_init), _ptr(g_ref_end), _ptr(g_dl_bounds), _ptr(g_shared)),
                       stream)

    def solve_long_vjp_device(self, B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl, lam, status,
                              ctrl_bar, cost_bar, g_seg=None, g_init=None, g_ref_end=None, g_dl_bounds=None, g_shared=None,
                              stream=None):
        """btrapz_solve_long_vjp_device (include/btrapz_hip_long_grad.h): solve_vjp_device with seg_stride up to 256 -- ctrl,
        lam and status are those of solve_long_warm_device."""
        self._vjp_call("btrapz_solve_long_vjp_device", B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl,
                       lam, status, ctrl_bar, cost_bar,
                       CGrads(_ptr(g_seg), _ptr(g_init), _ptr(g_ref_end), _ptr(g_dl_bounds), _ptr(g_shared)), stream)

    def _vjp_call(self, name, B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl, lam, status, ctrl_bar,
                  cost_bar, grads, stream):
        """The two entry points that take (sets, a batch record, a solve's ctrl / lam / status, cotangents, btrapz_grads)."""
        self._check(getattr(lib(), name)(self._h, _sets_array(sets), len(sets), _ptr(set_index), B, seg_stride, _ptr(seg),
                                         _ptr(seg_count), _ptr(init), _ptr(ref_end), _ptr(dl_bounds), _ptr(ctrl), _ptr(lam),
                                         _ptr(status), _ptr(ctrl_bar), _ptr(cost_bar), C.byref(grads), _stream(stream)), name)

    def solve_jvp_device(self, B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl, lam, status,
                         T, seg_dot=None, init_dot=None, ref_end_dot=None, dl_bounds_dot=None, shared_dot=None,
                         ctrl_dot=None, cost_dot=None, stream=None):
        """btrapz_solve_jvp_device: directional derivatives of a solve (elastic = 0, multipliers kept) along T tangents per
        candidate.  sets / set_index / seg_count as in solve_vjp_device; the *_dot device tensors carry a leading axis T
        (None: zero); ctrl_dot [T, B, 12 seg_stride] / cost_dot [T, B] are overwritten (either may be None)."""
        self._jvp_call("btrapz_solve_jvp_device", B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl, lam,
                       status, T, CTangents(_ptr(seg_dot), _ptr(init_dot), _ptr(ref_end_dot), _ptr(dl_bounds_dot), _ptr(shared_dot)),
                       ctrl_dot, cost_dot, stream)

    def solve_long_jvp_device(self, B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl, lam, status,
                              T, seg_dot=None, init_dot=None, ref_end_dot=None, dl_bounds_dot=None, shared_dot=None,
                              ctrl_dot=None, cost_dot=None, stream=None):
        """btrapz_solve_long_jvp_device (include/btrapz_hip_long_grad.h): solve_jvp_device with seg_stride up to 256 -- ctrl,
        lam and status are those of solve_long_warm_device."""
        self._jvp_call("btrapz_solve_long_jvp_device", B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl,
                       lam, status, T,
                       CTangents(_ptr(seg_dot), _ptr(init_dot), _ptr(ref_end_dot), _ptr(dl_bounds_dot), _ptr(shared_dot)),
                       ctrl_dot, cost_dot, stream)

    def _jvp_call(self, name, B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl, lam, status, T, tan,
                  ctrl_dot, cost_dot, stream):
        """The two entry points that take (sets, a batch record, a solve's ctrl / lam / status, T, btrapz_tangents, outputs)."""
        self._check(getattr(lib(), name)(self._h, _sets_array(sets), len(sets), _ptr(set_index), B, seg_stride, _ptr(seg),
                                         _ptr(seg_count), _ptr(init), _ptr(ref_end), _ptr(dl_bounds), _ptr(ctrl), _ptr(lam),
                                         _ptr(status), int(T), C.byref(tan), _ptr(ctrl_dot), _ptr(cost_dot), _stream(stream)),
                    name)

    def check_rows_device(self, B, seg_stride, sets, set_index, seg, seg_count, init, ref_end, dl_bounds, ctrl, unit=0,
                          margin=None, worst=None, eq_res=None, obj=None, stream=None):
        """btrapz_check_rows_device: the audit of ctrl [B, 12 seg_stride] against every row of the record's QPs.  sets /
        set_index / seg_count as in solve_vjp_device; unit 0 = the rows' own units, 1 = divided by the rows' norms; margin
        [B, 2, 4] / worst [B, 2, 4] int32 / eq_res [B, 2, 2] / obj [B] device tensors are overwritten (None: not wanted)."""
        out = CRowCheck(C.sizeof(CRowCheck), int(unit), _ptr(margin), _ptr(worst), _ptr(eq_res), _ptr(obj))
        self._check(lib().btrapz_check_rows_device(self._h, _sets_array(sets), len(sets), _ptr(set_index), int(B),
                                                   int(seg_stride), _ptr(seg), _ptr(seg_count), _ptr(init), _ptr(ref_end),
                                                   _ptr(dl_bounds), _ptr(ctrl), C.byref(out), _stream(stream)),
                    "btrapz_check_rows_device")

    def traj_cost_device(self, B, seg_stride, sets, set_index, seg, seg_count, init, ctrl, status, N, s_ref, l_ref,
                         ref_stride, a_cost, n_points=None, stream=None):
        """btrapz_traj_cost_device: a_cost [B] of the sampled trajectories of ctrl, scored with sets (list of layout.Shared;
        set_index None = every candidate with sets[0]); seg_count / status / n_points may be None; ref_stride N or 0."""
        self._check(lib().btrapz_traj_cost_device(self._h, _sets_array(sets), len(sets), _ptr(set_index), int(B),
                                                  int(seg_stride), _ptr(seg), _ptr(seg_count), _ptr(init), _ptr(ctrl),
                                                  _ptr(status), int(N), _ptr(s_ref), _ptr(l_ref), int(ref_stride),
                                                  _ptr(a_cost), _ptr(n_points), _stream(stream)), "btrapz_traj_cost_device")

    def traj_cost_vjp_device(self, B, seg_stride, sets, set_index, seg, seg_count, init, ctrl, status, N, s_ref, l_ref,
                             ref_stride, a_cost_bar, ctrl_bar=None, init_bar=None, params_bar=None, s_ref_bar=None,
                             l_ref_bar=None, stream=None):
        """btrapz_traj_cost_vjp_device: the gradient device tensors (any may be None) are overwritten."""
        self._check(lib().btrapz_traj_cost_vjp_device(self._h, _sets_array(sets), len(sets), _ptr(set_index), int(B),
                                                      int(seg_stride), _ptr(seg), _ptr(seg_count), _ptr(init), _ptr(ctrl),
                                                      _ptr(status), int(N), _ptr(s_ref), _ptr(l_ref), int(ref_stride),
                                                      _ptr(a_cost_bar), _ptr(ctrl_bar), _ptr(init_bar), _ptr(params_bar),
                                                      _ptr(s_ref_bar), _ptr(l_ref_bar), _stream(stream)),
                    "btrapz_traj_cost_vjp_device")

    def workspace_bytes(self):
        """btrapz_workspace_bytes: device memory the context holds for its launches right now."""
        return int(lib().btrapz_workspace_bytes(self._h))

    def last_solve_form(self):
        """btrapz_last_solve_form: 0 packed, 1 split, 2 long, 3 capped + resume, 4 queue; + 8: the two-wavefronts-per-SIMD form."""
        return int(lib().btrapz_last_solve_form(self._h))

    def rescue_violations_device(self, B, viol, stream=None):
        """btrapz_rescue_violations_device: viol [B][4] (position, velocity, acceleration, jerk rows) of the last solve
        with elastic != 0."""
        self._check(lib().btrapz_rescue_violations_device(self._h, int(B), _ptr(viol), _stream(stream)),
                    "btrapz_rescue_violations_device")

    def debug_axis_records(self, B):
        """(iters [B, 2], status [B, 2]) of the axis problems of the last batched solve."""
        it = np.zeros((B, 2), dtype=np.int32); st = np.zeros((B, 2), dtype=np.int32)
        self._check(lib().btrapz_debug_axis_records(self._h, B, _np_ptr(it), _np_ptr(st)), "btrapz_debug_axis_records")
        return it, st

    def debug_resume_keys(self, B):
        """keys [2, B] of the last capped solve's resume launch (0: not handed over)."""
        k = np.zeros((2, B), dtype=np.int32)
        self._check(lib().btrapz_debug_resume_keys(self._h, B, _np_ptr(k)), "btrapz_debug_resume_keys")
        return k

    def debug_set_schedule(self, mode):
        """btrapz_debug_set_schedule: 0 automatic, -1 never three launches, 1 / 2 three launches with the s / l axis first,
        3 / 4 the s / l axis first and the other axis quiet (uncapped, behind the first axis's resume wavefronts)."""
        self._check(lib().btrapz_debug_set_schedule(self._h, int(mode)), "btrapz_debug_set_schedule")

    def debug_solve_launches(self):
        """Solve-kernel launches of the main step of the last batched solve: 1, 2 or 3."""
        return int(lib().btrapz_debug_solve_launches(self._h))

    def debug_mqm_tables(self, shared):
        sh = CShared.from_shared(shared)
        h = np.zeros(168); d = np.zeros(168)
        self._check(lib().btrapz_debug_mqm_tables(self._h, C.byref(sh), _np_ptr(h), _np_ptr(d)), "btrapz_debug_mqm_tables")
        return h, d

    def eval_states_device(self, B, seg_stride, seg_count, seg, ctrl, n_times, times, x, stream=None):
        self._check(lib().btrapz_eval_states_device(self._h, B, seg_stride, _ptr(seg_count), _ptr(seg), _ptr(ctrl),
                                                    int(n_times), _ptr(times), _ptr(x), _stream(stream)),
                    "btrapz_eval_states_device")

    def eval_states_vjp_device(self, B, seg_stride, seg_count, seg, ctrl, n_times, times, x_bar, ctrl_bar=None,
                               times_bar=None, stream=None):
        """btrapz_eval_states_vjp_device: ctrl_bar [B, 12 seg_stride] and times_bar [B, n_times] (either may be None) are
        overwritten; ctrl may be None when times_bar is."""
        self._check(lib().btrapz_eval_states_vjp_device(self._h, int(B), int(seg_stride), _ptr(seg_count), _ptr(seg),
                                                        _ptr(ctrl), int(n_times), _ptr(times), _ptr(x_bar), _ptr(ctrl_bar),
                                                        _ptr(times_bar), _stream(stream)), "btrapz_eval_states_vjp_device")

    def sample_vjp_device(self, B, seg_stride, seg_count, delta, seg, sel, max_points, out_bar, ctrl_bar=None, init_bar=None,
                          stream=None, nsel=None):
        """btrapz_sample_vjp_device: ctrl_bar [nsel, 12 seg_stride] and init_bar [nsel, 6], one row per SELECTION (either
        may be None), are overwritten.  nsel: the length of sel unless given."""
        nsel = nsel if nsel is not None else sel.numel() if sel is not None else 0
        self._check(lib().btrapz_sample_vjp_device(self._h, int(B), int(seg_stride), _ptr(seg_count), float(delta), _ptr(seg),
                                                   int(nsel), _ptr(sel), int(max_points), _ptr(out_bar), _ptr(ctrl_bar),
                                                   _ptr(init_bar), _stream(stream)), "btrapz_sample_vjp_device")

    def corridor_batch_device(self, variant, B, N, num_obs, delta, s_bounds, l_bounds, ds_bounds, dl_bounds_knots,
                              s_ref, l_ref, seg_stride, seg, seg_count, ref_end, dl_bounds, stream=None):
        self._check(lib().btrapz_corridor_batch_device(self._h, int(variant), B, N, num_obs, float(delta),
                                                       _ptr(s_bounds), _ptr(l_bounds), _ptr(ds_bounds),
                                                       _ptr(dl_bounds_knots), _ptr(s_ref), _ptr(l_ref), seg_stride,
                                                       _ptr(seg), _ptr(seg_count), _ptr(ref_end), _ptr(dl_bounds),
                                                       _stream(stream)), "btrapz_corridor_batch_device")

    def corridor_batch_vjp_device(self, variant, B, N, num_obs, delta, s_bounds, l_bounds, ds_bounds, dl_bounds_knots,
                                  s_ref, l_ref, seg_stride, seg_bar, ref_end_bar, dl_bounds_bar, grads, stream=None):
        """btrapz_corridor_batch_vjp_device: grads = dict name -> device tensor (KNOT_GRADS; missing or None: not wanted),
        overwritten; the cotangents may be None."""
        g = C.byref(CKnotGrads(*[_ptr(grads.get(k)) for k in KNOT_GRADS])) if grads is not None else None
        self._check(lib().btrapz_corridor_batch_vjp_device(self._h, int(variant), int(B), int(N), int(num_obs), float(delta),
                                                           _ptr(s_bounds), _ptr(l_bounds), _ptr(ds_bounds),
                                                           _ptr(dl_bounds_knots), _ptr(s_ref), _ptr(l_ref), int(seg_stride),
                                                           _ptr(seg_bar), _ptr(ref_end_bar), _ptr(dl_bounds_bar), g,
                                                           _stream(stream)), "btrapz_corridor_batch_vjp_device")

    def prism_bounds_device(self, B, P, N, road, prisms, O, s_bounds, l_bounds, n_strips, stream=None):
        self._check(lib().btrapz_prism_bounds_device(self._h, B, P, N, C.byref(road), _ptr(prisms), O, _ptr(s_bounds),
                                                     _ptr(l_bounds), _ptr(n_strips), _stream(stream)),
                    "btrapz_prism_bounds_device")

    def prism_bounds_vjp_device(self, B, P, N, road, prisms, O, s_bounds_bar, l_bounds_bar, prisms_bar, stream=None):
        """btrapz_prism_bounds_vjp_device: prisms_bar [B, P, 8] is overwritten; either cotangent may be None (zero)."""
        self._check(lib().btrapz_prism_bounds_vjp_device(self._h, int(B), int(P), int(N), C.byref(road) if road is not None else None,
                                                         _ptr(prisms), int(O), _ptr(s_bounds_bar), _ptr(l_bounds_bar),
                                                         _ptr(prisms_bar), _stream(stream)), "btrapz_prism_bounds_vjp_device")

    def prism_bounds_jvp_device(self, B, P, N, road, prisms, O, T, prisms_dot, s_bounds_dot, l_bounds_dot, stream=None):
        """btrapz_prism_bounds_jvp_device: prisms_dot [T, B, P, 8]; s_bounds_dot / l_bounds_dot [T, B, O, N, 2] are
        overwritten (either may be None: not wanted)."""
        self._check(lib().btrapz_prism_bounds_jvp_device(self._h, int(B), int(P), int(N), C.byref(road) if road is not None else None,
                                                         _ptr(prisms), int(O), int(T), _ptr(prisms_dot), _ptr(s_bounds_dot),
                                                         _ptr(l_bounds_dot), _stream(stream)), "btrapz_prism_bounds_jvp_device")

    def corridor_batch_jvp_device(self, variant, B, N, num_obs, delta, s_bounds, l_bounds, ds_bounds, dl_bounds_knots,
                                  s_ref, l_ref, seg_stride, T, tangents, seg_dot, ref_end_dot, dl_bounds_dot, stream=None):
        """btrapz_corridor_batch_jvp_device: tangents = dict name -> device tensor with a leading axis T (KNOT_GRADS;
        missing or None: zero); seg_dot [T, NUM_SEG_FIELDS, B, seg_stride], ref_end_dot [T, B, 2], dl_bounds_dot [T, B, 10]
        are overwritten (any may be None: not wanted)."""
        t = C.byref(CKnotTangents(*[_ptr(tangents.get(k)) for k in KNOT_GRADS])) if tangents is not None else None
        self._check(lib().btrapz_corridor_batch_jvp_device(self._h, int(variant), int(B), int(N), int(num_obs), float(delta),
                                                           _ptr(s_bounds), _ptr(l_bounds), _ptr(ds_bounds),
                                                           _ptr(dl_bounds_knots), _ptr(s_ref), _ptr(l_ref), int(seg_stride),
                                                           int(T), t, _ptr(seg_dot), _ptr(ref_end_dot), _ptr(dl_bounds_dot),
                                                           _stream(stream)), "btrapz_corridor_batch_jvp_device")

    def prism_corridor_batch_device(self, variant, B, P, N, road, prisms, O, delta, ds_bounds, dl_bounds_knots, s_ref, l_ref,
                                    seg_stride, seg, seg_count, ref_end, dl_bounds, n_strips=None, stream=None):
        self._check(lib().btrapz_prism_corridor_batch_device(self._h, int(variant), B, P, N, C.byref(road), _ptr(prisms), O,
                                                             float(delta), _ptr(ds_bounds), _ptr(dl_bounds_knots), _ptr(s_ref),
                                                             _ptr(l_ref), seg_stride, _ptr(seg), _ptr(seg_count), _ptr(ref_end),
                                                             _ptr(dl_bounds), _ptr(n_strips), _stream(stream)),
                    "btrapz_prism_corridor_batch_device")

    def sample_ragged_device(self, B, seg_stride, seg_count, delta, seg, init, ctrl, sel, max_points, out, npoints,
                             stream=None):
        self._check(lib().btrapz_sample_ragged_device(self._h, B, seg_stride, _ptr(seg_count), float(delta), _ptr(seg),
                                                      _ptr(init), _ptr(ctrl), int(sel.numel()), _ptr(sel),
                                                      int(max_points), _ptr(out), _ptr(npoints), _stream(stream)),
                    "btrapz_sample_ragged_device")

    def argmin_device(self, B, group, index_base, cost, best_idx, best_cost, stream=None):
        self._check(lib().btrapz_argmin_device(self._h, B, group, int(index_base), _ptr(cost), _ptr(best_idx),
                                               _ptr(best_cost), _stream(stream)), "btrapz_argmin_device")

    def argmin_pairs_device(self, world, n, pairs, best_cost, best_idx, stream=None):
        self._check(lib().btrapz_argmin_pairs_device(self._h, int(world), int(n), _ptr(pairs), _ptr(best_cost), _ptr(best_idx),
                                                     _stream(stream)), "btrapz_argmin_pairs_device")

    def topk_device(self, B, group, K, index_base, cost, best_idx, best_cost, stream=None):
        """btrapz_topk_device: best_idx / best_cost [B // group, K], the K best of every group in the arg-min's order."""
        self._check(lib().btrapz_topk_device(self._h, int(B), int(group), int(K), int(index_base), _ptr(cost), _ptr(best_idx),
                                             _ptr(best_cost), _stream(stream)), "btrapz_topk_device")

    def topk_pairs_device(self, world, n, K, pairs, best_cost, best_idx, stream=None):
        """btrapz_topk_pairs_device: pairs [world, n, K, 2] int64 (cost bits, global index or -1) -> [n, K]."""
        self._check(lib().btrapz_topk_pairs_device(self._h, int(world), int(n), int(K), _ptr(pairs), _ptr(best_cost),
                                                   _ptr(best_idx), _stream(stream)), "btrapz_topk_pairs_device")

    def gather_rows_device(self, n, idx, index_base, B, row_doubles, src, rows, stream=None):
        """btrapz_gather_rows_device: rows[j] = src[idx[j] - index_base], NaN rows for -1 and for indices outside the shard."""
        self._check(lib().btrapz_gather_rows_device(self._h, int(n), _ptr(idx), int(index_base), int(B), int(row_doubles),
                                                    _ptr(src), _ptr(rows), _stream(stream)), "btrapz_gather_rows_device")

    def cartesian_device(self, refline, line_index, R, n, layout, f, count, cart=None, audit=None, stream=None):
        """btrapz_cartesian_device: refline = CRefLine of device pointers; f under `layout` (FRENET_SAMPLES [R, 6, n] /
        FRENET_STATES [R, 2, n, 3]); line_index / count int32 [R] or None; cart [R, 6, n] and / or audit = dict name ->
        device tensor (KIN_AUDIT; missing or None: not wanted) are overwritten."""
        au = C.byref(CKinAudit(*[_ptr(audit.get(k)) for k in KIN_AUDIT])) if audit is not None else None
        self._check(lib().btrapz_cartesian_device(self._h, C.byref(refline), _ptr(line_index), int(R), int(n), int(layout),
                                                  _ptr(f), _ptr(count), _ptr(cart), au, _stream(stream)),
                    "btrapz_cartesian_device")

    def cartesian_vjp_device(self, refline, line_index, R, n, layout, f, count, cart_bar, f_bar, stream=None):
        """btrapz_cartesian_vjp_device: f_bar (the layout of f) is overwritten."""
        self._check(lib().btrapz_cartesian_vjp_device(self._h, C.byref(refline), _ptr(line_index), int(R), int(n), int(layout),
                                                      _ptr(f), _ptr(count), _ptr(cart_bar), _ptr(f_bar), _stream(stream)),
                    "btrapz_cartesian_vjp_device")

    def cartesian_jvp_device(self, refline, line_index, R, n, layout, f, count, T, f_dot, cart_dot, stream=None):
        """btrapz_cartesian_jvp_device: f_dot [T] x the layout of f; cart_dot [T, R, 6, n] is written at the samples read."""
        self._check(lib().btrapz_cartesian_jvp_device(self._h, C.byref(refline), _ptr(line_index), int(R), int(n), int(layout),
                                                      _ptr(f), _ptr(count), int(T), _ptr(f_dot), _ptr(cart_dot),
                                                      _stream(stream)), "btrapz_cartesian_jvp_device")

    def frenet_device(self, refline, line_index, R, n, layout, order, cart, count, s_window, frenet, interval=None,
                      n_outside=None, stream=None):
        """btrapz_frenet_device: cart [R, 6, n] -> frenet under `layout`; s_window [R, 2] or None; interval int32 [R, n] and
        n_outside int32 [R] or None (not wanted)."""
        self._check(lib().btrapz_frenet_device(self._h, C.byref(refline), _ptr(line_index), int(R), int(n), int(layout), int(order),
                                               _ptr(cart), _ptr(count), _ptr(s_window), _ptr(frenet), _ptr(interval),
                                               _ptr(n_outside), _stream(stream)), "btrapz_frenet_device")

    def frenet_vjp_device(self, refline, line_index, R, n, layout, order, cart, frenet, interval, count, frenet_bar, cart_bar,
                          stream=None):
        """btrapz_frenet_vjp_device: cart_bar [R, 6, n] is overwritten."""
        self._check(lib().btrapz_frenet_vjp_device(self._h, C.byref(refline), _ptr(line_index), int(R), int(n), int(layout),
                                                   int(order), _ptr(cart), _ptr(frenet), _ptr(interval), _ptr(count),
                                                   _ptr(frenet_bar), _ptr(cart_bar), _stream(stream)), "btrapz_frenet_vjp_device")

    def frenet_jvp_device(self, refline, line_index, R, n, layout, order, cart, frenet, interval, count, T, cart_dot, frenet_dot,
                          stream=None):
        """btrapz_frenet_jvp_device: cart_dot [T, R, 6, n]; frenet_dot [T] x the layout of frenet is written at the samples read."""
        self._check(lib().btrapz_frenet_jvp_device(self._h, C.byref(refline), _ptr(line_index), int(R), int(n), int(layout),
                                                   int(order), _ptr(cart), _ptr(frenet), _ptr(interval), _ptr(count), int(T),
                                                   _ptr(cart_dot), _ptr(frenet_dot), _stream(stream)), "btrapz_frenet_jvp_device")

    def clearance_device(self, footprint, obstacles, scene_index, R, n, cart, count, d_safe, clear=None, which=None, audit=None,
                         stream=None):
        """btrapz_clearance_device: footprint = CFootprint, obstacles = CObstacles of device pointers; cart [R, 6, n];
        scene_index / count int32 [R] or None; clear [R, n], which int32 [R, n] and / or audit = dict name -> device tensor
        (CLEAR_AUDIT; missing or None: not wanted) are overwritten at the samples read."""
        au = C.byref(CClearAudit(*[_ptr(audit.get(k)) for k in CLEAR_AUDIT])) if audit is not None else None
        self._check(lib().btrapz_clearance_device(self._h, C.byref(footprint), C.byref(obstacles), _ptr(scene_index), int(R), int(n),
                                                  _ptr(cart), _ptr(count), float(d_safe), _ptr(clear), _ptr(which), au,
                                                  _stream(stream)), "btrapz_clearance_device")

    def clearance_vjp_device(self, footprint, obstacles, scene_index, R, n, cart, count, which, clear_bar, cart_bar, stream=None):
        """btrapz_clearance_vjp_device: cart_bar [R, 6, n] is overwritten as a whole."""
        self._check(lib().btrapz_clearance_vjp_device(self._h, C.byref(footprint), C.byref(obstacles), _ptr(scene_index), int(R),
                                                      int(n), _ptr(cart), _ptr(count), _ptr(which), _ptr(clear_bar),
                                                      _ptr(cart_bar), _stream(stream)), "btrapz_clearance_vjp_device")

    def clearance_jvp_device(self, footprint, obstacles, scene_index, R, n, cart, count, which, T, cart_dot, obs_dot, clear_dot,
                             stream=None):
        """btrapz_clearance_jvp_device: cart_dot [T, R, 6, n], obs_dot [T, n_scenes, O, 3, n] or None; clear_dot [T, R, n] is
        written at the samples read."""
        self._check(lib().btrapz_clearance_jvp_device(self._h, C.byref(footprint), C.byref(obstacles), _ptr(scene_index), int(R),
                                                      int(n), _ptr(cart), _ptr(count), _ptr(which), int(T), _ptr(cart_dot),
                                                      _ptr(obs_dot), _ptr(clear_dot), _stream(stream)),
                    "btrapz_clearance_jvp_device")

    def sample_device(self, B, S, delta, seg, init, ctrl, sel, max_points, out, npoints, stream=None):
        self._check(lib().btrapz_sample_device(self._h, B, S, float(delta), _ptr(seg), _ptr(init), _ptr(ctrl),
                                               int(sel.numel()), _ptr(sel), int(max_points), _ptr(out), _ptr(npoints),
                                               _stream(stream)), "btrapz_sample_device")


def find_traj_native(variant, params, input_path=None, output_path=None):
    """btrapz_find_traj(): the reference's find_traj with explicit paths."""
    cp = params if isinstance(params, CParams) else CParams(*params)
    enc = lambda s: os.fsencode(s) if s else None
    return lib().btrapz_find_traj(int(variant), enc(input_path), enc(output_path), C.byref(cp))


def find_traj_last_status():
    """(status, viol[4]) of the calling thread's last find_traj / find_traj_mem call (btrapz_find_traj_last_status)."""
    v = (C.c_double * 4)()
    st = lib().btrapz_find_traj_last_status(C.cast(v, C.c_void_p))
    return int(st), np.array(v[:])


class TrajCall:
    """btrapz_find_traj_mem() on candidate b of a spectral_amd.knots.KnotBatch, prepared once and callable many times
    (a replanning loop, a latency measurement): the input struct and the output buffers are built here, a call is the
    C function and two slices.  The arrays of `kb` are referenced, not copied, when they are contiguous float64."""

    def __init__(self, variant, params, kb, b=0, cap=None):
        self.variant = int(variant)
        self.cp = params if isinstance(params, CParams) else CParams(*params)
        self._arrs = [_np_f64(a[b]) for a in (kb.s_bounds, kb.l_bounds, kb.ds_bounds, kb.dl_bounds, kb.s_ref, kb.l_ref)]
        h = kb.header
        self.ti = CTrajInput(int(kb.N), int(kb.num_obs), float(kb.delta), (C.c_double * 3)(*kb.init[b, :3]),
                             (C.c_double * 3)(*kb.init[b, 3:]), float(h["ds_ref"]), float(h["dl_ref"]),
                             (C.c_double * 2)(*h["dds"]), (C.c_double * 2)(*h["ddds"]), (C.c_double * 2)(*h["ddl"]),
                             (C.c_double * 2)(*h["dddl"]), *[a.ctypes.data for a in self._arrs])
        self.cap = int(cap if cap is not None else 4 * kb.N + 16)
        self.traj = np.zeros((7, self.cap)); self.ctrl = np.zeros(12 * 256)
        self.n, self.S = C.c_int(0), C.c_int(0)
        self._fn = lib().btrapz_find_traj_mem_cap      # (control points of up to 256 segments: the buffer's size goes along)
        self._args = (self.variant, C.byref(self.ti), C.byref(self.cp), self.cap, self.traj.ctypes.data, C.byref(self.n),
                      self.ctrl.ctypes.data, self.ctrl.size, C.byref(self.S))

    def __call__(self, copy=True):
        """(cost, traj [7][n] rows t s l ds dl dds ddl, ctrl [12 S]); cost == 1e11 on failure (traj, ctrl None).
        copy=False returns views of the call's own buffers (overwritten by the next call)."""
        cost = self._fn(*self._args)
        if cost == 100000000000.0:
            return cost, None, None
        traj, ctrl = self.traj[:, :min(self.n.value, self.cap)], self.ctrl[:12 * self.S.value]
        return (cost, traj.copy(), ctrl.copy()) if copy else (cost, traj, ctrl)


def find_traj_mem(variant, params, kb, b=0, cap=None):
    """btrapz_find_traj_mem(): find_traj on candidate b of a spectral_amd.knots.KnotBatch (arrays in, arrays out).
    Returns (cost, traj [7][n] rows t s l ds dl dds ddl, ctrl [12 S]); cost == 1e11 on failure (traj, ctrl None)."""
    return TrajCall(variant, params, kb, b, cap)()


def prism_bounds_vjp_host(prisms, N, O, s_bounds_bar=None, l_bounds_bar=None, road=None):
    """btrapz_prism_bounds_vjp_host(): the backward pass of the prism stage on the host (no GPU).  prisms [B, P, 8];
    s_bounds_bar, l_bounds_bar [B, O, N, 2] (either may be None: zero).  Returns prisms_bar [B, P, 8]."""
    prisms = _np_f64(prisms)
    if prisms.ndim != 3 or prisms.shape[2] != 8:
        raise ValueError("prisms must be [B, P, 8]")
    B, P = prisms.shape[0], prisms.shape[1]
    bars = [_np_f64(s_bounds_bar), _np_f64(l_bounds_bar)]
    for a in bars:
        if a is not None and a.shape != (B, int(O), int(N), 2):
            raise ValueError("a cotangent must be [B, O, N, 2]")
    out = np.full((B, P, 8), np.nan)
    road = CRoad.reference() if road is None else road
    rc = lib().btrapz_prism_bounds_vjp_host(B, P, int(N), C.byref(road), _np_ptr(prisms), int(O), _np_ptr(bars[0]),
                                            _np_ptr(bars[1]), _np_ptr(out))
    if rc != 0:
        raise BtrapzError("btrapz_prism_bounds_vjp_host -> %d (invalid argument)" % rc)
    return out


def corridor_vjp_host(variant, delta, s_bounds, l_bounds, ds_bounds, dl_bounds_knots, s_ref, l_ref, seg_stride, seg_bar=None,
                      ref_end_bar=None, dl_bounds_bar=None, want=KNOT_GRADS):
    """btrapz_corridor_vjp_host(): the backward pass of the corridor stage for ONE candidate on the host (no GPU).
    s_bounds, l_bounds [num_obs, N, 2]; ds_bounds, dl_bounds_knots [N, 2]; s_ref, l_ref [N]; seg_bar
    [NUM_SEG_FIELDS, seg_stride], ref_end_bar [2], dl_bounds_bar [10] (any may be None).  Returns (dict of the wanted
    gradient arrays, the forward's seg_count)."""
    ins = [_np_f64(a) for a in (s_bounds, l_bounds, ds_bounds, dl_bounds_knots, s_ref, l_ref)]
    sb = ins[0]
    num_obs, N = (sb.shape[0], sb.shape[1]) if sb is not None else (0, 0)
    bars = [_np_f64(seg_bar), _np_f64(ref_end_bar), _np_f64(dl_bounds_bar)]
    if bars[0] is not None:
        assert bars[0].shape == (L.NUM_SEG_FIELDS, seg_stride)
    shapes = dict(s_bounds=(num_obs, N, 2), l_bounds=(num_obs, N, 2), ds_bounds=(N, 2), dl_bounds_knots=(N, 2), s_ref=(N,), l_ref=(N,))
    out = {k: np.full(shapes[k], np.nan) for k in want}
    g = CKnotGrads(*[_np_ptr(out.get(k)) for k in KNOT_GRADS])
    count = C.c_int(-2)
    rc = lib().btrapz_corridor_vjp_host(int(variant), int(N), int(num_obs), float(delta), *[_np_ptr(a) for a in ins],
                                        int(seg_stride), *[_np_ptr(a) for a in bars], C.byref(g), C.byref(count))
    if rc != 0:
        raise BtrapzError("btrapz_corridor_vjp_host -> %d (invalid argument)" % rc)
    return out, count.value


def prism_bounds_jvp_host(prisms, N, O, prisms_dot, road=None, want=("s_bounds", "l_bounds")):
    """btrapz_prism_bounds_jvp_host(): the forward-mode derivative of the prism stage on the host (no GPU).  prisms
    [B, P, 8]; prisms_dot [T, B, P, 8] (entries 6, 7 and inactive slots are not read).  Returns (s_bounds_dot, l_bounds_dot),
    each [T, B, O, N, 2] (None when not named in `want`)."""
    prisms, prisms_dot = _np_f64(prisms), _np_f64(prisms_dot)
    if prisms.ndim != 3 or prisms.shape[2] != 8:
        raise ValueError("prisms must be [B, P, 8]")
    B, P = prisms.shape[0], prisms.shape[1]
    if prisms_dot is not None and (prisms_dot.ndim != 4 or prisms_dot.shape[1:] != (B, P, 8)):
        raise ValueError("prisms_dot must be [T, B, P, 8]")
    T = prisms_dot.shape[0] if prisms_dot is not None else 0
    outs = [np.full((T, B, int(O), int(N), 2), np.nan) if k in want else None for k in ("s_bounds", "l_bounds")]
    road = CRoad.reference() if road is None else road
    rc = lib().btrapz_prism_bounds_jvp_host(B, P, int(N), C.byref(road), _np_ptr(prisms), int(O), int(T), _np_ptr(prisms_dot),
                                            _np_ptr(outs[0]), _np_ptr(outs[1]))
    if rc != 0:
        raise BtrapzError("btrapz_prism_bounds_jvp_host -> %d (invalid argument)" % rc)
    return outs[0], outs[1]


def corridor_jvp_host(variant, delta, s_bounds, l_bounds, ds_bounds, dl_bounds_knots, s_ref, l_ref, seg_stride, tangents,
                      want=("seg", "ref_end", "dl_bounds")):
    """btrapz_corridor_jvp_host(): the forward-mode derivative of the corridor stage for ONE candidate on the host (no
    GPU).  Inputs as corridor_vjp_host; tangents: dict name -> array shaped like the input with a leading axis T (KNOT_GRADS;
    missing or None: zero).  Returns (dict with "seg" [T, NUM_SEG_FIELDS, seg_stride], "ref_end" [T, 2], "dl_bounds" [T, 10]
    as named in `want`, the forward's seg_count)."""
    ins = [_np_f64(a) for a in (s_bounds, l_bounds, ds_bounds, dl_bounds_knots, s_ref, l_ref)]
    sb = ins[0]
    num_obs, N = (sb.shape[0], sb.shape[1]) if sb is not None else (0, 0)
    unknown = set(tangents) - set(KNOT_GRADS)
    if unknown:
        raise ValueError("unknown tangents: %s" % sorted(unknown))
    tan = {k: _np_f64(v) for k, v in tangents.items() if v is not None}
    T = next(iter(tan.values())).shape[0] if tan else 0
    shapes = dict(s_bounds=(num_obs, N, 2), l_bounds=(num_obs, N, 2), ds_bounds=(N, 2), dl_bounds_knots=(N, 2), s_ref=(N,), l_ref=(N,))
    for k, v in tan.items():
        if v.shape != (T,) + shapes[k]:
            raise ValueError("tangent %r: shape %s, expected %s" % (k, v.shape, (T,) + shapes[k]))
    out_shapes = dict(seg=(T, L.NUM_SEG_FIELDS, int(seg_stride)), ref_end=(T, 2), dl_bounds=(T, 10))
    out = {k: np.full(out_shapes[k], np.nan) for k in want}
    t = CKnotTangents(*[_np_ptr(tan.get(k)) for k in KNOT_GRADS])
    count = C.c_int(-2)
    rc = lib().btrapz_corridor_jvp_host(int(variant), int(N), int(num_obs), float(delta), *[_np_ptr(a) for a in ins],
                                        int(seg_stride), int(T), C.byref(t), _np_ptr(out.get("seg")), _np_ptr(out.get("ref_end")),
                                        _np_ptr(out.get("dl_bounds")), C.byref(count))
    if rc != 0:
        raise BtrapzError("btrapz_corridor_jvp_host -> %d (invalid argument)" % rc)
    return out, count.value


def corridor_from_file(variant, input_path, cap=256):
    """Host-side corridor stage (no GPU): list of CSegment, [] when nothing is selected."""
    buf = (CSegment * cap)()
    n = lib().btrapz_corridor_from_file(int(variant), os.fsencode(input_path), buf, cap)
    if n < 0:
        raise BtrapzError("btrapz_corridor_from_file(%s) -> %d" % (input_path, n))
    return [buf[i] for i in range(min(n, cap))]


def _refline_host(refline):
    """layout.RefLine -> (CRefLine of host pointers, the arrays it points into)."""
    arrs = [refline.host[k] for k in L.REFLINE_FIELDS]
    return CRefLine(refline.n_lines, refline.M, *[a.ctypes.data for a in arrs]), arrs


def _frenet_host(f, layout):
    """f as a contiguous float64 array under `layout` -> (f, R, n)."""
    f = _np_f64(f)
    if layout == FRENET_SAMPLES and f.ndim == 3 and f.shape[1] == 6:
        return f, f.shape[0], f.shape[2]
    if layout == FRENET_STATES and f.ndim == 4 and f.shape[1] == 2 and f.shape[3] == 3:
        return f, f.shape[0], f.shape[2]
    raise ValueError("f must be [R, 6, n] (FRENET_SAMPLES) or [R, 2, n, 3] (FRENET_STATES), not %s under layout %r" % (f.shape, layout))


def _i32_host(a, R):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.shape != (R,):
        raise ValueError("count / line_index must be [R]")
    return a


def cartesian_host(f, refline, layout=FRENET_SAMPLES, count=None, line_index=None, want=("cart", "audit"), cart=None):
    """btrapz_cartesian_host(): the Cartesian stage on the host (no GPU).  f under `layout`; refline: a layout.RefLine.
    Returns a dict: "cart" [R, 6, n] (rows x, y, theta, kappa, v, a; `cart`: the array to write into, so that a caller
    sees what is left alone) and / or "audit", a dict of the KIN_AUDIT arrays."""
    f, R, n = _frenet_host(f, layout)
    t, keep = _refline_host(refline)
    count, line_index = _i32_host(count, R), _i32_host(line_index, R)
    out = {}
    if "cart" in want:
        out["cart"] = np.full((R, 6, n), np.nan) if cart is None else cart
        assert out["cart"].dtype == np.float64 and out["cart"].flags.c_contiguous and out["cart"].shape == (R, 6, n)
    au = None
    if "audit" in want:
        out["audit"] = {k: np.zeros(R) for k in KIN_AUDIT[:6]}
        out["audit"]["n_outside"] = np.zeros(R, dtype=np.int32)
        out["audit"]["worst"] = np.zeros((R, 6), dtype=np.int32)
        au = C.byref(CKinAudit(*[_np_ptr(out["audit"][k]) for k in KIN_AUDIT]))
    rc = lib().btrapz_cartesian_host(C.byref(t), _np_ptr(line_index), R, n, int(layout), _np_ptr(f), _np_ptr(count),
                                     _np_ptr(out.get("cart")), au)
    if rc != 0:
        raise BtrapzError("btrapz_cartesian_host -> %d (invalid argument)" % rc)
    return out


def cartesian_vjp_host(f, refline, cart_bar, layout=FRENET_SAMPLES, count=None, line_index=None):
    """btrapz_cartesian_vjp_host(): cart_bar [R, 6, n] -> f_bar, shaped like f."""
    f, R, n = _frenet_host(f, layout)
    t, keep = _refline_host(refline)
    count, line_index = _i32_host(count, R), _i32_host(line_index, R)
    cart_bar = _np_f64(cart_bar)
    if cart_bar.shape != (R, 6, n):
        raise ValueError("cart_bar must be [R, 6, n]")
    f_bar = np.full(f.shape, np.nan)
    rc = lib().btrapz_cartesian_vjp_host(C.byref(t), _np_ptr(line_index), R, n, int(layout), _np_ptr(f), _np_ptr(count),
                                         _np_ptr(cart_bar), _np_ptr(f_bar))
    if rc != 0:
        raise BtrapzError("btrapz_cartesian_vjp_host -> %d (invalid argument)" % rc)
    return f_bar


def cartesian_jvp_host(f, refline, f_dot, layout=FRENET_SAMPLES, count=None, line_index=None, cart_dot=None):
    """btrapz_cartesian_jvp_host(): f_dot [T] x the shape of f -> cart_dot [T, R, 6, n] (`cart_dot`: the array to write
    into; samples at and beyond a row's count keep what it holds)."""
    f, R, n = _frenet_host(f, layout)
    t, keep = _refline_host(refline)
    count, line_index = _i32_host(count, R), _i32_host(line_index, R)
    f_dot = _np_f64(f_dot)
    if f_dot.shape[1:] != f.shape:
        raise ValueError("f_dot must be [T] x the shape of f")
    T = f_dot.shape[0]
    out = np.full((T, R, 6, n), np.nan) if cart_dot is None else cart_dot
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (T, R, 6, n)
    rc = lib().btrapz_cartesian_jvp_host(C.byref(t), _np_ptr(line_index), R, n, int(layout), _np_ptr(f), _np_ptr(count), T,
                                         _np_ptr(f_dot), _np_ptr(out))
    if rc != 0:
        raise BtrapzError("btrapz_cartesian_jvp_host -> %d (invalid argument)" % rc)
    return out


def _frenet_shape(layout, R, n):
    return (R, 6, n) if layout == FRENET_SAMPLES else (R, 2, n, 3)


def _cart_host(cart):
    cart = _np_f64(cart)
    if cart.ndim != 3 or cart.shape[1] != 6:
        raise ValueError("cart must be [R, 6, n], not %s" % (cart.shape,))
    return cart, cart.shape[0], cart.shape[2]


def frenet_host(cart, refline, layout=FRENET_SAMPLES, order=2, count=None, line_index=None, s_window=None, frenet=None,
                interval=None):
    """btrapz_frenet_host(): the projection onto the reference line on the host (no GPU).  cart [R, 6, n] (rows x, y, theta,
    kappa, v, a; rows above the order are not read); refline: a layout.RefLine; s_window [R, 2] or None.  Returns a dict:
    "frenet" under `layout` (NaN at OUTSIDE samples), "interval" [R, n] int32 (-1: OUTSIDE), "n_outside" [R] int32.
    `frenet` / `interval`: the arrays to write into, so that a caller sees what is left alone."""
    if layout not in (FRENET_SAMPLES, FRENET_STATES):
        raise ValueError("layout: FRENET_SAMPLES or FRENET_STATES, not %r" % (layout,))
    cart, R, n = _cart_host(cart)
    t, keep = _refline_host(refline)
    count, line_index = _i32_host(count, R), _i32_host(line_index, R)
    s_window = _np_f64(s_window)
    if s_window is not None and s_window.shape != (R, 2):
        raise ValueError("s_window must be [R, 2]")
    out = dict(frenet=np.full(_frenet_shape(layout, R, n), np.nan) if frenet is None else frenet,
               interval=np.full((R, n), -1, dtype=np.int32) if interval is None else interval,
               n_outside=np.zeros(R, dtype=np.int32))
    assert out["frenet"].dtype == np.float64 and out["frenet"].flags.c_contiguous and out["frenet"].shape == _frenet_shape(layout, R, n)
    assert out["interval"].dtype == np.int32 and out["interval"].flags.c_contiguous and out["interval"].shape == (R, n)
    rc = lib().btrapz_frenet_host(C.byref(t), _np_ptr(line_index), R, n, int(layout), int(order), _np_ptr(cart), _np_ptr(count),
                                  _np_ptr(s_window), _np_ptr(out["frenet"]), _np_ptr(out["interval"]), _np_ptr(out["n_outside"]))
    if rc != 0:
        raise BtrapzError("btrapz_frenet_host -> %d (invalid argument)" % rc)
    return out


def _frenet_grad_host(cart, frenet, interval, layout):
    cart, R, n = _cart_host(cart)
    frenet = _np_f64(frenet)
    if layout not in (FRENET_SAMPLES, FRENET_STATES) or frenet.shape != _frenet_shape(layout, R, n):
        raise ValueError("frenet must be %s under layout %r, not %s" % (_frenet_shape(layout, R, n), layout, frenet.shape))
    interval = np.ascontiguousarray(interval, dtype=np.int32)
    if interval.shape != (R, n):
        raise ValueError("interval must be [R, n]")
    return cart, frenet, interval, R, n


def frenet_vjp_host(cart, refline, frenet, interval, frenet_bar, layout=FRENET_SAMPLES, order=2, count=None, line_index=None):
    """btrapz_frenet_vjp_host(): frenet_bar (shaped like frenet) -> cart_bar [R, 6, n]; cart, frenet and interval are the
    forward's."""
    cart, frenet, interval, R, n = _frenet_grad_host(cart, frenet, interval, layout)
    t, keep = _refline_host(refline)
    count, line_index = _i32_host(count, R), _i32_host(line_index, R)
    frenet_bar = _np_f64(frenet_bar)
    if frenet_bar.shape != frenet.shape:
        raise ValueError("frenet_bar must be shaped like frenet")
    cart_bar = np.full((R, 6, n), np.nan)
    rc = lib().btrapz_frenet_vjp_host(C.byref(t), _np_ptr(line_index), R, n, int(layout), int(order), _np_ptr(cart), _np_ptr(frenet),
                                      _np_ptr(interval), _np_ptr(count), _np_ptr(frenet_bar), _np_ptr(cart_bar))
    if rc != 0:
        raise BtrapzError("btrapz_frenet_vjp_host -> %d (invalid argument)" % rc)
    return cart_bar


def frenet_jvp_host(cart, refline, frenet, interval, cart_dot, layout=FRENET_SAMPLES, order=2, count=None, line_index=None,
                    frenet_dot=None):
    """btrapz_frenet_jvp_host(): cart_dot [T, R, 6, n] -> frenet_dot [T] x the shape of frenet (`frenet_dot`: the array to
    write into; samples at and beyond a row's count keep what it holds)."""
    cart, frenet, interval, R, n = _frenet_grad_host(cart, frenet, interval, layout)
    t, keep = _refline_host(refline)
    count, line_index = _i32_host(count, R), _i32_host(line_index, R)
    cart_dot = _np_f64(cart_dot)
    if cart_dot.ndim != 4 or cart_dot.shape[1:] != (R, 6, n):
        raise ValueError("cart_dot must be [T, R, 6, n]")
    T = cart_dot.shape[0]
    out = np.full((T,) + frenet.shape, np.nan) if frenet_dot is None else frenet_dot
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (T,) + frenet.shape
    rc = lib().btrapz_frenet_jvp_host(C.byref(t), _np_ptr(line_index), R, n, int(layout), int(order), _np_ptr(cart), _np_ptr(frenet),
                                      _np_ptr(interval), _np_ptr(count), T, _np_ptr(cart_dot), _np_ptr(out))
    if rc != 0:
        raise BtrapzError("btrapz_frenet_jvp_host -> %d (invalid argument)" % rc)
    return out


def footprint_struct(footprint):
    """(half_length, half_width, centre_offset) or (half_length, half_width) -> CFootprint."""
    if isinstance(footprint, CFootprint):
        return footprint
    f = tuple(float(v) for v in footprint)
    if len(f) == 2:
        f += (0.0,)
    if len(f) != 3:
        raise ValueError("footprint: (half_length, half_width[, centre_offset])")
    return CFootprint(*f)


def _obstacles_host(obstacles, n):
    """layout.Obstacles -> (CObstacles of host pointers, the arrays it points into)."""
    h = obstacles.host
    keep = (h["pose"], h["half"], h["obs_count"])
    return CObstacles(obstacles.n_scenes, obstacles.O, obstacles.n, h["pose"].ctypes.data, h["half"].ctypes.data,
                      h["obs_count"].ctypes.data if h["obs_count"] is not None else None), keep


def _which_host(which, R, n):
    which = np.ascontiguousarray(which, dtype=np.int32)
    if which.shape != (R, n):
        raise ValueError("which must be [R, n]")
    return which


def clearance_host(cart, obstacles, footprint, scene_index=None, count=None, d_safe=0.0, want=("clear", "which", "audit"),
                   clear=None, which=None):
    """btrapz_clearance_host(): the clearance stage on the host (no GPU).  cart [R, 6, n]; obstacles: a layout.Obstacles;
    footprint: (half_length, half_width, centre_offset).  Returns a dict: "clear" [R, n], "which" [R, n] int32 (`clear` /
    `which`: the arrays to write into, so that a caller sees what is left alone) and / or "audit", a dict of the
    CLEAR_AUDIT arrays."""
    cart, R, n = _cart_host(cart)
    ft = footprint_struct(footprint)
    ob, keep = _obstacles_host(obstacles, n)
    count, scene_index = _i32_host(count, R), _i32_host(scene_index, R)
    out = {}
    if "clear" in want:
        out["clear"] = np.full((R, n), np.nan) if clear is None else clear
        assert out["clear"].dtype == np.float64 and out["clear"].flags.c_contiguous and out["clear"].shape == (R, n)
    if "which" in want:
        out["which"] = np.full((R, n), -1, dtype=np.int32) if which is None else which
        assert out["which"].dtype == np.int32 and out["which"].flags.c_contiguous and out["which"].shape == (R, n)
    au = None
    if "audit" in want:
        out["audit"] = dict(clear_min=np.zeros(R), worst=np.zeros((R, 2), dtype=np.int32), n_below=np.zeros(R, dtype=np.int32),
                            n_invalid=np.zeros(R, dtype=np.int32))
        au = C.byref(CClearAudit(*[_np_ptr(out["audit"][k]) for k in CLEAR_AUDIT]))
    rc = lib().btrapz_clearance_host(C.byref(ft), C.byref(ob), _np_ptr(scene_index), R, n, _np_ptr(cart), _np_ptr(count),
                                     float(d_safe), _np_ptr(out.get("clear")), _np_ptr(out.get("which")), au)
    if rc != 0:
        raise BtrapzError("btrapz_clearance_host -> %d (invalid argument)" % rc)
    return out


def clearance_vjp_host(cart, obstacles, footprint, which, clear_bar, scene_index=None, count=None):
    """btrapz_clearance_vjp_host(): clear_bar [R, n] -> cart_bar [R, 6, n] under the forward's `which`."""
    cart, R, n = _cart_host(cart)
    ft = footprint_struct(footprint)
    ob, keep = _obstacles_host(obstacles, n)
    count, scene_index = _i32_host(count, R), _i32_host(scene_index, R)
    which = _which_host(which, R, n)
    clear_bar = _np_f64(clear_bar)
    if clear_bar.shape != (R, n):
        raise ValueError("clear_bar must be [R, n]")
    cart_bar = np.full((R, 6, n), np.nan)
    rc = lib().btrapz_clearance_vjp_host(C.byref(ft), C.byref(ob), _np_ptr(scene_index), R, n, _np_ptr(cart), _np_ptr(count),
                                         _np_ptr(which), _np_ptr(clear_bar), _np_ptr(cart_bar))
    if rc != 0:
        raise BtrapzError("btrapz_clearance_vjp_host -> %d (invalid argument)" % rc)
    return cart_bar


def clearance_jvp_host(cart, obstacles, footprint, which, cart_dot, obs_dot=None, scene_index=None, count=None, clear_dot=None):
    """btrapz_clearance_jvp_host(): cart_dot [T, R, 6, n] and obs_dot [T, n_scenes, O, 3, n] or None -> clear_dot [T, R, n]
    (`clear_dot`: the array to write into; samples at and beyond a row's count keep what it holds)."""
    cart, R, n = _cart_host(cart)
    ft = footprint_struct(footprint)
    ob, keep = _obstacles_host(obstacles, n)
    count, scene_index = _i32_host(count, R), _i32_host(scene_index, R)
    which = _which_host(which, R, n)
    cart_dot = _np_f64(cart_dot)
    if cart_dot.ndim != 4 or cart_dot.shape[1:] != (R, 6, n):
        raise ValueError("cart_dot must be [T, R, 6, n]")
    T = cart_dot.shape[0]
    obs_dot = _np_f64(obs_dot)
    if obs_dot is not None and obs_dot.shape != (T, obstacles.n_scenes, obstacles.O, 3, n):
        raise ValueError("obs_dot must be [T, n_scenes, O, 3, n]")
    out = np.full((T, R, n), np.nan) if clear_dot is None else clear_dot
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (T, R, n)
    rc = lib().btrapz_clearance_jvp_host(C.byref(ft), C.byref(ob), _np_ptr(scene_index), R, n, _np_ptr(cart), _np_ptr(count),
                                         _np_ptr(which), T, _np_ptr(cart_dot), _np_ptr(obs_dot), _np_ptr(out))
    if rc != 0:
        raise BtrapzError("btrapz_clearance_jvp_host -> %d (invalid argument)" % rc)
    return out
