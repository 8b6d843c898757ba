"""ctypes binding of the C ABI in include/boundmpc_hip.h (libboundmpc_hip.so).

There is deliberately NO CPU fallback: if the HIP extension is missing or no GPU is present
the import / create call raises."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BOUNDMPC_HIP_LIB") or os.path.join(HERE, "csrc", "libboundmpc_hip.so")   # override: A/B builds of the same source


class Options(ctypes.Structure):
    _fields_ = [("tol", ctypes.c_double), ("max_iter", ctypes.c_int), ("mu_init", ctypes.c_double),
                ("mu_min_fac", ctypes.c_double), ("slack_push", ctypes.c_double),
                ("exact_hessian", ctypes.c_int), ("verbose", ctypes.c_int), ("mu_warm", ctypes.c_double), ("stall_window", ctypes.c_int),
                ("bound_margin", ctypes.c_double)]


_vp, _ci, _cd, _P = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.POINTER
_SOLVE_OUT = [_vp] * 8          # x, g, lam_g, lam_x, f, iters, status, kkt
_TICK = [_vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _ci]      # handle, B, path, entries, ... traj, flags
# the C ABI of include/boundmpc_hip.h: name -> (restype, argtypes)
SIGNATURES = {
    "bmpc_default_options": (_ci, [_P(Options)]), "bmpc_default_options_for": (_ci, [_ci, _P(Options)]), "bmpc_options_size": (_ci, []),
    "bmpc_error_string": (ctypes.c_char_p, [_ci]), "bmpc_build_hash": (ctypes.c_char_p, []),
    "bmpc_create": (_ci, [_ci, _ci, _cd, _P(Options), _P(_vp)]), "bmpc_destroy": (_ci, [_vp]),
    "bmpc_num_vars": (_ci, [_vp]), "bmpc_num_cons": (_ci, [_vp]), "bmpc_num_params": (_ci, [_vp]), "bmpc_state_len": (_ci, [_vp]),
    "bmpc_get_bounds": (_ci, [_vp] * 5), "bmpc_launch_info": (_ci, [_vp, _P(_ci), _P(_ci), _P(ctypes.c_longlong)]),
    "bmpc_solve_batch": (_ci, [_vp, _ci, _vp, _vp] + _SOLVE_OUT + [_vp]), "bmpc_solve_batch_host": (_ci, [_vp, _ci, _vp, _vp] + _SOLVE_OUT),
    "bmpc_solve_batch_warm": (_ci, [_vp, _ci, _vp, _vp, _vp, _ci] + _SOLVE_OUT + [_vp]),
    "bmpc_solve_batch_host_dual": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp] + _SOLVE_OUT),
    "bmpc_state_from_multipliers": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp, _cd, _vp, _vp]),
    "bmpc_graph_create": (_ci, [_vp, _ci, _vp, _vp, _vp, _ci] + _SOLVE_OUT + [_P(_vp)]), "bmpc_graph_launch": (_ci, [_vp, _vp]), "bmpc_graph_destroy": (_ci, [_vp]),
    "bmpc_kkt_len": (_ci, []), "bmpc_kkt_batch": (_ci, [_vp, _ci] + [_vp] * 9), "bmpc_kkt_batch_host": (_ci, [_vp, _ci] + [_vp] * 8),
    "bmpc_sens_len": (_ci, []), "bmpc_sens_batch": (_ci, [_vp, _ci] + [_vp] * 5 + [_cd] + [_vp] * 5), "bmpc_sens_batch_host": (_ci, [_vp, _ci] + [_vp] * 5 + [_cd] + [_vp] * 4),
    "bmpc_stream_lengths": (_ci, [_vp] + [_P(_ci)] * 4), "bmpc_stream_pack": (_ci, [_vp, _ci, _vp, _ci] + [_vp] * 6), "bmpc_stream_pack_rt": (_ci, [_vp, _ci, _vp, _ci] + [_vp] * 7),
    "bmpc_stream_post": (_ci, [_vp, _ci, _vp, _ci] + [_vp] * 6 + [_ci, _vp]), "bmpc_stream_tick": (_ci, _TICK + [_vp]), "bmpc_stream_graph_create": (_ci, _TICK + [_P(_vp)]),
    "bmpc_stream_rollout_len": (_ci, []), "bmpc_stream_rollout": (_ci, _TICK[:2] + [_ci] + _TICK[2:] + [_cd, _vp, _vp, _vp, _vp]),      # handle, B, ticks, path ... flags, goal_tol, hist, traj_hist, ticks_run, stream
    "bmpc_stream_log_len": (_ci, [_vp]), "bmpc_stream_log": (_ci, [_vp, _ci, _vp, _ci] + [_vp] * 5),
    "bmpc_stream_rollout_events": (_ci, _TICK[:2] + [_ci] + _TICK[2:] + [_cd, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp]),      # ... ticks_run, replan, replan_tick, replan_info, update_flags, disturb, stream
    "bmpc_stream_rollout_audit": (_ci, _TICK[:2] + [_ci] + _TICK[2:] + [_cd, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _cd, _vp]),      # ... disturb, tube_hist, audit, audit_tol, stream
    "bmpc_stream_rollout_log": (_ci, _TICK[:2] + [_ci] + _TICK[2:] + [_cd, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _cd, _vp, _ci, _vp, _vp]),      # ... audit_tol, log_hist, log_stages, track, stream
    "bmpc_stream_rollout_legs": (_ci, _TICK[:2] + [_ci] + _TICK[2:] + [_cd, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _cd, _vp, _ci, _vp] + [_ci] + [_vp] * 7),      # ... ticks_run, replan, replan_info, update_flags, disturb, tube_hist, audit, audit_tol, log_hist, log_stages, track, legs, leg_tick, leg_on, leg_tol, legs_done, leg_fired, leg_why, stream
    "bmpc_stream_rollout_tuned": (_ci, _TICK[:2] + [_ci] + _TICK[2:] + [_cd, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _cd, _vp, _ci, _vp] + [_ci] + [_vp] * 10),      # ... leg_why, tune, tune_info, tune_used, stream
    "bmpc_stream_rollout_plant": (_ci, _TICK[:2] + [_ci] + _TICK[2:] + [_cd, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _cd, _vp, _ci, _vp] + [_ci] + [_vp] * 14),      # ... tune_used, plant, plant_state, plant_info, plant_rec, stream
    "bmpc_stream_plant_len": (_ci, []), "bmpc_stream_plant_state_len": (_ci, []), "bmpc_stream_plant_rec_len": (_ci, []),
    "bmpc_stream_plant": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp]),      # handle, B, robot, sstate, plant, plant_state, plant_info, plant_rec, tick, stream
    "bmpc_stream_rollout_sensor": (_ci, _TICK[:2] + [_ci] + _TICK[2:] + [_cd, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _cd, _vp, _ci, _vp] + [_ci] + [_vp] * 20),      # ... plant_rec, sensor, sensor_state, sensor_info, sensor_rec, sensor_noise, meas_hist, stream
    "bmpc_stream_sensor_len": (_ci, []), "bmpc_stream_sensor_state_len": (_ci, []), "bmpc_stream_sensor_rec_len": (_ci, []),
    "bmpc_stream_sense": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp]),      # handle, B, robot, sstate, sensor, sensor_state, sensor_info, sensor_rec, sensor_noise, meas, tick, stream
    "bmpc_stream_unsense": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp, _vp]),      # handle, B, robot, sstate, sensor, sensor_state, stream
    "bmpc_stream_rollout_observer": (_ci, _TICK[:2] + [_ci] + _TICK[2:] + [_cd, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _cd, _vp, _ci, _vp] + [_ci] + [_vp] * 25),      # ... meas_hist, observer, observer_state, observer_info, observer_rec, sample_hist, stream
    "bmpc_stream_observer_len": (_ci, []), "bmpc_stream_observer_state_len": (_ci, []), "bmpc_stream_observer_rec_len": (_ci, []),
    "bmpc_stream_observe": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp]),      # the arguments of bmpc_stream_sense up to tick, observer, observer_state, observer_info, observer_rec, sample, stream
    "bmpc_stream_tune_len": (_ci, []), "bmpc_stream_tune_defaults": (_ci, [_vp, _ci, _vp]),
    "bmpc_stream_track_len": (_ci, []), "bmpc_stream_rollout_log_len": (_ci, [_vp, _ci]),
    "bmpc_stream_tube_len": (_ci, []), "bmpc_stream_tube": (_ci, [_vp, _ci, _vp, _vp, _vp, _vp]),
    "bmpc_stream_disturb_len": (_ci, []), "bmpc_stream_disturb": (_ci, [_vp, _ci, _vp, _vp, _vp]),
    "bmpc_stream_replan_len": (_ci, [_vp, _ci]), "bmpc_stream_update": (_ci, [_vp, _ci, _vp, _vp, _ci, _vp, _vp, _vp, _ci, _vp]),
    "bmpc_stream_set_rt_feasibility_tol": (_ci, [_vp, _cd]), "bmpc_stream_set_rt_position_row_cap": (_ci, [_vp, _cd]), "bmpc_stream_set_time_budget": (_ci, [_vp, _cd]),
    "bmpc_stream_set_level_rule": (_ci, [_vp, _cd, _cd, _cd]), "bmpc_set_barrier_hold": (_ci, [_vp, _ci]),
    "bmpc_set_latency_buffer": (_ci, [_vp, _vp]), "bmpc_set_timing": (_ci, [_vp, _ci]), "bmpc_last_kernel_ms": (_ci, [_vp, _P(ctypes.c_float)]), "bmpc_kernel_ms": (_ci, [_vp, _ci, _P(ctypes.c_float)]),
    "bmpc_set_team_waves": (_ci, [_vp, _ci]), "bmpc_set_rollout_waves": (_ci, [_vp, _ci]), "bmpc_get_rollout_waves": (_ci, [_vp]),
    "bmpc_team_info": (_ci, [_vp, _ci, _P(_ci), _P(_ci), _P(_ci)]),
    "bmpc_set_restoration": (_ci, [_vp, _ci, _ci, _ci]), "bmpc_get_restoration": (_ci, [_vp, _P(_ci), _P(_ci), _P(_ci)]),
    "bmpc_set_start_rollout": (_ci, [_vp, _ci]), "bmpc_get_start_rollout": (_ci, [_vp]), "bmpc_set_queue_order": (_ci, [_vp, _ci]), "bmpc_get_queue_order": (_ci, [_vp]),
    "bmpc_set_second_attempt": (_ci, [_vp, _ci]), "bmpc_get_second_attempt": (_ci, [_vp]),
}
SYMBOLS = list(SIGNATURES)


class BoundMPCHipError(RuntimeError):
    pass


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own HIP runtime; import it FIRST so that this process has exactly one libamdhip64
    # (loading the system runtime before torch's leaves the second one without devices).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise BoundMPCHipError(
            f"HIP extension {LIB_PATH} is missing - build it with `python -m boundmpc_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    in_tree = not os.environ.get("BOUNDMPC_HIP_LIB")      # (a library given by hand -- the A/B build of an older revision, tests/gpu_ab.py -- may lack entry points and is not tied to the tree)
    for name, (restype, argtypes) in SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        elif in_tree:
            raise BoundMPCHipError(f"{LIB_PATH} does not export {name} (stale build?): rebuild with `python -m boundmpc_amd.build`")
    if hasattr(lib, "bmpc_build_hash"):
        from . import build as _build
        want, have = _build.source_hash(), lib.bmpc_build_hash().decode()
        if in_tree and want != have:
            raise BoundMPCHipError(f"{LIB_PATH} was built from other sources or flags (library {have}, tree {want}): rebuild with `python -m boundmpc_amd.build`")
        if lib.bmpc_options_size() != ctypes.sizeof(Options):
            raise BoundMPCHipError(f"{LIB_PATH}: bmpc_options is {lib.bmpc_options_size()} bytes, this binding expects {ctypes.sizeof(Options)} (stale build?)")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise BoundMPCHipError(f"{what} failed: {load().bmpc_error_string(rc).decode()} (code {rc})")
