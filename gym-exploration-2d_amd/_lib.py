"""ctypes binding of libcagym_hip.so (include/cagym.h).  No fallback: a missing library raises."""
import ctypes as C
import os

import torch  # (before the library is loaded: load() binds to the HIP runtime torch already mapped)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CAGYM_LIB") or os.path.join(HERE, "csrc", "libcagym_hip.so")  # CAGYM_LIB: diagnostic builds

EGO_WIDTH = 12
FLAG_AT_GOAL, FLAG_IN_COLLISION, FLAG_RAN_OUT_OF_TIME, FLAG_DONE = 1, 2, 4, 8
FLAG_WAS_AT_GOAL, FLAG_WAS_IN_COLLISION, FLAG_ACTIVE = 16, 32, 64
GO_AGENT0, GO_ALL, GO_LEARNING = 0, 1, 2


class CagymConfig(C.Structure):
    _fields_ = [("n_worlds", C.c_int32), ("max_agents", C.c_int32), ("n_scenarios", C.c_int32),
                ("max_obstacles", C.c_int32), ("game_over_mode", C.c_int32), ("collide_with_static", C.c_int32),
                ("laserscan", C.c_int32), ("device", C.c_int32), ("dt", C.c_double),
                ("rvo_max_neighbors", C.c_int32), ("reserved", C.c_int32)]


class CagymOutputs(C.Structure):
    _fields_ = [("obs_oas", C.c_void_p), ("obs_ego", C.c_void_p), ("laserscan", C.c_void_p),
                ("reward", C.c_void_p), ("flags", C.c_void_p), ("game_over", C.c_void_p)]


class _DevArray(object):
    """Minimal __cuda_array_interface__ holder: zero-copy torch view of a raw device pointer."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<" + typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


def views(ptrs, fields, device, **sizes):
    """Zero-copy device tensors of a struct of device pointers (or a dict of addresses): one per row (name, typestr, shape) of
    `fields`.  A shape spells its dims: a letter is looked up in `sizes`, a digit or an int stands for itself.  u4 / u8 words come
    as int32 / int64: the bits, in the signed types torch computes with.  A null pointer gives no entry."""
    out = {}
    for name, ts, shape in fields:
        p = ptrs[name] if isinstance(ptrs, dict) else getattr(ptrs, name)
        if p:
            shape = [c if isinstance(c, int) else int(c) if c.isdigit() else sizes[c] for c in shape]
            out[name] = torch.as_tensor(_DevArray(p, shape, {"u4": "i4", "u8": "i8"}.get(ts, ts)), device=device)
    return out


# The field tables of the pointer structs and address lists: N worlds, M agents, S pool slots, K max_obstacles, L ring rows, C = 13.
STATE_FIELDS = [("pos_x", "f8", "NM"), ("pos_y", "f8", "NM"), ("vel_x", "f8", "NM"), ("vel_y", "f8", "NM"), ("heading", "f8", "NM"),
                ("heading_ego", "f8", "NM"), ("dist_to_goal", "f8", "NM"), ("time_remaining", "f8", "NM"), ("t", "f8", "NM"),
                ("goal_x", "f8", "NM"), ("goal_y", "f8", "NM"), ("radius", "f8", "NM"), ("pref_speed", "f8", "NM"), ("speed", "f8", "NM"),
                ("delta_heading", "f8", "NM"), ("aux0", "f8", "NM"), ("aux1", "f8", "NM"), ("action", "f4", "NM2"), ("status", "u4", "NM"),
                ("step_num", "i4", "NM"), ("n_agents", "i4", "N"), ("n_observed", "i4", "NM"), ("episode", "i4", "N"),
                ("map_bits", "u4", ("S", 300, 10)), ("stat_return", "f4", "N"), ("stat_episodes", "i4", "N"), ("stat_steps", "i4", "N"),
                ("stat_outcomes", "i4", "N3")]
SCENARIO_FIELDS = [("agents6", "f8", "SM6"), ("policy", "i4", "SM"), ("dynamics", "i4", "SM"), ("n_agents", "i4", "S"), ("coop", "f8", "SM")]
OBSTACLE_FIELDS = [("obstacles", "f8", "SK4"), ("n_obst", "i4", "S")]             # cagym_get_obstacles' two addresses
STREAM_FIELDS = [("next_episode", "i4", "N"), ("generated", "i8", "1"), ("n_failed", "i4", "1"), ("n_lapped", "i4", "1")]
EXPLORE_STREAM_FIELDS = [("field_next", "i4", "N"), ("fields_built", "i8", "1")]  # cagym_explore_stream_get's
# cagym_stream_replay_get's addresses (Q = the buffer's capacity); REPLAY_WORDS names the six u64 of `words`
REPLAY_FIELDS = [("buf_key", "u4", "Q"), ("words", "u8", "6"), ("slot_key", "u4", "S"), ("slot_gen", "u4", "S")]
REPLAY_WORDS = ("count", "harvested", "pushed", "replayed", "n_missed", "n_stale")
REPLAY_OUTCOMES = {"collision": 1, "goal": 2, "stuck": 4}  # the episode log's outcome bits
IG_FIELDS = [("edf_d2", "i4", ("S", 300, 300)), ("belief", "f8", ("N", 60, 60))]  # cagym_ig_get's
IG_EPISODE_FIELDS = [("running", "f8", "N"), ("sum", "f8", "N"), ("last", "f8", "N"), ("episodes", "i4", "N")]  # cagym_ig_get_episode_stats'


class CagymStatePtrs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _, _ in STATE_FIELDS]


class CagymGenParams(C.Structure):
    """cagym_gen_params (include/cagym.h)."""
    _fields_ = [("seed", C.c_uint64), ("n_min", C.c_int32), ("n_max", C.c_int32), ("ego_policy", C.c_int32),
                ("ego_dynamics", C.c_int32), ("policy_a", C.c_int32), ("policy_b", C.c_int32),
                ("other_dynamics", C.c_int32), ("max_tries", C.c_int32), ("p_b", C.c_double), ("side", C.c_double),
                ("min_travel", C.c_double), ("min_sep", C.c_double), ("radius", C.c_double), ("pref_speed", C.c_double),
                ("coop", C.c_double)]


class CagymGen2Params(C.Structure):
    """cagym_gen2_params (include/cagym.h)."""
    _fields_ = [("seed", C.c_uint64), ("kinds_mask", C.c_uint32), ("number_of_agents", C.c_int32), ("fixed_count", C.c_int32),
                ("ego_policy", C.c_int32), ("ego_dynamics", C.c_int32), ("override_policies", C.c_int32), ("policy_a", C.c_int32),
                ("policy_b", C.c_int32), ("other_dynamics", C.c_int32), ("n_obst_min", C.c_int32), ("n_obst_max", C.c_int32),
                ("max_tries", C.c_int32), ("p_b", C.c_double)]


class CagymExploreParams(C.Structure):
    """cagym_explore_params (include/cagym.h)."""
    _fields_ = [("seed", C.c_uint64), ("kinds_mask", C.c_uint32), ("n_robots", C.c_int32), ("n_targets", C.c_int32),
                ("n_obst_min", C.c_int32), ("n_obst_max", C.c_int32), ("max_tries", C.c_int32), ("target_radius", C.c_double),
                ("robot_pref_speed", C.c_double)]


class CagymScenarioPtrs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _, _ in SCENARIO_FIELDS]


EPREC_KEEP = {"first": 0, "last": 1}  # CAGYM_EPREC_KEEP_*
# cagym_episode_record_ptrs: (field, typestr, shape in terms of S / N / M)
EPREC_FIELDS = [("t", "f8", "SM"), ("extra_t", "f8", "SM"), ("flags", "u1", "SM"), ("ret", "f8", "S"), ("steps", "i4", "S"),
                ("outcome", "i4", "S"), ("count", "i4", "S"), ("t_run", "f8", "NM"), ("ret_run", "f8", "N"),
                ("steps_run", "i4", "N"), ("atgoal_run", "u4", "N"), ("cursor", "i4", "N"), ("desync", "i4", "1")]


class CagymEpisodeRecordPtrs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _, _ in EPREC_FIELDS]


# cagym_episode_log_ptrs: (field, typestr, shape in terms of L / N / M); the int32 capacity closes the struct
EPLOG_FIELDS = [("key", "u4", "L"), ("world", "i4", "L"), ("episode", "i4", "L"), ("slice", "i8", "L"), ("steps", "i4", "L"),
                ("ret", "f8", "L"), ("outcome", "i4", "L"), ("n_agents", "i4", "L"), ("n_obst", "i4", "L"), ("t", "f8", "LM"),
                ("extra_t", "f8", "LM"), ("flags", "u1", "LM"), ("t_run", "f8", "NM"), ("ret_run", "f8", "N"),
                ("steps_run", "i4", "N"), ("atgoal_run", "u4", "N"), ("cursor", "i4", "N"), ("head", "u8", "1"), ("desync", "i4", "1")]


class CagymEpisodeLogPtrs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _, _ in EPLOG_FIELDS] + [("capacity", C.c_int32)]


class DmctsParams(C.Structure):
    """cagym_dmcts_params (include/cagym.h)."""
    _fields_ = [(n, C.c_int32) for n in ("n_robots", "Ntree", "Nsims", "horizon", "Ncycles", "comm_n", "xdt", "reset_comms")] + \
               [("call_base", C.c_uint32), ("parallel_agents", C.c_uint32)] + \
               [(n, C.c_double) for n in ("c_p", "gamma", "radius", "dt", "fov_rad", "range")] + [("seed", C.c_uint64)]


class GreedyParams(C.Structure):
    """cagym_ig_greedy_params (include/cagym.h)."""
    _fields_ = [("n_robots", C.c_int32), ("coordinate", C.c_int32)] + \
               [(n, C.c_double) for n in ("dt", "radius", "fov_rad", "range")] + [("v", C.c_double * 3), ("w", C.c_double * 3)]


class IgObserveParams(C.Structure):
    """cagym_ig_observe_params (include/cagym_ig_observe.h; not in STRUCTS, which mirrors the structs cagym.h itself defines)."""
    _fields_ = [("n_robots", C.c_int32), ("window", C.c_int32), ("rotate", C.c_int32), ("flags", C.c_uint32)] + \
               [(n, C.c_double) for n in ("detect_range", "fov_rad", "range")]


IG_OBSERVE_ONLY_RESTARTED = 4  # CAGYM_IG_OBSERVE_ONLY_RESTARTED


class IgContextParams(C.Structure):
    """cagym_ig_context_params (include/cagym_ig_context.h; not in STRUCTS, as IgObserveParams)."""
    _fields_ = [("n_robots", C.c_int32), ("window", C.c_int32), ("rotate", C.c_int32), ("flags", C.c_uint32), ("clear_max", C.c_double)]


IG_CONTEXT_ONLY_MASKED = 1  # CAGYM_IG_CONTEXT_ONLY_MASKED


class IgGoalParams(C.Structure):
    """cagym_ig_goal_params (include/cagym_ig_goals.h; not in STRUCTS, as IgObserveParams)."""
    _fields_ = [("n_robots", C.c_int32), ("window", C.c_int32), ("rotate", C.c_int32), ("flags", C.c_uint32), ("radius", C.c_double),
                ("v_max", C.c_double), ("w_max", C.c_double), ("align_tol", C.c_double), ("goal_tol", C.c_double), ("dt", C.c_double)]


class IgViewParams(C.Structure):
    """cagym_ig_view_params (include/cagym_ig_viewpoints.h; not in STRUCTS, as IgObserveParams)."""
    _fields_ = [("n_points", C.c_int32), ("n_robots", C.c_int32), ("k", C.c_int32), ("flags", C.c_uint32), ("radius", C.c_double),
                ("range", C.c_double), ("min_sep", C.c_double), ("d0", C.c_double)]


class IgHeadingParams(C.Structure):
    """cagym_ig_heading_params (include/cagym_ig_headings.h; not in STRUCTS, as IgObserveParams)."""
    _fields_ = [("n_points", C.c_int32), ("n_headings", C.c_int32), ("flags", C.c_uint32), ("radius", C.c_double),
                ("range", C.c_double), ("fov", C.c_double), ("headings", C.c_double * 16)]


class IgAssignParams(C.Structure):
    """cagym_ig_assign_params (include/cagym_ig_assign.h; not in STRUCTS, as IgObserveParams)."""
    _fields_ = [("n_robots", C.c_int32), ("k", C.c_int32), ("mode", C.c_int32), ("flags", C.c_uint32), ("radius", C.c_double),
                ("range", C.c_double), ("d0", C.c_double), ("fov", C.c_double)]


IG_ASSIGN_MODES = {"slot": 0, "best": 1}  # CAGYM_IG_ASSIGN_SLOT / CAGYM_IG_ASSIGN_BEST


class IgRouteParams(C.Structure):
    """cagym_ig_route_params (include/cagym_ig_route.h; not in STRUCTS, as IgObserveParams)."""
    _fields_ = [("n_robots", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32), ("flags", C.c_uint32), ("radius", C.c_double),
                ("range", C.c_double), ("fov", C.c_double), ("d0", C.c_double)]


IG_ROUTE_MAX_WAYPOINTS = 16  # CAGYM_IG_ROUTE_MAX_WAYPOINTS


class IgCreditParams(C.Structure):
    """cagym_ig_credit_params (include/cagym_ig_credit.h; not in STRUCTS, as IgObserveParams)."""
    _fields_ = [("n_robots", C.c_int32), ("flags", C.c_uint32), ("detect_range", C.c_float), ("fov_rad", C.c_double), ("range", C.c_double)]


# cagym_ig_episode_log_ptrs (include/cagym_ig_episode_log.h): (field, typestr, shape in terms of L / N / M); the int32 capacity closes it
IGLOG_FIELDS = [("key", "u4", "L"), ("world", "i4", "L"), ("episode", "i4", "L"), ("slice", "i8", "L"), ("steps", "i4", "L"),
                ("ret", "f8", "L"), ("n_targets", "i4", "L"), ("n_found", "i4", "L"), ("found_at", "i4", "LM"), ("entropy", "f8", "L"),
                ("residual_mi", "f8", "L"), ("n_touched", "i4", "L"), ("steps_run", "i4", "N"), ("found_run", "i4", "NM"),
                ("cursor", "i4", "N"), ("head", "u8", "1"), ("desync", "i4", "1")]


class CagymIgEpisodeLogPtrs(C.Structure):
    """cagym_ig_episode_log_ptrs (not in STRUCTS, which mirrors the structs cagym.h itself defines)."""
    _fields_ = [(n, C.c_void_p) for n, _, _ in IGLOG_FIELDS] + [("capacity", C.c_int32)]


SNAP_MAGIC, SNAP_VERSION, SNAP_CORE, SNAP_IG = 0x43475331, 1, 1, 2  # CAGYM_SNAP_*


CKPT_SECTIONS = ("host", "state", "pool", "stream", "log", "replay")  # CAGYM_CKPT_*: the entries of cagym_checkpoint_sizes


class CagymSnapshotLayout(C.Structure):
    """cagym_snapshot_layout (include/cagym.h)."""
    _fields_ = [("magic", C.c_uint32), ("version", C.c_uint32), ("n_worlds", C.c_int32), ("max_agents", C.c_int32),
                ("n_scenarios", C.c_int32), ("max_obstacles", C.c_int32), ("fields", C.c_uint32), ("reserved", C.c_uint32),
                ("row_bytes", C.c_uint64)]


class CagymStreamPtrs(C.Structure):
    """cagym_stream_ptrs (include/cagym.h)."""
    _fields_ = [(n, C.c_void_p) for n, _, _ in STREAM_FIELDS]


class CagymTerminalOutputs(C.Structure):
    """cagym_terminal_outputs (include/cagym.h)."""
    _fields_ = [("obs_oas", C.c_void_p), ("obs_ego", C.c_void_p), ("laserscan", C.c_void_p)]


TRAJ_COLUMNS = ("t", "pos_x", "pos_y", "goal_x", "goal_y", "radius", "pref_speed", "vel_x", "vel_y", "speed", "heading", "a0", "a1")
# cagym_trajectory_ptrs: (field, typestr, shape in terms of L / C = 13 columns / N / M); the int32 n_slices closes the struct
TRAJ_FIELDS = [("rows", "f8", "LCNM"), ("moved", "u1", "LNM"), ("episode", "i4", "LN"), ("last", "u1", "LN"), ("head", "u8", "1"),
               ("desync", "i4", "1"), ("t_prev", "f8", "NM"), ("seen", "i4", "NM")]


class CagymTrajectoryPtrs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _, _ in TRAJ_FIELDS] + [("n_slices", C.c_int32)]


STRUCTS = {"cagym_config": CagymConfig, "cagym_outputs": CagymOutputs, "cagym_state_ptrs": CagymStatePtrs,
           "cagym_scenario_ptrs": CagymScenarioPtrs, "cagym_gen_params": CagymGenParams, "cagym_gen2_params": CagymGen2Params,
           "cagym_explore_params": CagymExploreParams, "cagym_dmcts_params": DmctsParams, "cagym_ig_greedy_params": GreedyParams,
           "cagym_episode_record_ptrs": CagymEpisodeRecordPtrs, "cagym_episode_log_ptrs": CagymEpisodeLogPtrs,
           "cagym_snapshot_layout": CagymSnapshotLayout, "cagym_stream_ptrs": CagymStreamPtrs,
           "cagym_terminal_outputs": CagymTerminalOutputs, "cagym_trajectory_ptrs": CagymTrajectoryPtrs}  # every struct of include/cagym.h

# ---- the prototypes of include/cagym.h: name -> argtypes; every function returns int except those of _RESTYPES ----------------
_vp, _int, _dbl, _P = C.c_void_p, C.c_int, C.c_double, C.POINTER
_OUT = _P(CagymOutputs)
_RESTYPES = {"cagym_last_error": C.c_char_p, "cagym_ga3c_act_workspace_bytes": C.c_size_t,
             "cagym_dmcts_workspace_bytes": C.c_size_t}
_ARGTYPES = {
    "cagym_version": [],
    "cagym_create": [_P(CagymConfig), _P(_vp)],
    "cagym_destroy": [_vp],
    "cagym_last_error": [_vp],
    "cagym_set_scenarios": [_vp] * 10,
    "cagym_reset": [_vp, _vp, _int, _OUT, _vp],
    "cagym_step": [_vp, _vp, _OUT, _vp],
    "cagym_step_autoreset": [_vp, _vp, _OUT, _vp],
    "cagym_step_begin": [_vp, _vp],
    "cagym_step_finish": [_vp, _vp, _OUT, _int, _vp],
    "cagym_rollout": [_vp, _int, _int, _OUT, _vp],
    "cagym_get_state": [_vp, _P(CagymStatePtrs)],
    "cagym_pack_episode_stats": [_vp, _vp, _vp],
    "cagym_kernel_name": [_vp, _int, _int, C.c_char_p, _int],
    "cagym_laserscan": [_vp, _vp, _vp],
    "cagym_occupancy_grid": [_vp, _vp, _vp],
    "cagym_generate_scenarios": [_vp, _P(CagymGenParams), _P(C.c_int32), _vp],
    "cagym_get_scenarios": [_vp, _P(CagymScenarioPtrs)],
    "cagym_generate_reference_scenarios": [_vp, _P(CagymGen2Params), _P(C.c_int32), _vp],
    "cagym_get_obstacles": [_vp, _P(_vp), _P(_vp)],
    "cagym_ga3c_state": [_vp, _int, _vp, _vp],
    "cagym_ga3c_load_weights": [_vp, _vp, _vp],
    "cagym_ga3c_forward": [_vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp],
    "cagym_ga3c_act_workspace_bytes": [_vp],
    "cagym_ga3c_act": [_vp, _vp, _int, _vp, _vp, _vp],
    "cagym_ga3c_act_merge": [_vp, _vp, _int, _vp, _vp, _vp, _vp],
    "cagym_ig_init": [_vp, _vp],
    "cagym_ig_reset_belief": [_vp, _vp, _vp],
    "cagym_ig_get": [_vp, _P(_vp), _P(_vp)],
    "cagym_ig_get_episode_stats": [_vp] + [_P(_vp)] * 4,
    "cagym_ig_visible_cells": [_vp, _vp, _vp, _int, _dbl, _dbl, _vp, _vp],
    "cagym_ig_update_belief": [_vp, _vp, _vp, _vp, _vp, _int, _int, _dbl, _dbl, _vp, _vp],
    "cagym_ig_mi_reward": [_vp, _vp, _vp, _int, _vp, _vp],
    "cagym_ig_next_pose": [_vp, _vp, _vp, _vp, _vp, _int, _int, _dbl, _vp, _vp, _vp],
    "cagym_ig_rollouts": [_vp] * 7 + [_int] * 4 + [_dbl] * 3 + [C.c_uint64, _vp, _vp, _vp, _vp, _vp],
    "cagym_ig_robot_inputs": [_vp, _int, _dbl, _vp, _vp, _vp, _vp, _vp],
    "cagym_ig_robot_actions": [_vp, _int, _vp, _vp, _vp],
    "cagym_ig_episode_boundary": [_vp, _vp, _vp, _vp, C.c_uint32, _vp, C.c_size_t, _vp],
    "cagym_ig_greedy_plan": [_vp, _P(GreedyParams), _vp, _vp, _vp, _vp, _vp, _vp],
    "cagym_ig_observe": [_vp, _P(IgObserveParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "cagym_ig_context_window": [_vp, _P(IgContextParams), _vp, _vp, _vp, _vp],
    "cagym_ig_geodesic": [_vp, _P(IgGoalParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "cagym_ig_goal_actions": [_vp, _P(IgGoalParams), _vp, _vp, _vp, _vp, _vp, _vp],
    "cagym_ig_goal_status": [_vp, _P(IgGoalParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "cagym_ig_view_gain": [_vp, _P(IgViewParams), _vp, _vp, _vp, _vp, _vp, _vp],
    "cagym_ig_propose_goals": [_vp, _P(IgViewParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "cagym_ig_view_gain_headings": [_vp, _P(IgHeadingParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "cagym_ig_assign_goals": [_vp, _P(IgAssignParams)] + [_vp] * 15,
    "cagym_ig_route_gains": [_vp, _P(IgRouteParams)] + [_vp] * 17,
    "cagym_ig_credit": [_vp, _P(IgCreditParams)] + [_vp] * 12,
    "cagym_ig_goal_face_actions": [_vp, _P(IgGoalParams), _vp, _vp, _vp, _vp, _vp],
    "cagym_ig_goal_face_status": [_vp, _P(IgGoalParams), C.c_double, _vp, _vp, _vp, _vp, _vp],
    "cagym_dmcts_workspace_bytes": [_int, _P(DmctsParams)],
    "cagym_dmcts_plan": [_vp, _P(DmctsParams), _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp],
    "cagym_episode_records_init": [_vp, _int, _vp],
    "cagym_episode_records_update": [_vp, _vp, _vp, _vp, _int, _vp],
    "cagym_episode_records_restart": [_vp, _vp, _int, _vp],
    "cagym_episode_records_get": [_vp, _P(CagymEpisodeRecordPtrs)],
    "cagym_episode_log_init": [_vp, _int, _vp],
    "cagym_episode_log_update": [_vp, _vp, _vp, _vp, _int, _vp],
    "cagym_episode_log_restart": [_vp, _vp, _int, _vp],
    "cagym_episode_log_get": [_vp, _P(CagymEpisodeLogPtrs)],
    "cagym_ig_episode_log_init": [_vp, _int, _dbl, _vp],
    "cagym_ig_episode_log_update": [_vp, _vp, _vp, _vp],
    "cagym_ig_episode_log_restart": [_vp, _vp, _int, _vp],
    "cagym_ig_episode_log_get": [_vp, _P(CagymIgEpisodeLogPtrs)],
    "cagym_snapshot_layout_of": [_vp, _P(CagymSnapshotLayout)],
    "cagym_snapshot": [_vp, _vp, _int, _vp, _vp],
    "cagym_restore": [_vp, _P(CagymSnapshotLayout), _vp, _vp, _int, _vp],
    "cagym_fork": [_vp, _vp, _vp, _int, _vp],
    "cagym_stream_scenarios": [_vp, _P(CagymGen2Params), _P(C.c_int32), _vp],
    "cagym_stream_refill": [_vp, _vp],
    "cagym_stream_set_params": [_vp, _P(CagymGen2Params)],
    "cagym_stream_get": [_vp, _P(CagymStreamPtrs)],
    "cagym_stream_stop": [_vp],
    "cagym_stream_replay_init": [_vp, _int, C.c_uint64, _vp],
    "cagym_stream_replay_set": [_vp, _dbl, C.c_uint32],
    "cagym_stream_replay_push": [_vp, _vp, _int, _vp],
    "cagym_stream_replay_harvest": [_vp, _vp],
    "cagym_stream_replay_get": [_vp, _P(_vp), _P(_vp), _P(_vp), _P(_vp), _P(C.c_int)],
    "cagym_generate_exploration_scenarios": [_vp, _P(CagymExploreParams), _P(C.c_int32), _vp],
    "cagym_stream_exploration_scenarios": [_vp, _P(CagymExploreParams), _P(C.c_int32), _vp],
    "cagym_stream_set_exploration_params": [_vp, _P(CagymExploreParams)],
    "cagym_explore_stream_get": [_vp, _P(_vp), _P(_vp)],
    "cagym_step_autoreset_keep": [_vp, _vp, _OUT, _P(CagymTerminalOutputs), _vp],
    "cagym_trajectory_init": [_vp, _int, _vp],
    "cagym_trajectory_restart": [_vp, _vp, _int, _vp],
    "cagym_trajectory_get": [_vp, _P(CagymTrajectoryPtrs)],
    "cagym_checkpoint_sizes": [_vp, _P(C.c_uint64)],
    "cagym_checkpoint_save": [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp],
    "cagym_checkpoint_load": [_vp, _vp, C.c_uint64, _vp, C.c_uint64, _vp],
}
# exports of the diagnostic builds only (CAGYM_STAMPS / CAGYM_WAVETRACE / CAGYM_WGTRACE; csrc/cagym_trace.h), declared when present
_DEBUG_ARGTYPES = {"cagym_debug_stamps": [_vp, _int], "cagym_debug_wavetrace_select": [_int], "cagym_debug_wavetrace": [_vp],
                   "cagym_debug_wgtrace": [_vp, _int], "cagym_debug_xtrace": [_vp]}

_lib = None


def load():
    """Load the HIP library and declare every prototype of include/cagym.h.  torch is imported first so that the library binds to
    the HIP runtime torch already mapped (same SONAME); there is deliberately no CPU / pure-Python fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libcagym_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `python gym-exploration-2d_amd/build.py`; there is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    protos = dict(_ARGTYPES)
    protos.update((n, a) for n, a in _DEBUG_ARGTYPES.items() if hasattr(L, n))
    for name, argtypes in protos.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, _RESTYPES.get(name, C.c_int)
    _lib = L
    return L


def check(L, env, rc, what):
    if rc != 0:
        msg = L.cagym_last_error(env)
        raise RuntimeError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def call(L, env, name, *args):
    """L.<name>(env, *args); a non-zero return raises check()'s RuntimeError under that name."""
    check(L, env, getattr(L, name)(env, *args), name)


def ptr(t):
    """A tensor's device address, or None (NULL) for None."""
    return None if t is None else t.data_ptr()
