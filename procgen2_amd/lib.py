"""ctypes binding of the engine's C ABI (include/procgen2_vec.h).

The shared library is the product; this module only declares prototypes.  It fails loudly when the
library has not been built — there is no Python or CPU fallback for the hot path.
"""
import collections
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_uint8, c_uint32, c_uint64, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")
DEFAULT_LIB = os.path.join(LIB_DIR, "libprocgen2_hip.so")

OBS_BYTES = 12288
OBS_SHAPE = (64, 64, 3)
NUM_ACTIONS = 15

# include/procgen2_vec.h PGV_MODE_*
MODES = {"default": 0, "easy": 1, "hard": 2, "memory": 3, "extreme": 4}


class Config(ctypes.Structure):
    """include/procgen2_vec.h `pgv_config`."""
    _fields_ = [("struct_size", c_uint32), ("num_envs", c_int32), ("game", c_char_p), ("stream", c_void_p),
                ("device", c_int32), ("seed_base", c_uint32), ("env_offset", c_int32), ("num_levels", c_int32),
                ("start_level", c_int32), ("mode", c_int32), ("game_flags", c_uint32)]


class EpisodeConfig(ctypes.Structure):
    """include/procgen2_vec.h `pgv_episode_config`."""
    _fields_ = [("struct_size", c_uint32), ("autoreset", c_int32), ("max_episode_steps", c_int32), ("final_capacity", c_int32)]


class EpisodeOutputs(ctypes.Structure):
    """include/procgen2_vec.h `pgv_episode_outputs` (device pointers)."""
    _fields_ = [("struct_size", c_uint32)] + [(name, c_void_p) for name in (
        "reward", "terminated", "truncated", "ended", "counts", "ended_env", "ended_return", "ended_length", "ended_level",
        "ended_level_known", "final_obs", "running_return", "running_length")]


class Sequence(ctypes.Structure):
    """include/procgen2_vec.h `pgv_sequence` (device pointers; host pointers for pgv_step_sequence_host)."""
    _fields_ = [("struct_size", c_uint32), ("steps", c_int32), ("actions", c_void_p), ("action_stride", c_int64),
                ("run_seed", c_uint32), ("frames", c_int32), ("rewards", c_void_p), ("dones", c_void_p),
                ("seq_return", c_void_p), ("seq_length", c_void_p), ("seq_done", c_void_p)]


class PolicyObsConfig(ctypes.Structure):
    """include/procgen2_vec.h `pgv_policy_obs_config`."""
    _fields_ = [("struct_size", c_uint32), ("stack", c_int32), ("gray", c_int32), ("dtype", c_int32), ("out", c_void_p)]


# include/procgen2_vec.h PGV_POLICY_*: name → (number, element bytes)
POLICY_DTYPES = {"uint8": (0, 1), "float16": (1, 2), "bfloat16": (2, 2), "float32": (3, 4)}


def policy_obs_enable(lib, h, stack=4, gray=True, dtype="float16", out=None):
    """pgv_policy_obs_enable.  dtype: a name of POLICY_DTYPES or the number; out: a device pointer (integer) or None for a
    tensor of the engine's own (pgv_policy_obs)."""
    number = POLICY_DTYPES[dtype][0] if dtype in POLICY_DTYPES else int(dtype)
    cfg = PolicyObsConfig(ctypes.sizeof(PolicyObsConfig), int(stack), int(gray), number, out)
    check(lib, lib.pgv_policy_obs_enable(h, ctypes.byref(cfg)), "pgv_policy_obs_enable")


class HistoryConfig(ctypes.Structure):
    """include/procgen2_vec.h `pgv_history_config`."""
    _fields_ = [("struct_size", c_uint32), ("capacity", c_int32), ("gray", c_int32), ("frames", c_void_p)]


def history_enable(lib, h, capacity, gray=False, frames=None):
    """pgv_history_enable.  frames: a device pointer (integer) or None for a ring of the engine's own (pgv_history_frames)."""
    cfg = HistoryConfig(ctypes.sizeof(HistoryConfig), int(capacity), int(gray), frames)
    check(lib, lib.pgv_history_enable(h, ctypes.byref(cfg)), "pgv_history_enable")


class TransitionsConfig(ctypes.Structure):
    """include/procgen2_vec.h `pgv_transitions_config`."""
    _fields_ = [("struct_size", c_uint32), ("reserved", c_uint32)]


class TransitionQuery(ctypes.Structure):
    """include/procgen2_vec.h `pgv_transition_query` (device pointers, each optional)."""
    _fields_ = [("struct_size", c_uint32), ("n", c_int32), ("gamma", c_float), ("stack", c_int32), ("dtype", c_int32),
                ("obs", c_void_p), ("next_obs", c_void_p), ("action", c_void_p), ("nstep_return", c_void_p), ("discount", c_void_p),
                ("steps", c_void_p), ("status", c_void_p)]


class Gae(ctypes.Structure):
    """include/procgen2_vec.h `pgv_gae` (`lam`: the header's `lambda`)."""
    _fields_ = [("struct_size", c_uint32), ("gamma", c_float), ("lam", c_float), ("values", c_void_p), ("trunc_values", c_void_p),
                ("advantages", c_void_p), ("returns", c_void_p)]


# include/procgen2_vec.h PGV_TR_*
TR_RECORDED, TR_TERMINATED, TR_TRUNCATED, TR_VOID, TR_CUT = 1, 2, 4, 8, 16


def transitions_enable(lib, h):
    """pgv_transitions_enable (after history_enable)."""
    cfg = TransitionsConfig(ctypes.sizeof(TransitionsConfig), 0)
    check(lib, lib.pgv_transitions_enable(h, ctypes.byref(cfg)), "pgv_transitions_enable")


def transition_query(n, gamma, stack, dtype, obs=None, next_obs=None, action=None, nstep_return=None, discount=None, steps=None, status=None):
    """A filled-in TransitionQuery.  dtype: a name of POLICY_DTYPES or the number; the outputs: device pointers (integers) or None."""
    number = POLICY_DTYPES[dtype][0] if dtype in POLICY_DTYPES else int(dtype)
    return TransitionQuery(ctypes.sizeof(TransitionQuery), int(n), float(gamma), int(stack), number, obs, next_obs, action, nstep_return,
                           discount, steps, status)


def gae(gamma, lam, values, advantages, trunc_values=None, returns=None):
    """A filled-in Gae of device pointers (integers)."""
    return Gae(ctypes.sizeof(Gae), float(gamma), float(lam), values, trunc_values, advantages, returns)


class StateLayoutStruct(ctypes.Structure):
    """include/procgen2_vec.h `pgv_state_layout`."""
    _fields_ = [("struct_size", c_uint32), ("width", c_int32), ("fixed", c_int32), ("record", c_int32), ("max_records", c_int32),
                ("cells", c_int32), ("tile_w", c_int32), ("tile_h", c_int32)]


StateLayout = collections.namedtuple("StateLayout", "width fixed record max_records cells tile_w tile_h fixed_names record_names")


def state_layout(lib, game, mode=None):
    """pgv_state_layout_of + pgv_state_names → StateLayout (host only: no GPU, no env).  game: a name or the id."""
    game_id = lib.pgv_game_id(game.encode()) if isinstance(game, str) else int(game)
    out = StateLayoutStruct(ctypes.sizeof(StateLayoutStruct))
    check(lib, lib.pgv_state_layout_of(game_id, mode_id(mode), ctypes.byref(out)), "pgv_state_layout_of")
    need = lib.pgv_state_names(game_id, mode_id(mode), None, 0)
    if need < 0:
        check(lib, 1, "pgv_state_names")
    buf = ctypes.create_string_buffer(need + 1)
    lib.pgv_state_names(game_id, mode_id(mode), buf, need + 1)
    fixed_names, record_names = buf.value.decode().split("|")
    return StateLayout(out.width, out.fixed, out.record, out.max_records, out.cells, out.tile_w, out.tile_h,
                       tuple(fixed_names.split()), tuple(record_names.split()))


class TilePathsStruct(ctypes.Structure):
    """include/procgen2_vec.h `pgv_tile_paths`."""
    _fields_ = [("struct_size", c_uint32), ("passable", c_uint32), ("source", c_int32), ("source_cells", c_void_p),
                ("probe", c_int32), ("probe_cells", c_void_p), ("dist", c_void_p), ("probe_dist", c_void_p),
                ("probe_step", c_void_p), ("cells_out", c_void_p)]


class PathLayoutStruct(ctypes.Structure):
    """include/procgen2_vec.h `pgv_path_layout`."""
    _fields_ = [("struct_size", c_uint32), ("cells", c_int32), ("tile_w", c_int32), ("tile_h", c_int32), ("has_goal", c_int32),
                ("agent_dx", c_float), ("agent_dy", c_float)]


PATH_POINTS = {"none": 0, "agent": 1, "goal": 2, "cells": 3}  # PGV_PATH_*
PathLayout = collections.namedtuple("PathLayout", "cells tile_w tile_h has_goal agent_dx agent_dy")


def path_layout(lib, game, mode=None):
    """pgv_path_layout_of → PathLayout (host only: no GPU, no env).  game: a name or the id."""
    game_id = lib.pgv_game_id(game.encode()) if isinstance(game, str) else int(game)
    out = PathLayoutStruct(ctypes.sizeof(PathLayoutStruct))
    check(lib, lib.pgv_path_layout_of(game_id, mode_id(mode), ctypes.byref(out)), "pgv_path_layout_of")
    return PathLayout(out.cells, out.tile_w, out.tile_h, bool(out.has_goal), out.agent_dx, out.agent_dy)


def passable_mask(passable):
    """An int as it is, or the tile ids of an iterable as bits."""
    if isinstance(passable, int):
        mask = passable
    else:
        mask = 0
        for t in passable:
            if not 0 <= int(t) < 32:
                raise ValueError("passable: tile id %r is not in 0 .. 31" % (t,))
            mask |= 1 << int(t)
    if not 0 <= mask < 2 ** 32:
        raise ValueError("passable: %r is not a 32-bit mask" % (passable,))
    return mask


class LevelLayoutStruct(ctypes.Structure):
    """include/procgen2_vec.h `pgv_level_layout`."""
    _fields_ = [("struct_size", c_uint32), ("supported", c_int32), ("cells", c_int32), ("tile_w", c_int32), ("tile_h", c_int32),
                ("backgrounds", c_int32)]


class LevelRowsStruct(ctypes.Structure):
    """include/procgen2_vec.h `pgv_level_rows` (device pointers; host pointers for the _host forms)."""
    _fields_ = [("struct_size", c_uint32), ("tiles", c_void_p), ("agent_cell", c_void_p), ("goal_cell", c_void_p),
                ("background", c_void_p), ("background_shift", c_void_p), ("ids", c_void_p), ("status", c_void_p)]


# include/procgen2_vec.h PGV_LEVEL_*: what a row's status says
LEVEL_STATUS = {"installed": 0, "no_env": 1, "bad_tile": 2, "bad_agent": 3, "bad_goal": 4, "bad_floor": 5}
LEVEL_KNOWN_CUSTOM = 2  # pgv_level_known: the caller's label
LevelLayout = collections.namedtuple("LevelLayout", "supported cells tile_w tile_h backgrounds")


def level_layout(lib, game, mode=None):
    """pgv_level_layout_of → LevelLayout (host only: no GPU, no env).  game: a name or the id."""
    game_id = lib.pgv_game_id(game.encode()) if isinstance(game, str) else int(game)
    out = LevelLayoutStruct(ctypes.sizeof(LevelLayoutStruct))
    check(lib, lib.pgv_level_layout_of(game_id, mode_id(mode), ctypes.byref(out)), "pgv_level_layout_of")
    return LevelLayout(bool(out.supported), out.cells, out.tile_w, out.tile_h, out.backgrounds)


def level_rows(tiles=None, agent_cell=None, goal_cell=None, background=None, background_shift=None, ids=None, status=None):
    """A filled-in LevelRowsStruct; the pointers are integers (data_ptr(), ctypes.data) or None."""
    return LevelRowsStruct(ctypes.sizeof(LevelRowsStruct), tiles, agent_cell, goal_cell, background, background_shift, ids, status)


class GatherAug(ctypes.Structure):
    """include/procgen2_vec.h `pgv_gather_aug`."""
    _fields_ = [("struct_size", c_uint32), ("out_height", c_int32), ("out_width", c_int32), ("pad", c_int32), ("edge", c_int32),
                ("cutout_min", c_int32), ("cutout_max", c_int32), ("cutout_color", c_int32), ("seed", c_uint32), ("params", c_void_p)]


# include/procgen2_vec.h PGV_AUG_EDGE_*, PGV_AUG_CUTOUT_*
AUG_EDGES = {"replicate": 0, "zero": 1}
AUG_CUTOUT_COLORS = {"black": 0, "random": 1}


def gather_aug(out_height, out_width, pad=0, edge="replicate", cutout_min=0, cutout_max=0, cutout_color="black", seed=0, params=None):
    """A filled-in GatherAug.  edge, cutout_color: a name or the number; params: a device pointer (integer) or None."""
    return GatherAug(ctypes.sizeof(GatherAug), int(out_height), int(out_width), int(pad), AUG_EDGES[edge] if edge in AUG_EDGES else int(edge),
                     int(cutout_min), int(cutout_max), AUG_CUTOUT_COLORS[cutout_color] if cutout_color in AUG_CUTOUT_COLORS else int(cutout_color),
                     int(seed) & 0xFFFFFFFF, params)


# include/procgen2_vec.h PGV_FRAMES_*
FRAMES = {"last": 0, "none": 1}


def sequence(steps, actions=None, action_stride=0, run_seed=0, frames="last", rewards=None, dones=None, seq_return=None,
             seq_length=None, seq_done=None):
    """A filled-in Sequence; the pointers are integers (data_ptr(), ctypes.data) or None.  frames: a name of FRAMES or the number."""
    return Sequence(ctypes.sizeof(Sequence), int(steps), actions, int(action_stride), int(run_seed) & 0xFFFFFFFF,
                    FRAMES[frames] if frames in FRAMES else int(frames), rewards, dones, seq_return, seq_length, seq_done)


# include/procgen2_vec.h PGV_AUTORESET_*
AUTORESET_MODES = {"next_step": 0, "same_step": 1}


def episodes_enable(lib, h, autoreset_mode, max_episode_steps=0, final_capacity=0):
    """pgv_episodes_enable + pgv_episode_outputs_get → EpisodeOutputs.  autoreset_mode: a name of AUTORESET_MODES or the number."""
    mode = AUTORESET_MODES[autoreset_mode] if autoreset_mode in AUTORESET_MODES else int(autoreset_mode)
    cfg = EpisodeConfig(ctypes.sizeof(EpisodeConfig), mode, int(max_episode_steps), int(final_capacity))
    check(lib, lib.pgv_episodes_enable(h, ctypes.byref(cfg)), "pgv_episodes_enable")
    out = EpisodeOutputs(ctypes.sizeof(EpisodeOutputs))
    check(lib, lib.pgv_episode_outputs_get(h, ctypes.byref(out)), "pgv_episode_outputs_get")
    return out


def mode_id(mode):
    if mode is None:
        return 0
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError("unknown distribution mode %r (one of %s)" % (mode, ", ".join(MODES)))
        return MODES[mode]
    return int(mode)


# include/procgen2_vec.h PGV_COINRUN_NO_*
COINRUN_NO_PIT, COINRUN_NO_CRATE, COINRUN_NO_DY, COINRUN_NO_MOBS = 1, 2, 4, 8
CHASER_FLOAT_ABS = JUMPER_FLOAT_ABS = 1  # include/procgen2_vec.h PGV_*_FLOAT_ABS


def make(lib, game, num_envs, device=0, seed_base=1, env_offset=0, stream=None, num_levels=0, start_level=0, mode=None,
         game_flags=0):
    """pgv_make_config → env handle (c_void_p)."""
    cfg = Config(ctypes.sizeof(Config), int(num_envs), game.encode(), stream, int(device), int(seed_base) & 0xFFFFFFFF,
                 int(env_offset), int(num_levels), int(start_level), mode_id(mode), int(game_flags))
    h = c_void_p()
    check(lib, lib.pgv_make_config(ctypes.byref(cfg), ctypes.byref(h)), "pgv_make")
    return h


_cached = {}


class EngineError(RuntimeError):
    pass


def load(path=None):
    """Load libprocgen2_hip.so (building is `python -m procgen2_amd.build` / __graft_entry__.build())."""
    path = os.path.abspath(path or os.environ.get("PROCGEN2_HIP_LIB") or DEFAULT_LIB)  # (the variable: experiment builds, tools/build_exp.py)
    if path in _cached:
        return _cached[path]
    if not os.path.exists(path):
        raise EngineError(
            "HIP engine library not found at %s — run `python -m procgen2_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback." % path)
    # One HIP runtime per process.  torch ships its own libamdhip64 under the same SONAME as /opt/rocm's, and the
    # dynamic loader hands whichever was loaded first to everyone who asks later.  The engine shares device pointers
    # and streams with torch (vec_env.py), so they must be the same runtime instance, and torch refuses to see a
    # device when it finds a foreign runtime already resident: load torch's first whenever torch is installed.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = ctypes.CDLL(path)
    P = c_void_p
    proto = {
        "pgv_game_name": (c_char_p, [c_int32]),
        "pgv_game_id": (c_int32, [c_char_p]),
        "pgv_make": (c_int32, [c_char_p, c_int32, c_int32, c_uint32, c_int32, P, POINTER(P)]),
        "pgv_make_levels": (c_int32, [c_char_p, c_int32, c_int32, c_uint32, c_int32, P, c_int32, c_int32, POINTER(P)]),
        "pgv_make_config": (c_int32, [POINTER(Config), POINTER(P)]),
        "pgv_game_modes": (c_uint32, [c_int32]),
        "pgv_mode": (c_int32, [P]),
        "pgv_close": (None, [P]),
        "pgv_reset": (c_int32, [P, P, P]),
        "pgv_step": (c_int32, [P, P]),
        "pgv_step_synthetic": (c_int32, [P, c_uint32]),
        "pgv_synthetic_action": (c_int32, [c_uint32, c_uint32, c_uint32]),
        "pgv_step_host": (c_int32, [P, P]),
        "pgv_reset_host": (c_int32, [P, P, P]),
        "pgv_decode_png": (c_int32, [c_char_p, POINTER(c_int32), POINTER(c_int32), P, ctypes.c_int64]),
        "pgv_sync": (c_int32, [P]),
        "pgv_generator_launches": (c_int64, [P]),
        "pgv_obs": (P, [P]),
        "pgv_reward": (P, [P]),
        "pgv_done": (P, [P]),
        "pgv_bind_outputs": (c_int32, [P, P, P, P]),
        "pgv_num_envs": (c_int32, [P]),
        "pgv_device": (c_int32, [P]),
        "pgv_stream": (P, [P]),
        "pgv_copy_out": (c_int32, [P, P, P, P]),
        "pgv_render_frame": (c_int32, [P, c_int32, c_int32, c_int32, P]),
        "pgv_render_frames": (c_int32, [P, P, c_int32, c_int32, c_int32, P]),
        "pgv_render_frames_host": (c_int32, [P, P, c_int32, c_int32, c_int32, P]),
        "pgv_snapshot_bytes": (c_int64, [P]),
        "pgv_save_state": (c_int32, [P, P, c_int64]),
        "pgv_load_state": (c_int32, [P, P, c_int64]),
        "pgv_env_record_bytes": (c_int64, [P]),
        "pgv_env_record_tag": (c_uint64, [P]),
        "pgv_save_envs": (c_int32, [P, P, c_int32, P]),
        "pgv_load_envs": (c_int32, [P, P, c_int32, P, c_uint64]),
        "pgv_save_envs_host": (c_int32, [P, P, c_int32, P]),
        "pgv_load_envs_host": (c_int32, [P, P, c_int32, P, c_uint64]),
        "pgv_assign_levels": (c_int32, [P, P, c_int32, P]),
        "pgv_assign_levels_host": (c_int32, [P, P, c_int32, P]),
        "pgv_level_numbers": (P, [P]),
        "pgv_level_known": (P, [P]),
        "pgv_episodes_enable": (c_int32, [P, POINTER(EpisodeConfig)]),
        "pgv_episode_outputs_get": (c_int32, [P, POINTER(EpisodeOutputs)]),
        "pgv_step_episodes": (c_int32, [P, P]),
        "pgv_step_episodes_synthetic": (c_int32, [P, c_uint32]),
        "pgv_step_episodes_host": (c_int32, [P, P]),
        "pgv_step_episodes_times": (c_int32, [P, c_int32, c_uint32, c_void_p, c_void_p]),
        "pgv_step_sequence": (c_int32, [P, POINTER(Sequence)]),
        "pgv_step_sequence_host": (c_int32, [P, POINTER(Sequence)]),
        "pgv_render_obs": (c_int32, [P, P]),
        "pgv_render_obs_host": (c_int32, [P, P]),
        "pgv_policy_obs_enable": (c_int32, [P, POINTER(PolicyObsConfig)]),
        "pgv_policy_obs": (P, [P]),
        "pgv_policy_obs_bytes_per_env": (c_int64, [P]),
        "pgv_policy_obs_restart": (P, [P]),
        "pgv_policy_obs_push": (c_int32, [P, P]),
        "pgv_policy_obs_push_host": (c_int32, [P, P]),
        "pgv_history_enable": (c_int32, [P, POINTER(HistoryConfig)]),
        "pgv_history_frames": (P, [P]),
        "pgv_history_began": (P, [P]),
        "pgv_history_pending": (P, [P]),
        "pgv_history_head": (c_int64, [P]),
        "pgv_history_capacity": (c_int32, [P]),
        "pgv_history_push": (c_int32, [P]),
        "pgv_history_gather": (c_int32, [P, P, P, c_int32, c_int32, c_int32, P]),
        "pgv_history_gather_aug": (c_int32, [P, P, P, c_int32, c_int32, c_int32, POINTER(GatherAug), P]),
        "pgv_gather_aug_params": (c_int32, [POINTER(GatherAug), c_int32, POINTER(c_int32)]),
        "pgv_transitions_enable": (c_int32, [P, POINTER(TransitionsConfig)]),
        "pgv_transitions_action": (P, [P]),
        "pgv_transitions_reward": (P, [P]),
        "pgv_transitions_flags": (P, [P]),
        "pgv_transitions_gather": (c_int32, [P, P, P, c_int32, POINTER(TransitionQuery)]),
        "pgv_transitions_gae": (c_int32, [P, c_int64, c_int32, POINTER(Gae)]),
        "pgv_step_synthetic_many": (c_int32, [P, c_int32, c_int32, c_uint32]),
        "pgv_timed_steps": (c_int32, [P, c_int32, c_uint32, POINTER(c_double), POINTER(c_double)]),
        "pgv_step_times": (c_int32, [P, c_int32, c_uint32, c_void_p, c_void_p]),
        "pgv_step_phases": (c_int32, [P, c_int32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
        "pgv_step_phases_many": (c_int32, [P, c_int32, c_int32, c_uint32, c_void_p]),
        "pgv_set_debug": (c_int32, [P, c_int32]),
        "pgv_dump_state": (c_int32, [P, c_int32, POINTER(c_float), c_int32]),
        "pgv_dump_tiles": (c_int32, [P, c_int32, POINTER(c_uint8), c_int32]),
        "pgv_state_layout_of": (c_int32, [c_int32, c_int32, POINTER(StateLayoutStruct)]),
        "pgv_state_names": (c_int64, [c_int32, c_int32, c_char_p, c_int64]),
        "pgv_state_rows": (c_int32, [P, P, c_int32, P, P]),
        "pgv_tile_rows": (c_int32, [P, P, c_int32, P]),
        "pgv_state_rows_host": (c_int32, [P, P, c_int32, P, P]),
        "pgv_tile_rows_host": (c_int32, [P, P, c_int32, P]),
        "pgv_tile_paths_rows": (c_int32, [P, P, c_int32, POINTER(TilePathsStruct)]),
        "pgv_tile_paths_rows_host": (c_int32, [P, P, c_int32, POINTER(TilePathsStruct)]),
        "pgv_path_layout_of": (c_int32, [c_int32, c_int32, POINTER(PathLayoutStruct)]),
        "pgv_level_layout_of": (c_int32, [c_int32, c_int32, POINTER(LevelLayoutStruct)]),
        "pgv_get_levels": (c_int32, [P, P, c_int32, POINTER(LevelRowsStruct)]),
        "pgv_set_levels": (c_int32, [P, P, c_int32, POINTER(LevelRowsStruct)]),
        "pgv_get_levels_host": (c_int32, [P, P, c_int32, POINTER(LevelRowsStruct)]),
        "pgv_set_levels_host": (c_int32, [P, P, c_int32, POINTER(LevelRowsStruct)]),
        "pgv_last_error": (c_char_p, []),
    }
    for name, (res, args) in proto.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _cached[path] = lib
    return lib


def check(lib, rc, what):
    if rc != 0:
        msg = lib.pgv_last_error()
        raise EngineError("%s failed: %s" % (what, msg.decode() if msg else "unknown error"))


EXPORTED_VEC_SYMBOLS = [
    "pgv_game_name", "pgv_game_id", "pgv_make", "pgv_make_levels", "pgv_make_config", "pgv_game_modes", "pgv_mode", "pgv_close", "pgv_reset", "pgv_step", "pgv_step_synthetic", "pgv_step_synthetic_many",
    "pgv_synthetic_action", "pgv_step_host", "pgv_reset_host", "pgv_decode_png", "pgv_sync", "pgv_generator_launches", "pgv_obs", "pgv_reward", "pgv_done", "pgv_bind_outputs", "pgv_num_envs",
    "pgv_device", "pgv_stream", "pgv_copy_out", "pgv_render_frame", "pgv_render_frames", "pgv_render_frames_host", "pgv_snapshot_bytes", "pgv_save_state", "pgv_load_state",
    "pgv_env_record_bytes", "pgv_env_record_tag", "pgv_save_envs", "pgv_load_envs", "pgv_save_envs_host", "pgv_load_envs_host",
    "pgv_assign_levels", "pgv_assign_levels_host", "pgv_level_numbers", "pgv_level_known",
    "pgv_episodes_enable", "pgv_episode_outputs_get", "pgv_step_episodes", "pgv_step_episodes_synthetic", "pgv_step_episodes_host", "pgv_step_episodes_times",
    "pgv_step_sequence", "pgv_step_sequence_host", "pgv_render_obs", "pgv_render_obs_host",
    "pgv_policy_obs_enable", "pgv_policy_obs", "pgv_policy_obs_bytes_per_env", "pgv_policy_obs_restart", "pgv_policy_obs_push", "pgv_policy_obs_push_host",
    "pgv_history_enable", "pgv_history_frames", "pgv_history_began", "pgv_history_pending", "pgv_history_head", "pgv_history_capacity", "pgv_history_push",
    "pgv_history_gather", "pgv_history_gather_aug", "pgv_gather_aug_params",
    "pgv_transitions_enable", "pgv_transitions_action", "pgv_transitions_reward", "pgv_transitions_flags", "pgv_transitions_gather", "pgv_transitions_gae",
    "pgv_timed_steps", "pgv_step_times", "pgv_step_phases", "pgv_step_phases_many", "pgv_set_debug", "pgv_dump_state", "pgv_dump_tiles",
    "pgv_state_layout_of", "pgv_state_names", "pgv_state_rows", "pgv_tile_rows", "pgv_state_rows_host", "pgv_tile_rows_host",
    "pgv_tile_paths_rows", "pgv_tile_paths_rows_host", "pgv_path_layout_of",
    "pgv_level_layout_of", "pgv_get_levels", "pgv_set_levels", "pgv_get_levels_host", "pgv_set_levels_host",
    "pgv_last_error",
]
EXPORTED_CENV_SYMBOLS = [
    "make_data", "reset_data", "step_data", "render_data", "cenv_get_env_version", "cenv_make", "cenv_reset",
    "cenv_step", "cenv_render", "cenv_close",
]
