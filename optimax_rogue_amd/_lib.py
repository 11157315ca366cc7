"""ctypes loader for liborx.so (the HIP engine, C-ABI in include/orx.h).

There is no fallback: if the library is missing or cannot be loaded, every
engine call raises.  Build it with ``python -m optimax_rogue_amd.build`` (or
``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes
import os

from .config import OrxCfg

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "liborx.so")
ABI_VERSION = 7


class OrxState(ctypes.Structure):
    """ctypes mirror of orx_state_t (device pointers)."""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "p_x", "p_y", "p_depth", "p_health", "st_x", "st_y", "tick", "status", "episode",
        "ret_sum", "ep_count", "counters", "npc_pos", "npc_health", "npc_alive",
        "p_layout", "bank_tiles", "bank_ground", "bank_meta", "sep_start", "mt_py", "mt_np",
        "dstore", "p_rpg", "item_pos", "item_mask", "npc_grid")]


class OrxRolloutShape(ctypes.Structure):
    """ctypes mirror of orx_rollout_shape_t."""
    _fields_ = [(n, ctypes.c_int32) for n in ("games_per_wave", "lanes_per_game", "nontemporal",
                                                "threads_per_block", "lds_bytes")]


class OrxEnvStepArgs(ctypes.Structure):
    """ctypes mirror of orx_env_step_args_t (orx_env_step_ex's arguments in
    one block: VecEnv.step updates a prebuilt block and passes one pointer)."""
    _fields_ = [("cfg", ctypes.POINTER(OrxCfg)), ("st", ctypes.POINTER(OrxState)),
                ("actions", ctypes.c_void_p), ("action_bytes", ctypes.c_int32),
                ("action_cols", ctypes.c_int32), ("policy_p2", ctypes.c_int32),
                ("pad0", ctypes.c_int32), ("act", ctypes.c_void_p), ("obs", ctypes.c_void_p),
                ("reward", ctypes.c_void_p), ("done", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("bad_actions", ctypes.c_void_p),
                ("n_games", ctypes.c_int64), ("seed", ctypes.c_uint64),
                ("game_offset", ctypes.c_int64), ("stream", ctypes.c_void_p)]


class OrxError(RuntimeError):
    def __init__(self, fn: str, code: int, msg: str):
        super().__init__(f"{fn} returned {code}: {msg}")
        self.code = code


_lib = None

vp, i64, i32, u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64
_int, _str = ctypes.c_int, ctypes.c_char_p
_cfg, _st = ctypes.POINTER(OrxCfg), ctypes.POINTER(OrxState)

# header -> name -> (restype, argtypes).  include/orx.h: what every library
# has, then what is bound only when present (an A/B diagnostic may load an
# older build); the other headers' symbols are optional too.
_REQUIRED = {
    "orx_abi_version": (_int, []),
    "orx_last_error": (_str, []),
    "orx_validate_cfg": (_int, [_cfg]),
    "orx_reset": (_int, [_cfg, _st, vp, i64, u64, i64, vp]),
    "orx_step": (_int, [_cfg, _st, vp, i64, u64, i64, vp]),
    "orx_step_events": (_int, [_cfg, _st, vp, vp, vp, i64, u64, i64, vp]),
    "orx_policy": (_int, [_cfg, _st, i32, i32, vp, i64, u64, i64, vp]),
    "orx_rollout": (_int, [_cfg, _st, i32, i32, i32, vp, vp, i64, u64, i64, vp]),
    "orx_dungeon_stairs": (_int, [_cfg, vp, vp, vp, vp, vp, vp, i64, u64, vp]),
    "orx_dungeon_spawn": (_int, [_cfg, _st, vp, vp, vp, vp, vp, vp, vp, i64, u64, vp]),
    "orx_seed_mt": (_int, [_cfg, _st, i64, u64, i64, vp]),
    "orx_build_id": (_str, []),
    "orx_rollout_lanes": (_int, [i64]),
}
TABLES = {
    "orx.h": {
        **_REQUIRED,
        "orx_dstore_depths": (_int, [_cfg]),
        "orx_rollout_shape": (_int, [_cfg, i32, i32, i64, i32, i32,
                                     ctypes.POINTER(OrxRolloutShape)]),
        "orx_rollout_concurrent": (_int, [_cfg, _st, i32, i32, i32, vp, vp, i64, u64, i64, i32,
                                          vp]),
        "orx_env_step": (_int, [_cfg, _st, vp, i32, i32, i32, vp, vp, vp, vp, vp, i64, u64, i64,
                                vp]),
        "orx_rollout_ex": (_int, [_cfg, _st, i32, i32, i32, vp, vp, i32, i64, u64, i64, i32, vp]),
        "orx_env_step_ex": (_int, [_cfg, _st, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64, u64,
                                   i64, vp]),
        "orx_step_n": (_int, [_cfg, _st, vp, i32, vp, i32, i64, u64, i64, vp]),
        "orx_max_events": (_int, [_cfg]),
        "orx_step_n_ex": (_int, [_cfg, _st, vp, i32, vp, i32, i64, u64, i64, i32, vp]),
        "orx_env_step_args": (_int, [ctypes.POINTER(OrxEnvStepArgs)]),
    },
    "orx_view.h": {"orx_view": (_int, [_cfg, _st, i32, i32, vp, vp, i64, vp])},
    "orx_path.h": {
        "orx_path_field": (_int, [_cfg, vp, vp, vp]),
        "orx_path_query": (_int, [_cfg, _st, vp, i32, i32, vp, vp, vp, i64, vp]),
        "orx_path_build_id": (_str, []),
        "orx_path_rows": (_int, [_cfg, vp, vp, vp, vp, i64, vp]),
        "orx_path_seek": (_int, [_cfg, _st, vp, i32, vp, vp, vp, i64, vp]),
        "orx_path_threat": (_int, [_cfg, _st, vp, i32, i32, vp, vp, vp, vp, vp, i64, vp]),
        "orx_path_ticks": (_int, [_cfg, _st, vp, i32, i32, vp, vp, vp, i64, vp]),
    },
    "orx_moves.h": {
        "orx_moves": (_int, [_cfg, _st, i32, vp, vp, vp, i64, vp]),
        "orx_moves_build_id": (_str, []),
    },
    "orx_npc.h": {
        "orx_npc_max_events": (_int, [_cfg]),
        "orx_npc_step": (_int, [_cfg, _st, vp, vp, i64, u64, i64, vp]),
        "orx_npc_step_events": (_int, [_cfg, _st, vp, vp, vp, vp, i64, u64, i64, vp]),
        "orx_npc_step_n": (_int, [_cfg, _st, vp, vp, i32, vp, i32, i64, u64, i64, i32, vp]),
        "orx_npc_env_step": (_int, [ctypes.POINTER(OrxEnvStepArgs), vp]),
        "orx_npc_build_id": (_str, []),
    },
    "orx_npc_query.h": {
        "orx_npc_options": (_int, [_cfg, _st, vp, vp, vp, vp, i64, vp]),
        "orx_npc_seek": (_int, [_cfg, _st, vp, vp, vp, vp, i64, vp]),
        "orx_npc_query_build_id": (_str, []),
    },
    "orx_sight.h": {
        "orx_sight": (_int, [_cfg, _st, i32, i32, vp, vp, vp, i64, vp]),
        "orx_sight_build_id": (_str, []),
    },
    "orx_explore.h": {
        "orx_explore_update": (_int, [_cfg, _st, i32, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
        "orx_explore_seek": (_int, [_cfg, _st, vp, i32, vp, vp, vp, vp, vp, i64, vp]),
        "orx_explore_build_id": (_str, []),
    },
    "orx_route.h": {
        "orx_route_planes": (_int, [_cfg, vp, vp, vp]),
        "orx_route": (_int, [_cfg, _st, vp, i32, vp, vp, vp, vp, vp, vp, i64, vp]),
        "orx_route_build_id": (_str, []),
    },
}
EXPORTS = tuple(TABLES["orx.h"])
(VIEW_EXPORTS, PATH_EXPORTS, MOVES_EXPORTS, NPC_EXPORTS, NPC_QUERY_EXPORTS, SIGHT_EXPORTS,
 EXPLORE_EXPORTS, ROUTE_EXPORTS) = (tuple(t) for h, t in TABLES.items() if h != "orx.h")


def load() -> ctypes.CDLL:
    """Loads liborx.so once.  torch is imported first so the library binds to the
    HIP runtime (libamdhip64.so.7) already mapped by PyTorch-ROCm."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (HIP runtime first)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"HIP engine library missing: {LIB_PATH} -- run "
                           "`python -m optimax_rogue_amd.build` first")
    L = ctypes.CDLL(LIB_PATH)
    for table in TABLES.values():
        for name, (restype, argtypes) in table.items():
            if name in _REQUIRED or hasattr(L, name):   # (a missing required symbol raises)
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
    v = L.orx_abi_version()
    if v != ABI_VERSION:
        raise RuntimeError(f"liborx.so ABI {v} != expected {ABI_VERSION}")
    _lib = L
    return L


def check(fn: str, code: int) -> None:
    if code != 0:
        msg = load().orx_last_error().decode(errors="replace")
        raise OrxError(fn, code, msg)


def build_id() -> str:
    """orx_build_id() of the loaded library (build.source_id() of its sources)."""
    return load().orx_build_id().decode()


def part_id(name: str) -> str:
    """The id of part ``name`` (build.PARTS) in the loaded library, which is
    build.tree_ids()[name] of its sources; "" for a library built without it."""
    from .build import PARTS
    fn = getattr(load(), PARTS[name].symbol, None)
    return fn().decode() if fn is not None else ""
