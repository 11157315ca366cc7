"""Builds the HIP engine in-tree: optimax_rogue_amd/liborx.so for gfx950.

    python -m optimax_rogue_amd.build [--force]

Diagnostic variants (results wrong by design; used by tools/ab_*.py and
tools/stamps.py to attribute time) are built by the same recipe with extra
preprocessor definitions, into tools/ab_libs/ by default:

    python -m optimax_rogue_amd.build --variant diag16     # -DORX_DIAG=16: no trajectory stores
    python -m optimax_rogue_amd.build --variant diag32     # -DORX_DIAG=32: trajectory stores only
    python -m optimax_rogue_amd.build --variant stamps     # -DORX_STAMPS: s_memtime timeline
    python -m optimax_rogue_amd.build --define ORX_STREAM_AUX=0 --out /tmp/x.so

The definitions are folded into the library's build id (``orx_build_id()``
= ``source_id(defines)``), so a diagnostic library can never pass for the
product build (tests/test_gpu_parity.py::test_loaded_library_is_the_trees_kernel).
"""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
from collections import namedtuple
from pathlib import Path
from typing import Iterable, Optional

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
SRC = os.path.join(PKG_DIR, "csrc", "orx_engine.hip")
HDR = os.path.join(ROOT, "include", "orx.h")
# the queries, one more object of the library each: the egocentric map view
# (orx_view), the staircase distance field (orx_path_*), what each move would
# do (orx_moves), and what the three share (internal, hashed into every id)
VIEW_SRC = os.path.join(PKG_DIR, "csrc", "orx_view.hip")
VIEW_HDR = os.path.join(ROOT, "include", "orx_view.h")
PATH_SRC = os.path.join(PKG_DIR, "csrc", "orx_path.hip")
PATH_HDR = os.path.join(ROOT, "include", "orx_path.h")
MOVES_SRC = os.path.join(PKG_DIR, "csrc", "orx_moves.hip")
MOVES_HDR = os.path.join(ROOT, "include", "orx_moves.h")
QUERY_HDR = os.path.join(PKG_DIR, "csrc", "orx_query.h")
# the seek-shaped rules that path, npc_query, explore and route share (internal)
SEEK_HDR = os.path.join(PKG_DIR, "csrc", "orx_seek.h")
PLAN_HDR = os.path.join(PKG_DIR, "csrc", "orx_plan.h")   # the engine's launch plan (host side)
# the tick with the NPCs' moves from the caller (orx_npc_*): defined in the
# engine's source (it needs the moving-NPC tick), declared in a header of its own
NPC_HDR = os.path.join(ROOT, "include", "orx_npc.h")
# the enemies' queries (orx_npc_options / orx_npc_seek): one more object
NPC_QUERY_SRC = os.path.join(PKG_DIR, "csrc", "orx_npc_query.hip")
NPC_QUERY_HDR = os.path.join(ROOT, "include", "orx_npc_query.h")
# line of sight through the walls of orx_view's window (orx_sight): one more object
SIGHT_SRC = os.path.join(PKG_DIR, "csrc", "orx_sight.hip")
SIGHT_HDR = os.path.join(ROOT, "include", "orx_sight.h")
# the map a player remembers and the way to its edge (orx_explore_*): one more object
EXPLORE_SRC = os.path.join(PKG_DIR, "csrc", "orx_explore.hip")
EXPLORE_HDR = os.path.join(ROOT, "include", "orx_explore.h")
# walking distances over the remembered map (orx_route*): one more object
ROUTE_SRC = os.path.join(PKG_DIR, "csrc", "orx_route.hip")
ROUTE_HDR = os.path.join(ROOT, "include", "orx_route.h")
OUT = os.path.join(PKG_DIR, "liborx.so")
ARCH = os.environ.get("ORX_OFFLOAD_ARCH", "gfx950")
AB_LIBS = os.path.join(ROOT, "tools", "ab_libs")

# named diagnostic variants: their -D sets
VARIANTS = {
    "diag16": ("ORX_DIAG=16",),   # rollout without its trajectory stores
    "diag32": ("ORX_DIAG=32",),   # the trajectory stores alone (no tick runs)
    "stamps": ("ORX_STAMPS",),    # per-wave s_memtime stamps + rare-block counts
    "diag64": ("ORX_DIAG=64",),   # the paired RandomBot tick block without Philox
    "noremap": ("ORX_XCD_REMAP=0",),  # workgroups in dispatch order (no XCD-aware remap)
    "envw5": ("ORX_ENV_WAVES=5",),    # orx_env_step_ex held to 5 waves per SIMD
    "envw6": ("ORX_ENV_WAVES=6",),    # ... to 6
    "envd1": ("ORX_ENV_DIAG=1",),     # orx_env_step without its tick (outputs of the loaded state)
    "envd2": ("ORX_ENV_DIAG=2",),     # orx_env_step without its observation rows
}


# The library's parts, each with a build id of its own: the C function that
# returns it, the -D macro that carries it into the build, the files it hashes
# (in this order), the sources compiled.  Ids, flags and compile list come from here.
Part = namedtuple("Part", "symbol macro files sources")
PARTS = {
    "engine": Part("orx_build_id", "ORX_BUILD_ID", (SRC, HDR, VIEW_SRC, VIEW_HDR, QUERY_HDR,
                                                     PLAN_HDR), (SRC, VIEW_SRC)),
    "path": Part("orx_path_build_id", "ORX_PATH_BUILD_ID", (PATH_SRC, PATH_HDR, QUERY_HDR,
                                                               SEEK_HDR), (PATH_SRC,)),
    "moves": Part("orx_moves_build_id", "ORX_MOVES_BUILD_ID", (MOVES_SRC, MOVES_HDR, QUERY_HDR),
                  (MOVES_SRC,)),
    "npc": Part("orx_npc_build_id", "ORX_NPC_BUILD_ID", (NPC_HDR, SRC), ()),   # (in SRC)
    "npc_query": Part("orx_npc_query_build_id", "ORX_NPC_QUERY_BUILD_ID",
                      (NPC_QUERY_SRC, NPC_QUERY_HDR, QUERY_HDR, SEEK_HDR), (NPC_QUERY_SRC,)),
    "sight": Part("orx_sight_build_id", "ORX_SIGHT_BUILD_ID", (SIGHT_SRC, SIGHT_HDR, QUERY_HDR),
                  (SIGHT_SRC,)),
    "explore": Part("orx_explore_build_id", "ORX_EXPLORE_BUILD_ID",
                    (EXPLORE_SRC, EXPLORE_HDR, QUERY_HDR, SEEK_HDR), (EXPLORE_SRC,)),
    "route": Part("orx_route_build_id", "ORX_ROUTE_BUILD_ID", (ROUTE_SRC, ROUTE_HDR, QUERY_HDR,
                                                                  SEEK_HDR), (ROUTE_SRC,)),
}
# (SRC first: _build_parts splits it)
SOURCES = [src for p in PARTS.values() for src in p.sources]


def hipcc() -> str:
    for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"), "hipcc"):
        if os.path.sep not in c or os.path.exists(c):
            return c
    return "hipcc"


def tree_ids(defines: Iterable[str] = ()) -> dict:
    """The ids of a library built from this tree, by part name: the first 16
    hex digits of SHA-256 over the part's files, and for the engine of a build
    with extra definitions ``+`` and their sorted list (its own id, then)."""
    ids = {name: hashlib.sha256(b"".join(Path(p).read_bytes() for p in part.files)).hexdigest()[:16]
           for name, part in PARTS.items()}
    d = sorted(defines)
    ids["engine"] += "+" + ",".join(d) if d else ""
    return ids


def source_id(defines: Iterable[str] = ()) -> str:
    """What orx_build_id() of a library built from these sources returns."""
    return tree_ids(defines)["engine"]


def built_ids(path: str = OUT):
    """``tree_ids``'s dict for the library at `path` ("" for a part it was built
    without; None if it cannot be loaded), read in one child process so this
    one does not map a library that a later build replaces."""
    code = ("import ctypes,sys; L=ctypes.CDLL(sys.argv[1])\n"
            "for f in (getattr(L,s,None) for s in sys.argv[2:]):\n"
            "    f and setattr(f,'restype',ctypes.c_char_p); print(f().decode() if f else '')")
    cmd = [sys.executable, "-c", code, path] + [p.symbol for p in PARTS.values()]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
    except (OSError, subprocess.SubprocessError):
        return None
    lines = out.stdout.split("\n")
    if out.returncode != 0 or len(lines) <= len(PARTS):
        return None
    return {name: line.strip() for name, line in zip(PARTS, lines)}


def _fresh(out: str, ids: dict) -> bool:
    return os.path.exists(out) and built_ids(out) == ids


def build(force: bool = False, verbose: bool = False, defines: Iterable[str] = (),
          out: Optional[str] = None) -> str:
    defines = tuple(defines)
    out = out or (OUT if not defines else os.path.join(AB_LIBS, "custom.so"))
    ids = tree_ids(defines)
    if not force and _fresh(out, ids):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # one build per output at a time (parallel test workers in a fresh tree):
    # the others wait on the lock and then find the library built
    import fcntl
    with open(out + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and _fresh(out, ids):
            return out
        return _build_locked(out, ids, defines, verbose)


def _build_locked(out: str, ids: dict, defines, verbose: bool) -> str:
    base = [hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall"] \
        + [f'-D{p.macro}="{ids[name]}"' for name, p in PARTS.items()] \
        + [f"-D{d}" for d in defines]
    if any(d.split("=")[0] == "ORX_STAMPS" for d in defines):
        # one translation unit (the stamps buffer is a device global read back
        # by the host side, so every kernel must live in the host's unit)
        cmd = base + ["-shared", "-o", out + ".tmp"] + SOURCES
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    else:
        _build_parts(base, out + ".tmp", verbose)
    os.replace(out + ".tmp", out)
    return out


# The split build: orx_engine.hip compiled NPARTS times in parallel (part 0:
# the host side, every kernel instance declared extern; parts 1..NPARTS-1:
# their share of the explicit instantiations, orx_engine.hip "Kernel
# instances"), then linked -- about a minute on 8 cores instead of ~6 for one
# translation unit.  The other SOURCES (orx_view.hip, orx_path.hip,
# orx_moves.hip, orx_npc_query.hip, orx_sight.hip, orx_explore.hip and orx_route.hip: small)
# are one more object each, compiled last.
NPARTS = 17


def _build_parts(base, out, verbose=False, jobs=None):
    import tempfile
    jobs = jobs or max(1, min(NPARTS, int(os.environ.get("MAX_JOBS", 0)) or os.cpu_count() or 1))
    with tempfile.TemporaryDirectory(prefix="orx_build_") as tmp:
        objs = [os.path.join(tmp, f"part{k}.o") for k in range(NPARTS)]
        cmds = [base + ["-c", f"-DORX_NPARTS={NPARTS}", f"-DORX_PART={k}", "-o", objs[k], SRC]
                for k in range(NPARTS)]
        for src in SOURCES[1:]:
            objs.append(os.path.join(tmp, os.path.basename(src)[:-len(".hip")] + ".o"))
            cmds.append(base + ["-c", "-o", objs[-1], src])
        if verbose:
            print(" ".join(cmds[0]) + f"  (parts 0..{NPARTS - 1}, {jobs} at a time)")
        # the heaviest parts first (the paired and one-lane rollouts)
        order = list(range(1, NPARTS)) + [0] + list(range(NPARTS, len(cmds)))
        running, failed = [], []
        while order or running:
            while order and len(running) < jobs:
                k = order.pop(0)
                running.append((k, subprocess.Popen(cmds[k])))
            k, p = running.pop(0)
            if p.wait() != 0:
                failed.append(k)
        if failed:
            raise subprocess.CalledProcessError(1, f"hipcc part(s) {failed}")
        link = [hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", out] + objs
        if verbose:
            print(" ".join(link))
        subprocess.check_call(link)


def build_variant(name: str, force: bool = False, verbose: bool = False) -> str:
    """tools/ab_libs/<name>.so for a named diagnostic variant (VARIANTS)."""
    return build(force, verbose, VARIANTS[name], os.path.join(AB_LIBS, name + ".so"))


def main(argv):
    force = "--force" in argv
    defines, out, variants = [], None, []
    it = iter(argv)
    for a in it:
        if a == "--define":
            defines.append(next(it))
        elif a == "--out":
            out = os.path.abspath(next(it))
        elif a == "--variant":
            variants.append(next(it))
    if len(variants) > 1 and out:
        raise SystemExit("--out names one library: give one --variant with it")
    for v in variants:   # --variant NAME [--out PATH]: that variant (plus any --define)
        print(build(force, True, VARIANTS[v] + tuple(defines),
                    out or os.path.join(AB_LIBS, v + ".so")))
    if not variants:
        print(build(force, verbose=True, defines=defines, out=out))


if __name__ == "__main__":
    main(sys.argv[1:])
