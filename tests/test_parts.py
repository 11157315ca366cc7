"""CPU: the library's parts (optimax_rogue_amd.build.PARTS) against the built
library, one case per part -- the header's exports are defined symbols and
bound, the part's id is the hash of a file list written out here, the
library's own id is that, and the part's entry of the table is pinned.  Loads
the built library; no GPU calls.
"""
import hashlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optimax_rogue_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
csrc = lambda *names: tuple(os.path.join(CSRC, n) for n in names)
include = lambda *names: tuple(os.path.join(INCLUDE, n) for n in names)

# part -> (its header, the id's symbol and macro, the files hashed in this
# order, the sources compiled)
PARTS = {
    "engine": ("orx.h", "orx_build_id", "ORX_BUILD_ID",
               csrc("orx_engine.hip") + include("orx.h") + csrc("orx_view.hip")
               + include("orx_view.h") + csrc("orx_query.h", "orx_plan.h"),
               csrc("orx_engine.hip", "orx_view.hip")),
    "path": ("orx_path.h", "orx_path_build_id", "ORX_PATH_BUILD_ID",
             csrc("orx_path.hip") + include("orx_path.h") + csrc("orx_query.h", "orx_seek.h"),
             csrc("orx_path.hip")),
    "moves": ("orx_moves.h", "orx_moves_build_id", "ORX_MOVES_BUILD_ID",
              csrc("orx_moves.hip") + include("orx_moves.h") + csrc("orx_query.h"),
              csrc("orx_moves.hip")),
    # (defined in the engine's source: nothing of its own to compile)
    "npc": ("orx_npc.h", "orx_npc_build_id", "ORX_NPC_BUILD_ID",
            include("orx_npc.h") + csrc("orx_engine.hip"), ()),
    "npc_query": ("orx_npc_query.h", "orx_npc_query_build_id", "ORX_NPC_QUERY_BUILD_ID",
                  csrc("orx_npc_query.hip") + include("orx_npc_query.h")
                  + csrc("orx_query.h", "orx_seek.h"), csrc("orx_npc_query.hip")),
    "sight": ("orx_sight.h", "orx_sight_build_id", "ORX_SIGHT_BUILD_ID",
              csrc("orx_sight.hip") + include("orx_sight.h") + csrc("orx_query.h"),
              csrc("orx_sight.hip")),
    "explore": ("orx_explore.h", "orx_explore_build_id", "ORX_EXPLORE_BUILD_ID",
                csrc("orx_explore.hip") + include("orx_explore.h")
                + csrc("orx_query.h", "orx_seek.h"), csrc("orx_explore.hip")),
    "route": ("orx_route.h", "orx_route_build_id", "ORX_ROUTE_BUILD_ID",
              csrc("orx_route.hip") + include("orx_route.h") + csrc("orx_query.h", "orx_seek.h"),
              csrc("orx_route.hip")),
}


@pytest.fixture(scope="module")
def defined(engine_lib):
    """The ``T`` symbols of the built library, and ``built_ids`` of it."""
    from optimax_rogue_amd import _lib, build
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    return set(re.findall(r" T (orx_\w+)", out)), build.built_ids(_lib.LIB_PATH)


@pytest.mark.parametrize("name", list(PARTS))
def test_part_symbols_and_build_id(engine_lib, defined, name):
    """The library exports and binds the entry points of the part's header; the
    part's id is the hash of its files, in the tree, in the loaded library and
    in a child process's reading of it (a stale library is rebuilt:
    build.build compares all ids); its table entry names what it names here."""
    from optimax_rogue_amd import _lib, build
    header, symbol, macro, files, sources = PARTS[name]
    symbols, built = defined
    exports = tuple(_lib.TABLES[header])
    if name == "engine":   # (orx_view has a header of its own and no id of its own)
        exports += tuple(_lib.TABLES["orx_view.h"])
    assert symbol in exports
    for export in exports:
        assert export in symbols and hasattr(engine_lib, export)
    h = hashlib.sha256()
    for p in files:
        with open(p, "rb") as f:
            h.update(f.read())
    ids = build.tree_ids()
    assert ids[name] == h.hexdigest()[:16] == _lib.part_id(name) == built[name]
    assert getattr(engine_lib, symbol)().decode() == ids[name]
    assert build.PARTS[name] == build.Part(symbol, macro, files, sources)
    assert all(src in build.SOURCES for src in sources)
    assert built == ids and list(built) == list(PARTS) == list(build.PARTS)
    if name == "engine":
        assert ids[name] == build.source_id() == _lib.build_id()


def test_the_compile_list_is_the_tables():
    from optimax_rogue_amd import build
    assert build.SOURCES == [src for part in PARTS.values() for src in part[4]]
    assert [os.path.basename(s) for s in build.SOURCES] == [
        "orx_engine.hip", "orx_view.hip", "orx_path.hip", "orx_moves.hip", "orx_npc_query.hip",
        "orx_sight.hip", "orx_explore.hip", "orx_route.hip"]
    assert build.SOURCES[0] == build.SRC


def test_header_tables_are_pairwise_disjoint():
    from optimax_rogue_amd import _lib
    assert set(_lib.TABLES) == {part[0] for part in PARTS.values()} | {"orx_view.h"}
    names = [n for table in _lib.TABLES.values() for n in table]
    assert len(names) == len(set(names))
    assert _lib.EXPORTS == tuple(_lib.TABLES["orx.h"])
