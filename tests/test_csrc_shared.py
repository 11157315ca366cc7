"""The rules the query kernels share are defined once (source text only)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "optimax_rogue_amd", "csrc")

# a definition of each lifted name: a function's opens with its return type,
# its qualifiers before it at most (a call or a member's use does not match)
FUNCTION = r"^\s*(?:(?:inline|static|__host__|__device__|__forceinline__)\s+)*(?:bool|void|uint32_t|int)\s+%s\s*\("
DEFINITIONS = {
    "key_valid": FUNCTION % "key_valid",
    "wave_min": FUNCTION % "wave_min",
    "wave_sync": FUNCTION % "wave_sync",
    "grid_columns": FUNCTION % "grid_columns",
    "gather16": FUNCTION % "gather16",
    "spread4": FUNCTION % "spread4",
    "misaligned": FUNCTION % "misaligned",
    "room": FUNCTION % "room",            # the closed-form room distance
    "struct Seeker": r"^\s*struct\s+Seeker\b",
}


def sources():
    names = sorted(n for n in os.listdir(CSRC) if n.endswith((".hip", ".h")))
    assert "orx_seek.h" in names and "orx_query.h" in names and "orx_engine.hip" in names
    out = {}
    for n in names:
        with open(os.path.join(CSRC, n), encoding="utf-8") as f:
            out[n] = f.read()
    return out


def test_each_shared_rule_is_defined_in_one_file():
    src = sources()
    for name, pattern in DEFINITIONS.items():
        where = {n: len(re.findall(pattern, text, re.M)) for n, text in src.items()}
        where = {n: k for n, k in where.items() if k}
        assert sum(where.values()) == 1, (name, where)
        (home,) = where
        assert home in ("orx_seek.h", "orx_query.h"), (name, home)
    # the room distance's detour rule itself, however a copy might be named
    detour = [n for n, text in src.items() if "(ay < sy) != (ty < sy)" in text]
    assert detour == ["orx_seek.h"]


def test_nothing_is_restated():
    for n, text in sources().items():
        lines = [ln for ln in text.splitlines() if re.search(r"\brestated\b", ln, re.I)]
        if n == "orx_engine.hip":
            # its note on the reference's semantics
            assert all("reference" in ln.lower() or "semantics" in ln.lower() for ln in lines), lines
        else:
            assert lines == [], (n, lines)
