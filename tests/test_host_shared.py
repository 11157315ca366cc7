"""The rules the queries' host side shares are written once (source text only)."""
import ast
import os
import re

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "optimax_rogue_amd")
PART_NAMES = ("engine", "path", "moves", "npc", "npc_query", "sight", "explore", "route")


def modules():
    names = sorted(n for n in os.listdir(PKG) if n.endswith(".py"))
    assert {"path.py", "npc_query.py", "explore.py", "route.py", "query.py", "view.py",
            "engine.py", "engine_queries.py", "build.py", "_lib.py"} <= set(names)
    out = {}
    for n in names:
        with open(os.path.join(PKG, n), encoding="utf-8") as f:
            out[n] = f.read()
    return out


def test_the_seek_core_is_defined_once():
    src = modules()
    for name in ("between", "is_stair", "first_move", "bank_of"):
        where = {n: len(re.findall(rf"^\s*def {name}\(", text, re.M)) for n, text in src.items()}
        where = {n: k for n, k in where.items() if k}
        assert sum(where.values()) == 1, (name, where)
        assert set(where) <= {"path.py", "query.py"}, (name, where)


def test_a_bank_is_made_from_a_configuration_in_two_places():
    found = []
    for n, text in modules().items():
        tree = ast.parse(text)
        for fn in ast.walk(tree):
            if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
                own = [c for c in ast.walk(fn) if isinstance(c, ast.Call)
                       and ast.unparse(c) == "DungeonBank(cfg.layouts)"]
                found += [(n, fn.name)] * len(own)
        assert text.count("DungeonBank(cfg.layouts)") == sum(1 for m, _ in found if m == n), n
    assert sorted(found) == [("engine.py", "__init__"), ("query.py", "bank_of")]


def test_no_part_has_a_wrapper_of_its_own():
    pattern = rf"^\s*def (?:{'|'.join(PART_NAMES)})_(?:build_)?id\("
    for n, text in modules().items():
        assert re.findall(pattern, text, re.M) == [], n
