"""CPU tests of the arena's boundary: the header declares the pit entry points and the ctypes table binds each with its
argument types, the ABI number did not move (entry points were added, no argument list changed), and the arena module
stands on the library alone."""
import ast
import ctypes as C
import os
import re

from conftest import PKG, REPO

NEW = {
    "snk_engine_step_active_tape": 8,
    "snk_pit_scratch_elems": 1,
    "snk_pit_rows": 8,
    "snk_pit_moves": 7,
    "snk_pit_verdict": 10,
}


def _header():
    return open(os.path.join(REPO, "include", "snake_engine.h")).read()


def test_header_declares_the_pit_entry_points_with_the_lines_they_replace():
    txt = _header()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == n_args, name
    for cite in ("pit_mp_game_runner.py:23-35", "pit_agent.py:10-28", "pit_mp_game_runner.py:36-38", "pit_mp_game_runner.py:39-62"):
        assert cite in txt, cite
    # the entry point that was there before keeps its argument list
    m = re.search(r"\bint\s+snk_engine_step_active\s*\(([^;]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 7


def test_lib_binds_each_new_entry_point_with_argtypes():
    import snake_engine
    from snake_engine import _lib
    L = snake_engine.lib()
    for name, n_args in NEW.items():
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == n_args, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(args), name
    assert _lib.PROTOTYPES["snk_engine_step_active"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    assert L.snk_pit_scratch_elems(1) >= 4 and L.snk_pit_scratch_elems(5000) >= 2 * 5 + 2      # two columns of tile sums


def test_abi_version_is_still_113():
    import snake_engine
    from snake_engine import _lib
    assert _lib.ABI_VERSION == 113 == snake_engine.lib().snk_version()
    assert re.search(r"#define SNK_ABI_VERSION 113\b", _header())


def test_arena_stands_on_the_library_alone():
    src = open(os.path.join(PKG, "snake_engine", "arena.py")).read()
    mods = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            mods |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add("." * node.level + (node.module or ""))
    assert mods == {"collections", "numpy", "torch", "._lib", ".engine"}, mods
    assert "oracle" not in src.lower()
    import snake_engine.arena as A
    assert A.ArenaResult._fields == ("winners", "lengths", "turns", "wins_a", "wins_b", "draws")
    assert callable(A.Arena.match) and callable(A.Arena.test_pit) and callable(A.Arena.ladder_row)


def test_runner_has_run_device_beside_an_unchanged_run():
    import inspect
    from utils.pit_mp_game_runner import MPGameRunner
    assert list(inspect.signature(MPGameRunner.run_device).parameters) == ["self", "Alice", "Bob", "Alice_snake_cnt", "spawn_tape"]
    assert list(inspect.signature(MPGameRunner.run).parameters) == ["self", "Alice", "Bob", "Alice_snake_cnt", "spawn_tape"]
