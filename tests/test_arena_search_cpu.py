"""CPU tests of the searching pit's boundary: the header declares snk_pit_roots and snk_pit_search_moves and the ctypes table
binds them with their argument types, the ABI number is still 113, Searcher has the signature the arena documents, and the CPU
statement the GPU test compares with (tests/search_pit_ref.py) is well-posed on its committed seeds and equals the pinned
oracle.pit_oracle.pit_run when both sides are greedy."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

NEW = {"snk_pit_roots": 9, "snk_pit_search_moves": 10}


def _header():
    return open(os.path.join(REPO, "include", "snake_engine.h")).read()


def test_header_declares_the_two_entry_points_in_the_pit_section():
    txt = _header()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == n_args, name
    pit = txt[txt.index("the pit match on the device"):txt.index("training half")]
    assert "snk_pit_roots" in pit and "snk_pit_search_moves" in pit
    assert pit.count("agent.py:25-99 behind pit_mp_game_runner.py:23-38") >= 2       # the reference lines they stand for
    # the older pit entries keep their argument lists
    for name, n_args in (("snk_pit_rows", 8), ("snk_pit_moves", 7), ("snk_pit_verdict", 10)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == n_args, name


def test_lib_binds_the_two_entry_points_with_argtypes():
    import snake_engine
    from snake_engine import _lib
    L = snake_engine.lib()
    vp, i32 = C.c_void_p, C.c_int
    want = {"snk_pit_roots": [vp, vp, i32, vp, vp, vp, vp, vp, vp],
            "snk_pit_search_moves": [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]}
    for name, args in want.items():
        assert _lib.PROTOTYPES[name] == (C.c_int, args), name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name


def test_abi_version_is_113_in_the_header_the_bindings_and_the_library():
    import snake_engine
    from snake_engine import _lib
    assert re.search(r"#define SNK_ABI_VERSION 113\b", _header())
    assert _lib.ABI_VERSION == 113
    assert snake_engine.lib().snk_version() == 113


def test_bad_arguments_are_refused_before_any_launch():
    """negative codes with a message, and n = 0 is a no-op (no device is touched: the checks come first)"""
    import snake_engine
    L = snake_engine.lib()
    assert L.snk_pit_roots(None, None, 0, None, None, None, None, None, None) < 0 and b"snk_pit_roots" in L.snk_last_error()
    assert L.snk_pit_search_moves(None, None, None, None, -1, 4, 1, 0, None, None) < 0 and b"snk_pit_search_moves" in L.snk_last_error()
    assert L.snk_pit_search_moves(None, None, None, None, 5, 9, 1, 0, None, None) < 0
    assert L.snk_pit_search_moves(None, None, None, None, 5, 4, 5, 0, None, None) < 0      # a_cnt beyond the snakes
    assert L.snk_pit_search_moves(None, None, None, None, 5, 4, 1, 0, None, None) < 0      # NULL arrays
    assert L.snk_pit_search_moves(None, None, None, None, 0, 4, 1, 0, None, None) == 0     # no game: nothing to do


def test_searcher_signature():
    from snake_engine.arena import Arena, Searcher
    sig = inspect.signature(Searcher.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("net", inspect.Parameter.empty), ("breadth", 128), ("depth", 8), ("softmax_base", 100), ("seed", None),
        ("sequential", False), ("tape_u", None), ("tt_capacity", None)]
    for name in ("search", "end_of_turn", "clear"):
        assert callable(getattr(Searcher, name))
    with pytest.raises(TypeError):
        Searcher(object())                                   # no v_device: the arena evaluates on the device only
    assert inspect.signature(Arena.test_pit).parameters["search"].default is None
    assert inspect.signature(Arena.ladder_row).parameters["search"].default is None
    assert list(inspect.signature(Arena.match).parameters) == ["self", "alice", "bob", "alice_snake_cnt", "init_tape", "spawn_tape"]


@pytest.mark.parametrize("name", list(__import__("search_pit_ref").CASES))
def test_the_committed_seeds_are_well_posed(oracle, name):
    import search_pit_ref as R
    out = R.reference(name)
    board, n, breadth, searching, seed = R.CASES[name]
    print(f"\n{name}: {out['turns']} turns, q_gap {out['q_gap']:.3e}, u_edge {out['u_edge']:.3e}, draws {out['tape_pos']}")
    R.check_well_posed(out)
    assert 4 <= n <= 6 and breadth in (8, 16)
    assert [p is not None for p in out["tape_pos"]] == list(searching) and all(p > 0 for p in out["tape_pos"] if p is not None)
    assert len(out["winners"]) == n and max(out["lengths"]) == out["turns"] == len(out["spawn_log"])


@pytest.mark.parametrize("board", ["7x7x2", "11x11x4"])
def test_greedy_v_greedy_helper_equals_the_pinned_pit_oracle(oracle, board):
    """no team searches: the helper's loop is pit_run's, draw for draw -- which pins the helper to the oracle that the recorded
    reference pits pin"""
    import search_pit_ref as R
    from oracle.obs_key import StubNet
    from oracle.pit_oracle import pit_run
    games, _ = R.start_games(board, 6)
    out = R.search_pit_run(games, (StubNet(0), StubNet(1)), (False, False), 1, 77)
    games2, _ = R.start_games(board, 6)
    rng = np.random.RandomState(77)
    log = []
    winners, lengths = pit_run(games2, StubNet(0), StubNet(1), 1, draws=lambda turn, g: (rng.random_sample(), rng.random_sample()),
                               spawn_log=log)
    assert out["winners"] == winners and out["lengths"] == lengths and out["turns"] == max(lengths) >= 3
    assert len(log) == len(out["spawn_log"]) and all(np.array_equal(a, b) for a, b in zip(log, out["spawn_log"]))
    for a, b in zip(out["games"], games2):
        ca, cb = a.compact(), b.compact()
        assert all(np.array_equal(ca[k], cb[k]) for k in R.KEYS)
    assert out["tape_pos"] == [None, None] and out["q_gap"] == np.inf and out["u_edge"] == np.inf
