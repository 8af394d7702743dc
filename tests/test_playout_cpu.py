"""CPU tests of the playout opponent: the library's surface (the three entry points bound with the stated signatures, the host-only
size functions), the Python layer's refusals (no GPU: nothing is launched), the properties of the statement itself
(tests/playout_ref.py) on hand-built boards, and a strength reading of the statement against the plain script.

Cells are (y, x); heading 0 = y-1, 1 = x+1, 2 = y+1, 3 = x-1; move 0 turns left, 1 goes straight, 2 turns right."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import look_ref as K
import playout_ref as M
import script_ref as R

HD = 1


def play(st, s, P=2, T=6, eps=0, seed=0, g=0, flags=R.ALL, H=7):
    return M.playout_scores(H, H, len(st["alive"]), HD, st, g, s, P, T, eps, seed, flags)


# ---- the library's surface and the Python layer (nothing is launched) ---------------------------------------------------------------
def test_the_entry_points_are_exported_with_their_prototypes():
    """The header, the bindings and the library agree on the ABI number.  The number itself stays 113: the three entry points are
    added and no older argument list changed -- the rule by which the lookahead's and the deep opponent's were added under 113 --
    and thirteen tests of the suite pin 113"""
    import snake_engine
    from snake_engine import _lib
    L = snake_engine.lib()
    i32, vp = C.c_int, C.c_void_p
    want = {"snk_pit_playout_clones": (i32, [i32]),
            "snk_pit_playout_scratch_elems": (C.c_long, [i32, i32, i32]),
            "snk_pit_playout_values": (i32, [vp, vp, vp, i32, C.c_uint32, i32, i32, i32, C.c_uint64, vp, vp, vp])}
    for name, (res, args) in want.items():
        assert hasattr(L, name)
        assert _lib.PROTOTYPES[name] == (res, args) and getattr(L, name).argtypes == args and getattr(L, name).restype == res
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "snake_engine.h")).read()
    number = int(re.search(r"#define SNK_ABI_VERSION (\d+)", header).group(1))
    assert number == _lib.ABI_VERSION == L.snk_version()
    comment = header[header.index("#define SNK_ABI_VERSION"):header.index("int snk_version(void);")]
    for name in want:
        assert name in comment, f"{name} is missing from the list of what was added under {number}"
        assert re.search(rf"\b{name}\(const snk_engine \*e, snk_engine \*sub, const int32_t \*d_pairs, int m, uint32_t flags, int P, "
                         rf"int T, int eps,\s+uint64_t seed, int32_t \*d_scratch, float \*d_q, void \*stream\);", header) \
            if name.endswith("values") else re.search(rf"\b{name}\(int ", header)


def test_the_size_functions():
    import snake_engine
    L = snake_engine.lib()
    assert [L.snk_pit_playout_clones(P) for P in (1, 2, 8, 64)] == [3, 6, 24, 192]
    assert [L.snk_pit_playout_clones(P) for P in (0, -1, 65, 1 << 30, -(1 << 31))] == [-1] * 5
    assert L.snk_pit_playout_scratch_elems(-1, 4, 8) == -1
    assert [L.snk_pit_playout_scratch_elems(8, S, 8) for S in (1, 9, 0, -2)] == [-1] * 4
    assert [L.snk_pit_playout_scratch_elems(8, 4, P) for P in (0, 65, -1)] == [-1] * 3
    for S, P in ((2, 1), (4, 8), (8, 64)):
        edge = (1 << 28) // (3 * P * S)
        assert L.snk_pit_playout_scratch_elems(edge, S, P) > 0 and L.snk_pit_playout_scratch_elems(edge + 1, S, P) == -1
        sizes = [L.snk_pit_playout_scratch_elems(m, S, P) for m in (0, 1, 2, 100, 1000)]
        assert sizes == sorted(sizes) and sizes[0] >= 0
        n = 100 * 3 * P
        # int32 elements: per row its three plain scores; per clone a source slot, a fate and S + 1 bytes; per (clone, snake) a pair
        # and three scores
        assert sizes[3] >= 3 * 100 + 2 * n + n * (S + 1) // 4 + n * S * (2 + 3)
        assert sizes[3] <= 3 * 100 + 2 * n + n * (S + 1) // 4 + n * S * (2 + 3) + 64


def test_playout_is_a_scripted_with_its_refusals():
    from snake_engine import arena
    from snake_engine.arena import Arena, Playout, Scripted, Searcher
    s = Playout()
    assert isinstance(s, Scripted) and not hasattr(s, "v_device")
    assert (s.flags, s.playouts, s.horizon, s.explore, s.seed) == (7, 8, 8, 64, 0)
    t = Playout(5, 64, 1, 256, (1 << 64) - 1)
    assert (t.flags, t.playouts, t.horizon, t.explore, t.seed) == (5, 64, 1, 256, (1 << 64) - 1)
    assert Playout(0, playouts=1, horizon=64, explore=0).flags == 0
    for bad in (dict(flags=8), dict(playouts=0), dict(playouts=65), dict(horizon=0), dict(horizon=65), dict(explore=-1),
                dict(explore=257), dict(seed=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            Playout(**bad)
    with pytest.raises(TypeError):
        Searcher(s)
    net = type("Net", (), {"v_device": lambda self, planes, mask: None})()
    a, b = Arena._sides(s, net, dict(breadth=8, depth=4), 3)
    assert a is s and isinstance(b, Searcher)
    assert arena.PLAYOUT_SLOT_BUDGET == 1 << 18 and "not tuned" in Playout.__doc__


def test_the_tools_know_the_baseline_names():
    import importlib.util
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    spec = importlib.util.spec_from_file_location("playout_names", os.path.join(tools, "playout_names.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse("play") == {} and mod.parse("play8x16") == dict(playouts=8, horizon=16) and mod.parse("play64x1") == dict(playouts=64, horizon=1)
    for bad in ("look", "7", "play8", "playx", "play8x", "deep2", "play-1x2"):
        assert mod.parse(bad) is None
    assert "playout_names" in open(os.path.join(tools, "league.py")).read() and "playout_names" in open(os.path.join(tools, "search_pit.py")).read()


# ---- the statement's own properties ---------------------------------------------------------------------------------------------------
def test_a_blocked_move_scores_minus_one_and_the_others_lie_in_range():
    st = M.CORRIDOR
    plain = R.scores(7, 7, st, 0)
    q = play(st, 0, P=3, T=4, eps=128, seed=5)
    assert plain[2] == -1 and q[2] == -1 and plain[0] >= 0 and plain[1] >= 0
    assert all(0 <= z <= M.high(3, 4) for z in q[:2]) and M.high(64, 64) == 32770
    assert float(np.float32(M.high(64, 64))) == M.high(64, 64)
    small = R.board(5, 5, [([(0, 0), (1, 0)], 0), ([(4, 4), (3, 4)], 2)])           # both heads in corners, facing the edge
    q = M.playout_scores(5, 5, 2, HD, small, 0, 0, 2, 3, 0, 0)
    assert R.scores(5, 5, small, 0)[:2] == [-1, -1] and q[:2] == [-1, -1] and q[2] >= 0


def test_a_dead_end_corridor_that_closes_within_the_horizon():
    st = M.CORRIDOR
    plain, look = R.scores(7, 7, st, 0), K.look_scores(7, 7, 2, HD, st, 0)
    assert plain[1] > plain[0] >= 0 and R.move(plain) == 1                   # the plain script goes for the food in the corridor
    assert look[1] >= look[0] >= 0 and R.move(look) == 1                      # and so does the script one tick deep
    root = M.snake_oracle.Game.from_compact(7, 7, 2, HD, 0.15, st)
    into = [M.playout_value(root, 0, 0, 1, p, 6, 0, 0, R.ALL) for p in range(2)]
    away = [M.playout_value(root, 0, 0, 0, p, 6, 0, 0, R.ALL) for p in range(2)]
    assert into == [4, 4], "four ticks to the end of the corridor, eating there, and no move left at tick 4"
    assert away == [6, 6]
    q = play(st, 0, P=2, T=6, eps=0)
    assert q == [4 * 12 + 1, 4 * 8 + 2, -1] and R.move(q) == 0            # the tie-break counts the blocked move too
    assert R.move(play(st, 0, P=2, T=3, eps=0)) == 1                          # a horizon that ends inside the corridor sees nothing


def test_a_lone_snake_gets_the_plain_scores():
    H, W, S, hd, boards = M.HAND
    st = boards[M.LONE]
    assert M.playout_scores(H, W, S, hd, st, 3, 0, 4, 5, 64, 1) == R.scores(H, W, st, 0) != [-1, -1, -1]
    assert M.playout_scores(H, W, S, hd, st, 3, 1, 4, 5, 64, 1) == [-1, -1, -1]           # a dead snake
    assert M.playout_scores(H, W, S, hd, st, 3, 3, 4, 5, 64, 1) == [-1, -1, -1]           # no such snake


def test_starving_and_meeting_head_on():
    H, W, S, hd, boards = M.HAND
    q = M.playout_scores(H, W, S, hd, boards[M.STARVE], 1, 0, 2, 3, 0, 0)
    open_ = [a for a in range(3) if q[a] != -1]
    assert len(open_) == 3 and all(q[a] // 4 == 2 * 1 for a in open_), "health 2: alive after tick 0, starved at tick 1, twice"
    q = M.playout_scores(H, W, S, hd, boards[M.HEADON], 2, 0, 2, 3, 0, 0)
    assert q[1] // 4 == 0, "straight on into the longer snake's only move: dead at tick 0 in both playouts"
    assert M.playout_scores(H, W, S, hd, boards[M.HEADON], 2, 1, 2, 3, 0, 0)[::2] == [-1, -1]


def test_eps_zero_is_independent_of_the_seed_and_eps_256_is_not():
    H, W, S, hd, boards = M.sampled("7x7x2")
    two = [st for st in boards if st["alive"].sum() == 2][:3]
    assert len(two) == 3
    at = lambda eps, seed: [M.board_playout_scores(H, W, S, hd, st, g, 2, 3, eps, seed) for g, st in enumerate(two)]
    assert at(0, 1) == at(0, 2 ** 63 + 11) == at(0, 0)
    assert at(256, 1) != at(256, 2)
    assert at(256, 1) == at(256, 1)


def test_a_rows_scores_do_not_depend_on_its_place_in_the_list():
    """the key holds the slot and the snake: the statement has no row index at all.  The same board in another slot is another
    position of the key"""
    H, W, S, hd, boards = M.sampled("7x7x2")
    st = next(st for st in boards if st["alive"].sum() == 2)
    one = M.playout_scores(H, W, S, hd, st, 4, 1, 2, 3, 256, 7)
    both = M.board_playout_scores(H, W, S, hd, st, 4, 2, 3, 256, 7)
    assert both[1] == one and M.board_playout_scores(H, W, S, hd, st, 4, 2, 3, 256, 7, only=[1]) == {1: one}
    other = [M.board_playout_scores(H, W, S, hd, st, g, 2, 3, 256, 7) for g in range(5, 9)]
    assert any(o != both for o in other)


# ---- a strength reading of the statement itself ---------------------------------------------------------------------------------------
def test_the_statement_plays_the_plain_script_to_the_end():
    """RefPlayout(P=4, T=6) against RefScripted(), one snake each, on the sixteen recorded 7x7x2 start boards.  The counts are a
    reading, no threshold is set here"""
    out = M.reference("strength-7x7x2")
    n = M.N_DUEL
    wins = sum(w == 0 for w in out["winners"])
    losses = sum(w == 1 for w in out["winners"])
    draws = sum(w is None for w in out["winners"])
    print(f"RefPlayout(P=4, T=6) v RefScripted() on {n} 7x7x2 boards: wins {wins}, draws {draws}, losses {losses}, {out['turns']} turns")
    assert wins + draws + losses == n == len(out["lengths"])
    assert out["turns"] == max(out["lengths"]) and min(out["lengths"]) >= 1 and not out["open"]
    assert all(not (st["alive"][0] and st["alive"][1]) for st in out["boards"])       # every game has its verdict
