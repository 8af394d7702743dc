"""CPU tests of the scripted opponent's statement (tests/script_ref.py) on hand-built 7x7 boards whose answers are worked out
by hand below, of the tie order, of the ABI entry and of the Python layer's refusals (no GPU: nothing is launched).

Cells are (y, x); heading 0 = y-1, 1 = x+1, 2 = y+1, 3 = x-1; move 0 turns left, 1 goes straight, 2 turns right.  H + W = 14.
BOARDS is also what tests/test_script_gpu.py imports into an engine: the kernel must give the same hand-checked numbers."""
import numpy as np
import pytest

import script_ref as R

H = W = 7


def sc(room, safe, food, fill):
    return ((room * 2 + safe) * 64 + food) * 512 + fill


def by_flags(parts, length, flags):
    """the scores of hand-worked parts [(space, safe, food) or None for a blocked move] under a flag subset"""
    out = []
    for p in parts:
        if p is None:
            out.append(-1)
            continue
        space, safe, food = p
        space = space if flags & R.SPACE else 0
        out.append(sc(min(space, length, 255), safe if flags & R.HEADS else 1, food if flags & R.FOOD else 0, min(space, 511)))
    return out


# A. a pocket next to an open side.  Snake 0 (length 4) heads up at (2, 1) with its body down column 1 and its tail at (4, 0);
# snake 1 lies along the top edge with its tail at (1, 0).  Left is (2, 0): with (3, 0) a pocket of TWO cells, closed by (1, 0),
# (4, 0), (3, 1) and the head.  Straight (1, 1) and right (2, 2) both open on everything else: 49 - 8 bodies - 2 pocket = 39.
# Snake 1 is as long as snake 0, but its head (0, 2) is two steps from (1, 1) and from (2, 2): every move is safe.  No food.
POCKET = R.board(H, W, [([(2, 1), (3, 1), (4, 1), (4, 0)], 0), ([(0, 2), (0, 1), (0, 0), (1, 0)], 1)])
POCKET_PARTS = [(2, 1, 0), (39, 1, 0), (39, 1, 0)]

# B. heads.  Snake 0 (length 3) heads up at (3, 3).  Left (3, 2) is next to the head (3, 1) of snake 1 (length 4, longer): unsafe.
# Straight (2, 3) is next to the head (1, 3) of snake 2 (length 3, equal): unsafe.  Right (3, 4) is next to the head (3, 5) of
# snake 3 (length 2, shorter): safe.  Every other head is three steps from every other target.  12 body cells, the 37 free
# cells are one region.  Food at (0, 0): 5 steps from (3, 2) and from (2, 3) -> 14 - 5 = 9; 7 steps from (3, 4) -> 7.
HEADS = R.board(H, W, [([(3, 3), (4, 3), (5, 3)], 0), ([(3, 1), (4, 1), (5, 1), (6, 1)], 0), ([(1, 3), (0, 3), (0, 4)], 2),
                       ([(3, 5), (4, 5)], 0)], food=[(0, 0)])
HEADS_PARTS = [(37, 0, 9), (37, 0, 9), (37, 1, 7)]

# C. the same with snake 1 dead: its four cells are free (41 in one region) and its head frightens nobody, so left is safe.
HEADS_DEAD = R.board(H, W, [([(3, 3), (4, 3), (5, 3)], 0), ([(3, 1), (4, 1), (5, 1), (6, 1)], 0), ([(1, 3), (0, 3), (0, 4)], 2),
                            ([(3, 5), (4, 5)], 0)], food=[(0, 0)], dead=[1])
HEADS_DEAD_PARTS = [(41, 1, 9), (41, 0, 9), (41, 1, 7)]

# D. two foods at equal distance.  Snake 0 (length 3) heads up at (3, 3), snake 1 (length 2, shorter) sits in the corner; 44 free
# cells, one region.  Food at (3, 0) and (0, 3).  Left (3, 2): 2 and 4 steps -> 14 - 2 = 12.  Straight (2, 3): 4 and 2 -> 12.
# Right (3, 4): 4 and 4, the two foods at the same distance -> 10.
FOODS = R.board(H, W, [([(3, 3), (4, 3), (5, 3)], 0), ([(6, 6), (6, 5)], 1)], food=[(3, 0), (0, 3)])
FOODS_PARTS = [(44, 1, 12), (44, 1, 12), (44, 1, 10)]

# E. every move blocked.  Snake 0 came along the top edge into the corner (0, 0), heading 3 (x-1), and its tail lies at (1, 0):
# left is (1, 0), its own tail (tails count); straight and right leave the board.
BLOCKED = R.board(H, W, [([(0, 0), (0, 1), (1, 1), (1, 0)], 3), ([(6, 6), (6, 5), (6, 4)], 1)])
BLOCKED_PARTS = [None, None, None]

# F. board A with snake 1 dead: the wall at (1, 0) is gone, the pocket is part of the one region of 49 - 4 = 45 cells.
POCKET_DEAD = R.board(H, W, [([(2, 1), (3, 1), (4, 1), (4, 0)], 0), ([(0, 2), (0, 1), (0, 0), (1, 0)], 1)], dead=[1])
POCKET_DEAD_PARTS = [(45, 1, 0), (45, 1, 0), (45, 1, 0)]

# name: (board, snake, its length, the hand-worked parts per move, the move with all flags on)
BOARDS = {
    "pocket": (POCKET, 0, 4, POCKET_PARTS, 2),            # straight and right tie above the pocket: the later one
    "heads": (HEADS, 0, 3, HEADS_PARTS, 2),               # the only safe move
    "heads-dead": (HEADS_DEAD, 0, 3, HEADS_DEAD_PARTS, 0),    # left and right are safe, left is nearer the food
    "foods": (FOODS, 0, 3, FOODS_PARTS, 1),               # left and straight tie: the later one
    "blocked": (BLOCKED, 0, 4, BLOCKED_PARTS, 2),         # all -1: 2
    "pocket-dead": (POCKET_DEAD, 0, 4, POCKET_DEAD_PARTS, 2),
}


@pytest.mark.parametrize("name", list(BOARDS))
def test_hand_built_board(name):
    st, s, length, parts, want_move = BOARDS[name]
    assert int(st["length"][s]) == length
    got = R.scores(H, W, st, s)
    assert got == by_flags(parts, length, R.ALL), name
    assert R.move(got) == want_move
    assert all(-1 <= z < 1 << 24 for z in got)                # exact as float32


def test_the_pocket_scores_spelled_out():
    """room is the pocket's 2 against the snake's 4: ((2*2+1)*64+0)*512+2 against ((4*2+1)*64+0)*512+39"""
    assert R.scores(H, W, POCKET, 0) == [163842, 294951, 294951]
    assert R.scores(H, W, HEADS, 0) == [(6 * 64 + 9) * 512 + 37, (6 * 64 + 9) * 512 + 37, (7 * 64 + 7) * 512 + 37]
    assert R.scores(H, W, FOODS, 0) == [(7 * 64 + 12) * 512 + 44, (7 * 64 + 12) * 512 + 44, (7 * 64 + 10) * 512 + 44]
    assert R.scores(H, W, BLOCKED, 0) == [-1, -1, -1]


@pytest.mark.parametrize("flags", range(8))
def test_each_flag_subset(flags):
    for name, (st, s, length, parts, _) in BOARDS.items():
        assert R.scores(H, W, st, s, flags) == by_flags(parts, length, flags), (name, flags)
    # flags = 0: any unblocked move scores the same
    if flags == 0:
        assert R.scores(H, W, HEADS, 0, 0) == [64 * 512] * 3 and R.scores(H, W, BLOCKED, 0, 0) == [-1] * 3


def test_a_dead_snake_scores_nothing_and_occupies_nothing():
    assert R.scores(H, W, POCKET_DEAD, 1) == [-1, -1, -1]
    assert R.scores(H, W, POCKET_DEAD, 2) == [-1, -1, -1] and R.scores(H, W, POCKET_DEAD, -1) == [-1, -1, -1]
    # the live snake 1 of board A: heads right along the top edge at (0, 2); left leaves the board, straight (0, 3) and right
    # (1, 2) open on the 39 cells; snake 0 is as long (4) and its head (2, 1) is two steps from (1, 2) and four from (0, 3)
    assert R.scores(H, W, POCKET, 1) == [-1, sc(4, 1, 0, 39), sc(4, 1, 0, 39)]


def test_the_tie_order_is_that_of_the_pit_moves():
    from oracle.mcts_oracle import argmaxs
    cases = [(5, 5, 1), (5, 1, 5), (1, 5, 5), (5, 5, 5), (-1, -1, -1), (3, 2, 1), (1, 3, 2), (1, 2, 3), (-1, 7, 7), (7, -1, 7)]
    assert [R.move(z) for z in cases] == [1, 2, 2, 2, 2, 0, 1, 2, 2, 2]
    assert [int(m) for m in argmaxs(np.array(cases, np.float32))] == [R.move(z) for z in cases]


def test_flood_counts_by_a_queue():
    assert R.flood(5, 5, set(), 2, 2) == 25
    wall = {1 * 5 + x for x in range(5)}                      # row 1 closed: row 0 is a region of 5, rows 2..4 one of 15
    assert R.flood(5, 5, wall, 0, 4) == 5 and R.flood(5, 5, wall, 4, 0) == 15
    assert R.flood(5, 5, wall - {1 * 5 + 4}, 0, 0) == 21      # a door at the row's end: no wrap to the next row's start needed


# ---- the ABI and the Python layer (nothing is launched) -----------------------------------------------------------------------------
def test_the_entry_point_is_exported_with_its_prototype():
    import snake_engine
    from snake_engine import _lib
    L = snake_engine.lib()
    assert hasattr(L, "snk_pit_script_values")
    restype, args = _lib.PROTOTYPES["snk_pit_script_values"]
    assert len(args) == 6
    txt = open(__import__("os").path.join(__import__("conftest").REPO, "include", "snake_engine.h")).read()
    for name, value in (("SNK_SCRIPT_SPACE", 1), ("SNK_SCRIPT_HEADS", 2), ("SNK_SCRIPT_FOOD", 4)):
        assert f"#define {name} {value}u" in txt
    from snake_engine import arena
    assert (arena.SCRIPT_SPACE, arena.SCRIPT_HEADS, arena.SCRIPT_FOOD) == (1, 2, 4) == (R.SPACE, R.HEADS, R.FOOD)


def test_scripted_holds_flags_only_and_cannot_be_searched():
    from snake_engine.arena import Arena, Scripted, Searcher
    from snake_engine import league
    s = Scripted()
    assert s.flags == 7 and vars(s) == {"flags": 7} and not hasattr(s, "v_device")
    assert Scripted(0).flags == 0 and Scripted(5).flags == 5
    with pytest.raises(ValueError):
        Scripted(8)
    with pytest.raises(TypeError):
        Searcher(s)
    net = type("Net", (), {"v_device": lambda self, planes, mask: None})()
    a, b = Arena._sides(s, net, dict(breadth=8, depth=4), 3)
    assert a is s and isinstance(b, Searcher) and b.net is net
    assert Arena._sides(s, net, None, 3) == (s, net)
    sides = league.searchers([net, s, net], dict(breadth=8, depth=4), seed=1)
    assert sides[1] is s and isinstance(sides[0], Searcher) and isinstance(sides[2], Searcher) and sides[2].seed == 1 + 303


def test_owner_table_accepts_a_scripted_owner_and_keeps_its_refusals():
    from snake_engine.arena import Scripted, Searcher
    from snake_engine.league import League
    lg = League.__new__(League)
    lg.game_cnt, lg.snake_cnt = 4, 2
    net = type("Net", (), {"v_device": lambda self, planes, mask: None})()
    ok = np.array([[0, 1]] * 4)
    assert lg._owner_table([Scripted(), net], ok).dtype == np.uint8
    assert lg._owner_table([Scripted(), Scripted(1)], ok).tolist() == ok.tolist()
    assert lg._owner_table([Scripted(), Searcher(net)], ok, searchers=True).shape == (4, 2)
    with pytest.raises(TypeError, match="a Searcher cannot sit in League.play"):
        lg._owner_table([Scripted(), Searcher(net)], ok)
    with pytest.raises(TypeError, match="has no v_device"):
        lg._owner_table([Scripted(), object()], ok)
    with pytest.raises(ValueError, match="outside 0..1"):
        lg._owner_table([Scripted(), net], np.array([[0, 2]] * 4))
