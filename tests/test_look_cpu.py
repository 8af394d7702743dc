"""CPU tests of the lookahead opponent's statement (tests/look_ref.py): hand-built 7x7 boards on which the lookahead and the plain
script disagree, each with the reason asserted; the range of the values on sampled golden boards; the library's surface and the
Python layer's refusals (no GPU: nothing is launched); and a strength reading of the statement itself against the plain script.

Cells are (y, x); heading 0 = y-1, 1 = x+1, 2 = y+1, 3 = x-1; move 0 turns left, 1 goes straight, 2 turns right."""
import numpy as np
import pytest

import look_ref as K
import script_ref as R

H = W = 7
HD = 1


def look(st, s, flags=R.ALL):
    return K.look_scores(H, W, len(st["alive"]), HD, st, s, flags)


# A. a tail cell that moves away.  Snake 0 heads up at (3, 3); straight is (2, 3), the tail of snake 1, which lies along row 2 and
# heads right at (2, 5).  Whatever snake 1 does, its tail leaves (2, 3) on the tick (there is no food to grow on).
TAIL = R.board(H, W, [([(3, 3), (4, 3), (5, 3)], 0), ([(2, 5), (2, 4), (2, 3)], 1)])

# B. a head-on cell that a longer snake can reach but need not, beside a wall.  Snake 0 (length 3) heads up the right edge at
# (3, 6): left (3, 5), straight (2, 6), right leaves the board.  Snake 1 (length 4) heads down the same edge at (1, 6): its
# straight is (2, 6) too, its left leaves the board, its right is (1, 5).
HEADON = R.board(H, W, [([(3, 6), (4, 6), (5, 6)], 0), ([(1, 6), (0, 6), (0, 5), (0, 4)], 2)])

# C. two punishable moves with different death counts.  Snake 0 (length 2) heads up at (3, 3).  Snake 1 (length 3) heads down at
# (1, 3): its straight is (2, 3).  Snake 2 (length 3) heads right at (2, 2): its straight is (2, 3), its right is (3, 2).
# Snake 0's left (3, 2) dies in the 3 of 9 replies in which snake 2 turns right; its straight (2, 3) dies in the 3 + 3 - 1 = 5 in
# which snake 1 or snake 2 goes straight; its right (3, 4) is out of everybody's reach.
COUNTS = R.board(H, W, [([(3, 3), (4, 3)], 0), ([(1, 3), (0, 3), (0, 2)], 2), ([(2, 2), (2, 1), (2, 0)], 1)])

# D. food eaten on the tick.  Snake 0 (length 3) heads up at (3, 3) with food on (2, 3), snake 1 sits in a corner.
FOOD = R.board(H, W, [([(3, 3), (4, 3), (5, 3)], 0), ([(6, 5), (6, 6)], 3)], food=[(2, 3)])
NO_FOOD = R.board(H, W, [([(3, 3), (4, 3), (5, 3)], 0), ([(6, 5), (6, 6)], 3)])

# E. the sole survivor.  Snake 1 came into the corner (0, 0) heading x-1 with its body behind and below it: left is (1, 0), a body
# node that is not its tail, straight and right leave the board -- it dies whatever it does.  Snake 0 has three free moves.
DOOMED = R.board(H, W, [([(4, 4), (5, 4), (6, 4)], 0), ([(0, 0), (0, 1), (1, 1), (1, 0), (2, 0)], 3)])


def test_a_tail_cell_that_moves_away():
    assert R.scores(H, W, TAIL, 0)[1] == -1                   # the plain script: the cell is occupied
    children, alive = K.child_boards(H, W, 2, HD, TAIL)
    assert alive == [0, 1] and len(children) == 9
    for c in children:                                        # the reason: in no child does snake 1 still lie on (2, 3)
        assert 2 * W + 3 not in c["nodes"][1][:int(c["length"][1])].tolist()
    q = look(TAIL, 0)
    assert q[1] >= 0 and all(z >= 0 for z in q)
    assert R.move(R.scores(H, W, TAIL, 0)) != 1


def test_a_head_on_cell_ranks_between_a_safe_move_and_a_wall():
    plain, q = R.scores(H, W, HEADON, 0), look(HEADON, 0)
    assert plain[2] == -1 and plain[1] >= 0 and plain[0] >= 0
    leaf, alive = K.leaves(H, W, 2, HD, HEADON)
    # child j: snake 0 moves j % 3, snake 1 moves j // 3.  Straight against straight: the longer snake 1 wins the head-on
    assert 0 not in leaf[1 + 3 * 1] and leaf[1 + 3 * 1][1] == K.WIN
    assert [0 in leaf[1 + 3 * b] for b in range(3)] == [True, False, True]        # snake 1 need not go there
    assert all(0 not in leaf[2 + 3 * b] for b in range(3))                        # the wall kills whatever snake 1 does
    assert q[1] == -2 - 1 and q[2] == -2 - 3
    assert q[0] >= 0 and q[0] > q[1] > q[2]
    assert leaf[0 + 3 * 0] == {0: K.WIN}                      # snake 1 leaves the board: a leaf of 2^24, which the minimum hides
    assert q[0] == min(leaf[0 + 3 * b][0] for b in range(3)) < K.WIN
    assert R.move(q) == 0
    assert look(HEADON, 1)[0] == -5                           # snake 1's own way off the board


def test_two_punishable_moves_with_different_death_counts():
    q = look(COUNTS, 0)
    assert q[0] == -2 - 3 and q[1] == -2 - 5 and q[2] >= 0
    assert R.move([q[0], q[1], -30]) == 0                     # of the two, the move with fewer ways to die ranks higher
    assert all(z >= 0 for z in R.scores(H, W, COUNTS, 0))     # the plain script sees three open cells


def test_food_eaten_on_the_tick_raises_the_leafs_room():
    with_food, without = look(FOOD, 0, R.SPACE), look(NO_FOOD, 0, R.SPACE)
    assert without[1] >> 16 == 3 and with_food[1] >> 16 == 4  # room = min(space, length): the length is 4 after eating
    assert with_food[0] >> 16 == without[0] >> 16 == 3 and with_food[2] >> 16 == 3
    children, _ = K.child_boards(H, W, 2, HD, FOOD)
    assert [int(c["length"][0]) for c in children] == [3, 4, 3] * 3 and [int(c["health"][0]) for c in children] == [89, 100, 89] * 3


def test_a_sole_survivor_scores_two_to_the_24():
    leaf, _ = K.leaves(H, W, 2, HD, DOOMED)
    assert leaf == [{0: K.WIN}] * 9
    assert look(DOOMED, 0) == [1 << 24] * 3
    assert look(DOOMED, 1) == [-5, -5, -5]
    assert float(np.float32(1 << 24)) == 1 << 24 and float(np.float32(-29)) == -29


def test_one_and_five_alive_snakes_get_the_plain_scores():
    one = R.board(H, W, [([(3, 3), (4, 3), (5, 3)], 0), ([(2, 5), (2, 4), (2, 3)], 1)], dead=[1])
    assert look(one, 0) == R.scores(H, W, one, 0) and look(one, 1) == [-1, -1, -1]
    five = R.board(H, W, [([(1, 1), (1, 0)], 1), ([(1, 5), (1, 6)], 3), ([(5, 1), (5, 0)], 1), ([(5, 5), (5, 6)], 3),
                          ([(3, 3), (4, 3)], 0)], food=[(3, 0)])
    for s in range(5):
        assert look(five, s) == R.scores(H, W, five, s)
    four = {k: v.copy() for k, v in five.items()}
    four["alive"][4] = 0                                      # one snake fewer: looked ahead, and no longer the plain scores
    assert K.board_look_scores(H, W, 5, HD, four) != R.board_scores(H, W, four)
    assert look(four, 4) == [-1, -1, -1] and look(four, 5) == [-1, -1, -1] and look(four, -1) == [-1, -1, -1]


@pytest.mark.parametrize("cfg", list(K.STRIDE))
def test_every_value_on_the_sampled_golden_boards_is_in_range(cfg):
    H_, W_, S, hd, boards = K.sampled(cfg)
    got = K.sampled_scores(cfg)
    assert len(got) == len(boards) >= 30
    vals = [z for q in got for row in q.values() for z in row]
    assert len(vals) >= 150 and all(isinstance(z, (int, np.integer)) and K.LOW <= z <= K.HIGH for z in vals)
    assert any(z <= -3 for z in vals) and any(z >= 0 for z in vals)
    alive = [int(np.count_nonzero(st["alive"])) for st in boards]
    if S > 4:                                                 # the fallback while more than four live, the full fanout afterwards
        assert any(a > 4 for a in alive) and any(2 <= a <= 4 for a in alive)


# ---- the library's surface and the Python layer (nothing is launched) ---------------------------------------------------------------
def test_the_entry_points_are_exported_with_their_prototypes():
    import snake_engine
    from snake_engine import _lib
    L = snake_engine.lib()
    for name, n_args in (("snk_pit_look_fanout", 1), ("snk_pit_look_scratch_elems", 2), ("snk_pit_look_values", 8)):
        assert hasattr(L, name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args and getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    assert L.snk_version() == _lib.ABI_VERSION == 113
    assert [L.snk_pit_look_fanout(S) for S in range(2, 9)] == [9, 27, 81, 81, 81, 81, 81] == [K.fanout(S) for S in range(2, 9)]
    assert [L.snk_pit_look_fanout(S) for S in (-3, 0, 1, 9, 1 << 20)] == [-1] * 5


def test_the_scratch_functions_refusals():
    import snake_engine
    L = snake_engine.lib()
    assert L.snk_pit_look_scratch_elems(-1, 4) == -1
    assert [L.snk_pit_look_scratch_elems(8, S) for S in (1, 9, 0)] == [-1] * 3
    assert L.snk_pit_look_scratch_elems((1 << 28) // 81 + 1, 4) == -1 and L.snk_pit_look_scratch_elems((1 << 28) // 81, 4) > 0
    sizes = [L.snk_pit_look_scratch_elems(m, 4) for m in (0, 1, 2, 1000, 16384)]
    assert sizes == sorted(sizes) and sizes[0] >= 0
    # int32 elements: per row its group, source, bits and plain scores; per leaf a pair and three scores, and S + 1 bytes
    assert sizes[3] >= 1000 * (3 + 3) + 81000 * (2 + 3) + 81000 * (4 + 1) // 4
    assert L.snk_pit_look_scratch_elems(1000, 2) < sizes[3] < L.snk_pit_look_scratch_elems(1000, 8)


def test_lookahead_is_a_scripted_with_its_refusals():
    from snake_engine import arena
    from snake_engine.arena import Arena, Lookahead, Scripted, Searcher
    s = Lookahead()
    assert isinstance(s, Scripted) and s.flags == 7 and not hasattr(s, "v_device")
    assert Lookahead(0).flags == 0 and Lookahead(5).flags == 5
    with pytest.raises(ValueError):
        Lookahead(8)
    with pytest.raises(TypeError):
        Searcher(s)
    net = type("Net", (), {"v_device": lambda self, planes, mask: None})()
    a, b = Arena._sides(s, net, dict(breadth=8, depth=4), 3)
    assert a is s and isinstance(b, Searcher)
    assert arena.LOOK_SLOT_BUDGET // 81 >= 4096 * 4           # a 4 096-game 11x11x4 match, every seat, in one chunk


# ---- a strength reading of the statement itself ---------------------------------------------------------------------------------------
def test_the_statement_plays_the_plain_script_to_the_end():
    """RefLookahead() against RefScripted(), one snake each, on the sixteen recorded 7x7x2 start boards.  The counts are a reading
    (DESIGN section 7 quotes them), no threshold is set here"""
    out = K.reference("duel-7x7x2")
    n = K.N_DUEL
    wins = sum(w == 0 for w in out["winners"])
    losses = sum(w == 1 for w in out["winners"])
    draws = sum(w is None for w in out["winners"])
    print(f"RefLookahead() v RefScripted() on {n} 7x7x2 boards: wins {wins}, draws {draws}, losses {losses}, {out['turns']} turns")
    assert wins + draws + losses == n == len(out["lengths"])
    assert out["turns"] == max(out["lengths"]) and min(out["lengths"]) >= 1
    assert all(not (st["alive"][0] and st["alive"][1]) for st in out["boards"])       # every game has its verdict
