"""CPU tests of the deep opponent's statement (tests/deep_ref.py): depth 1 is the lookahead's statement; hand-built 7x7 boards on
which depth 2 and depth 1 choose differently, each with the reason asserted; the ordering constants; the range of the values on
sampled golden boards; the library's surface and the Python layer's refusals (no GPU: nothing is launched); and a strength
reading of the statement itself against the lookahead's.

Cells are (y, x); heading 0 = y-1, 1 = x+1, 2 = y+1, 3 = x-1; move 0 turns left, 1 goes straight, 2 turns right."""
import numpy as np
import pytest

import deep_ref as D
import look_ref as K
import script_ref as R

H = W = 7
HD = 1


def deep(st, s, depth=2, flags=R.ALL):
    return D.deep_scores(H, W, len(st["alive"]), HD, st, s, depth, flags)


def look(st, s, flags=R.ALL):
    return K.look_scores(H, W, len(st["alive"]), HD, st, s, flags)


def child(st, moves):
    """the board after one tick in which alive snake k makes moves[k]"""
    children, alive = K.child_boards(H, W, len(st["alive"]), HD, st)
    return children[sum(m * 3 ** k for k, m in enumerate(moves))]


# A. a corridor that closes behind the head.  Snake 0 (length 4) heads down the left edge at (2, 0): left is (2, 1), straight is
# (3, 0), right leaves the board.  Snake 1 (length 5, its tail doubled after a meal) heads x-1 at (4, 2).  One tick deep both open
# cells score the same and the tie goes to the later move, straight.  But when snake 1 answers with (4, 1), snake 0 stands at
# (3, 0) between the edge, its own neck and the cells (3, 1) and (4, 0), both of which the longer snake 1 can enter next.
TRAP = R.board(H, W, [([(2, 0), (1, 0), (1, 1), (1, 2)], 2), ([(4, 2), (4, 3), (4, 4), (4, 5), (4, 5)], 3)],
               food=[(0, 0), (5, 2), (6, 4)])

# B. a head-on that can only be forced on the second tick.  Snake 0 (length 4) heads x+1 along the top edge at (0, 3), its tail
# below it on (1, 2): left leaves the board, straight is (0, 4), right is (1, 3).  Snake 1 (length 5) heads up at (2, 5) and can
# reach neither cell on this tick.  Food on (0, 6) draws the lookahead straight on.  After straight against straight snake 0
# stands at (0, 4) and snake 1 at (1, 5), next to both (0, 5) and (1, 4): whichever snake 0 takes, snake 1 can meet it there.
HEADON2 = R.board(H, W, [([(0, 3), (0, 2), (1, 2), (1, 1)], 1), ([(2, 5), (3, 5), (4, 5), (5, 5), (6, 5)], 0)], food=[(0, 6)])

# C. a win seen at tick two.  Snake 1 (length 9) has coiled itself around the corner: from (0, 1), heading up, left is (0, 0),
# straight leaves the board and right is its own body.  It lives through this tick by entering (0, 0) and dies on the next
# whatever it does.  Snake 0 is far away with three free moves and food to its left.
WIN2 = R.board(H, W, [([(4, 4), (5, 4), (6, 4)], 0),
                      ([(0, 1), (1, 1), (1, 0), (2, 0), (2, 1), (2, 2), (1, 2), (0, 2), (0, 3)], 0)], food=[(4, 3)])

# D. two moves that can be punished at once, with different death counts: test_look_cpu's board C
COUNTS = R.board(H, W, [([(3, 3), (4, 3)], 0), ([(1, 3), (0, 3), (0, 2)], 2), ([(2, 2), (2, 1), (2, 0)], 1)])


def test_depth_one_is_the_lookahead_on_every_sampled_golden_board():
    for cfg in K.STRIDE:
        Hh, Ww, S, hd, boards = K.sampled(cfg)
        want = K.sampled_scores(cfg)
        for st, w in zip(boards, want):
            assert D.board_deep_scores(Hh, Ww, S, hd, st, 1) == w
    assert D.low(1) == K.LOW and D.WIN == K.WIN


def test_a_corridor_that_closes_behind_the_head():
    q1, q2 = look(TRAP, 0), deep(TRAP, 0)
    assert q1[0] == q1[1] >= 0 and R.move(q1) == 1            # one tick deep: a tie, and the later move wins it
    shut = child(TRAP, (1, 1))                                # straight, and snake 1 straight on to (4, 1)
    assert shut["nodes"][0][0] == 3 * W + 0 and shut["nodes"][1][0] == 4 * W + 1
    below = look(shut, 0)
    assert below == [-3, -3, -5]                              # (3, 1) and (4, 0) can each be met by snake 1, the third is the edge
    assert q2[1] == max(below) == -3                          # the reason: every continuation of the worst reply is punishable
    assert q2[0] >= 0 and R.move(q2) == 0
    assert q2[2] == -2 - 3 - 32 and q1[2] == -2 - 3           # the edge itself: death on this tick


def test_a_head_on_that_can_only_be_forced_on_the_second_tick():
    q1, q2 = look(HEADON2, 0), deep(HEADON2, 0)
    assert R.move(q1) == 1 and q1[1] >= 0                     # no reply can punish (0, 4) on this tick
    met = child(HEADON2, (1, 1))
    assert met["nodes"][0][0] == 0 * W + 4 and met["nodes"][1][0] == 1 * W + 5
    below = look(met, 0)
    assert below[0] == -5 and below[1] == -3 and below[2] == -3
    for mine, its in ((1, 1), (2, 0)):                        # the head-ons themselves: (0, 5) and (1, 4), the shorter snake dies
        hit = child(met, (mine, its))
        assert not hit["alive"][0] and hit["alive"][1]
    assert q2[1] == -3 and q2[2] >= 0 and R.move(q2) == 2


def test_a_win_seen_at_tick_two():
    q1, q2 = look(WIN2, 0), deep(WIN2, 0)
    assert max(q1) < D.WIN and R.move(q1) == 0                # one tick deep snake 1 lives on in (0, 0): go for the food
    assert look(WIN2, 1) == [-1, -5, -5]                      # its own view: one move left, into a cell with no way out
    for reply in range(3):                                    # the reason: after two ticks snake 1 is dead whatever both did
        c = child(WIN2, (1, reply))
        if c["alive"][1]:
            assert reply == 0 and all(not child(c, (1, r))["alive"][1] for r in range(3))
    assert q2 == [D.WIN] * 3 and R.move(q2) == 2
    assert deep(WIN2, 1) == [-5, -2 - 3 - 32, -2 - 3 - 32]    # death at tick two ranks above death now


def test_the_ordering_constants():
    assert D.STEP_PENALTY > 27 and D.low(2) == -61 and D.low(4) == -125
    q1, q2 = look(COUNTS, 0), deep(COUNTS, 0)
    assert q1[0] == -2 - 3 and q1[1] == -2 - 5
    assert q2[0] == -2 - 3 - 32 and q2[1] == -2 - 5 - 32      # fewer ways to die ranks higher at the same tick
    assert R.move([q2[0], q2[1], -100]) == 0
    trap = deep(TRAP, 0)                                      # an immediate punishable move scores below a move whose every
    assert max(q2[0], q2[1], trap[2]) < D.low(1) <= -29 <= min(look(met, 0)[1] for met in [child(HEADON2, (1, 1))])
    assert trap[2] < trap[1] < 0                              # continuation is punishable
    assert float(np.float32(D.low(4))) == D.low(4)


@pytest.mark.parametrize("cfg", ["7x7x2", "9x9x3"])
def test_every_depth_two_value_on_the_sampled_golden_boards_is_in_range(cfg):
    H_, W_, S, hd, boards = D.sampled(cfg)
    got = D.sampled_scores(cfg, 2)
    assert len(got) == len(boards) >= 8
    vals = [z for q in got for row in q.values() for z in row]
    assert len(vals) >= 40 and all(isinstance(z, (int, np.integer)) and -61 <= z <= 1 << 24 for z in vals)
    assert any(z <= -35 for z in vals) and any(z >= 0 for z in vals)


# ---- the library's surface and the Python layer (nothing is launched) ---------------------------------------------------------------
def test_the_entry_points_are_exported_with_their_prototypes():
    import snake_engine
    from snake_engine import _lib
    L = snake_engine.lib()
    for name, n_args in (("snk_pit_deep_fanout", 2), ("snk_pit_deep_scratch_elems", 3), ("snk_pit_deep_values", 9)):
        assert hasattr(L, name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args and getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    assert L.snk_version() == _lib.ABI_VERSION == 113


def test_the_fanout_table():
    import snake_engine
    L = snake_engine.lib()
    assert [L.snk_pit_deep_fanout(2, d) for d in range(1, 6)] == [9, 81, 729, 6561, -1]
    assert [L.snk_pit_deep_fanout(3, d) for d in range(1, 4)] == [27, 729, -1]
    for S in range(4, 9):
        assert [L.snk_pit_deep_fanout(S, d) for d in range(1, 4)] == [81, 6561, -1]
    assert [L.snk_pit_deep_fanout(S, 1) for S in (-3, 0, 1, 9, 1 << 20)] == [-1] * 5
    assert [L.snk_pit_deep_fanout(2, d) for d in (0, -1, -(1 << 31), 1 << 30)] == [-1] * 4
    for S in range(2, 9):
        assert L.snk_pit_deep_fanout(S, 1) == L.snk_pit_look_fanout(S)
        for d in range(0, 6):
            assert L.snk_pit_deep_fanout(S, d) == D.fanout(S, d)


def test_the_scratch_function():
    import snake_engine
    L = snake_engine.lib()
    for S in range(2, 9):
        for m in (0, 1, 2, 255, 1000, 16384):
            assert L.snk_pit_deep_scratch_elems(m, S, 1) == L.snk_pit_look_scratch_elems(m, S) >= 0
        for m in (0, 1, 2, 100, 1000):                            # depth 1 is the lookahead: one scratch plan
            assert L.snk_pit_deep_scratch_elems(m, S, 1) == L.snk_pit_look_scratch_elems(m, S)
    assert L.snk_pit_deep_scratch_elems(-1, 4, 2) == -1
    assert [L.snk_pit_deep_scratch_elems(8, S, 2) for S in (1, 9, 0)] == [-1] * 3
    assert [L.snk_pit_deep_scratch_elems(8, S, d) for S, d in ((4, 0), (4, 3), (3, 3), (2, 5), (2, -1))] == [-1] * 5
    assert L.snk_pit_deep_scratch_elems((1 << 28) // 6561 + 1, 4, 2) == -1 and L.snk_pit_deep_scratch_elems((1 << 28) // 6561, 4, 2) > 0
    for S, d in ((2, 2), (2, 4), (3, 2), (4, 2)):
        sizes = [L.snk_pit_deep_scratch_elems(m, S, d) for m in (0, 1, 2, 100, 1000)]
        assert sizes == sorted(sizes) and sizes[0] >= 0
        FD = L.snk_pit_deep_fanout(S, d)
        # int32 elements: per leaf row a pair and three scores; per leaf node S + 1 bytes
        assert sizes[3] >= 100 * FD * (2 + 3) + 100 * FD * (S + 1) // 4


def test_deep_is_a_scripted_with_its_refusals():
    from snake_engine import arena
    from snake_engine.arena import Arena, Deep, Scripted, Searcher
    s = Deep()
    assert isinstance(s, Scripted) and s.flags == 7 and s.depth == 2 and not hasattr(s, "v_device")
    assert Deep(0).flags == 0 and Deep(5, 3).depth == 3 and Deep(depth=1).depth == 1
    with pytest.raises(ValueError):
        Deep(8)
    with pytest.raises(ValueError):
        Deep(depth=0)
    with pytest.raises(TypeError):
        Searcher(s)
    net = type("Net", (), {"v_device": lambda self, planes, mask: None})()
    a, b = Arena._sides(s, net, dict(breadth=8, depth=4), 3)
    assert a is s and isinstance(b, Searcher)
    assert arena.DEEP_BYTE_BUDGET == 1 << 30


# ---- a strength reading of the statement itself ---------------------------------------------------------------------------------------
def test_the_statement_plays_the_lookahead_to_the_end():
    """RefDeep(2) against RefLookahead(), one snake each, on the sixteen recorded 7x7x2 start boards.  The counts are a reading,
    no threshold is set here"""
    out = D.reference("duel-7x7x2")
    n = D.N_DUEL
    wins = sum(w == 0 for w in out["winners"])
    losses = sum(w == 1 for w in out["winners"])
    draws = sum(w is None for w in out["winners"])
    print(f"RefDeep(2) v RefLookahead() on {n} 7x7x2 boards: wins {wins}, draws {draws}, losses {losses}, {out['turns']} turns")
    assert wins + draws + losses == n == len(out["lengths"])
    assert out["turns"] == max(out["lengths"]) and min(out["lengths"]) >= 1 and not out["open"]
    assert all(not (st["alive"][0] and st["alive"][1]) for st in out["boards"])       # every game has its verdict
