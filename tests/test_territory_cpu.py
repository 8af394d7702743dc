"""CPU tests of the territory opponent's statement (tests/territory_ref.py): the two facts that follow from the definition on the
golden trajectories, hand-made boards for the head-on rule, the hungry threshold, a reading of the statement against the plain
script, and the ABI entry and the Python layer's refusals (no GPU: nothing is launched).

Cells are (y, x); heading 0 = y-1, 1 = x+1, 2 = y+1, 3 = x-1; move 0 turns left, 1 goes straight, 2 turns right."""
import os

import numpy as np
import pytest

import script_ref as R
import territory_ref as T

SMALL = ["5x5x2", "7x7x2", "9x9x3", "11x11x4"]


# ---- the two facts that follow from the definition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", SMALL)
def test_territory_never_exceeds_space_on_the_golden_trajectories(cfg):
    """every alive row of every board: the same moves are blocked, safe and food are the script's, and room and fill -- below their
    caps on these boards -- are at most the script's; somewhere they are smaller"""
    H, W, S, boards = T.golden(cfg)
    assert H * W < 255
    rows = smaller = 0
    for st, terr in zip(boards, T.golden_scores(cfg)):
        plain = R.board_scores(H, W, st)
        assert sorted(terr) == sorted(plain) == [s for s in range(S) if st["alive"][s]]
        for s in terr:
            rows += 1
            for zt, zp in zip(terr[s], plain[s]):
                assert (zt == -1) == (zp == -1)
                if zt != -1:
                    (room_t, safe_t, food_t, fill_t), (room_p, safe_p, food_p, fill_p) = T.parts(zt), T.parts(zp)
                    assert (safe_t, food_t) == (safe_p, food_p) and fill_t <= fill_p and room_t <= room_p
                    assert room_t == min(fill_t, int(st["length"][s]))
                    smaller += fill_t < fill_p
    assert rows > 100 and smaller > 0


@pytest.mark.parametrize("cfg", SMALL)
def test_a_lone_snake_gets_the_scripts_scores(cfg):
    """s the only alive snake: no front but its own, and the scores at hungry = 100 are the script's -- on the boards of the
    trajectories that have one snake left, and on every board with all snakes but one declared dead"""
    H, W, S, boards = T.golden(cfg)
    made = 0
    for i, st in enumerate(boards):
        alive = [s for s in range(S) if st["alive"][s]]
        if len(alive) == 1:
            assert T.scores(H, W, st, alive[0]) == R.scores(H, W, st, alive[0])
        elif alive:
            made += 1
            s = alive[i % len(alive)]
            alone = dict(st, alive=np.array([int(t == s) for t in range(S)], np.uint8))
            for flags in (R.ALL, R.SPACE, R.HEADS | R.FOOD):
                assert T.scores(H, W, alone, s, flags) == R.scores(H, W, alone, s, flags)
            assert T.scores(H, W, alone, alive[(i + 1) % len(alive)]) == [-1, -1, -1]
    assert made > 50


# ---- the head-on rule: a corridor of five cells entered from both ends -------------------------------------------------------------
def corridor(len_a, len_b):
    """7x7.  Row 1 is bodies from edge to edge, so row 0 is a corridor one cell wide.  Snake 0 stands at its west end, head (0, 0)
    heading east, body (1, 0), (1, 1), (1, 2) and on into row 2; snake 1 at its east end, head (0, 6) heading west, body (1, 6),
    (1, 5), (1, 4), (1, 3) and on into row 2.  Either has ONE open move, straight into the corridor: (0, 1) and (0, 5).  The five
    free cells (0, 1) .. (0, 5) lie 0, 1, 2, 3, 4 steps from snake 0's target and 4, 3, 2, 1, 0 from snake 1's: the middle cell
    (0, 3) is the tie"""
    assert 4 <= len_a <= 6 and 5 <= len_b <= 7
    a = [(0, 0), (1, 0), (1, 1), (1, 2), (2, 2), (2, 1)][:len_a]
    b = [(0, 6), (1, 6), (1, 5), (1, 4), (1, 3), (2, 3), (2, 4)][:len_b]
    return R.board(7, 7, [(a, 1), (b, 3)])


@pytest.mark.parametrize("len_a, len_b, mine, theirs", [(6, 5, 3, 2),      # the longer snake takes the tie cell
                                                        (5, 5, 2, 2),      # equal lengths: neither does
                                                        (4, 5, 2, 3)])     # the shorter snake loses it
def test_a_tie_goes_to_the_longer_snake_and_an_equal_tie_to_neither(len_a, len_b, mine, theirs):
    st = corridor(len_a, len_b)
    for s, want in ((0, mine), (1, theirs)):
        q, plain = T.scores(7, 7, st, s), R.scores(7, 7, st, s)
        assert [z == -1 for z in q] == [True, False, True] == [z == -1 for z in plain]
        room, safe, food, fill = T.parts(q[1])
        assert (room, safe, food, fill) == (want, 1, 0, want) and T.parts(plain[1]) == (min(5, int(st["length"][s])), 1, 0, 5)
    y, x = T.targets(7, 7, st, 0)[1]
    assert (y, x) == (0, 1) and T.territory(7, 7, st, 0, y, x) == mine
    assert T.start_set(7, 7, st, 1, T._occupied(st)) == [(0, 5)]


def test_distances_by_a_queue():
    wall = {1 * 5 + x for x in range(4)}                      # row 1 closed but for a door at its east end
    d = T.distances(5, 5, wall, [(0, 0)])
    assert d[(0, 0)] == 0 and d[(0, 4)] == 4 and d[(1, 4)] == 5 and d[(2, 0)] == 10 and len(d) == 21
    d = T.distances(5, 5, wall, [(0, 0), (2, 0)])             # the nearest source counts
    assert d[(2, 0)] == 0 and d[(2, 4)] == 4 and d[(1, 4)] == 5
    assert T.distances(5, 5, wall, []) == {}                  # an empty start set reaches nothing
    assert (0, 0) not in T.distances(5, 5, wall | {1 * 5 + 4}, [(2, 2)])


# ---- a target inside a strong snake's start set --------------------------------------------------------------------------------------
def test_a_target_a_strong_snake_can_step_on_is_no_territory():
    """snake 0 (length 2) heads east at (3, 2), snake 1 (length 3) heads west at (3, 4): both can step on (3, 3).  Behind it snake 0
    is nowhere first -- every cell is as near to snake 1's start set, which holds the target itself -- so straight has territory 0;
    it is unsafe too, and what is left of the score is the food term: not -1, the move is not blocked"""
    st = R.board(7, 7, [([(3, 2), (3, 1)], 1), ([(3, 4), (3, 5), (3, 6)], 3)], food=[(0, 3)])
    q = T.scores(7, 7, st, 0)
    assert T.parts(q[1]) == (0, 0, 14 - 3, 0) and q[1] == 11 * 512 >= 0
    assert T.parts(R.scores(7, 7, st, 0)[1])[3] == 44
    assert T.parts(q[0])[3] > 0 and T.parts(q[2])[3] > 0 and R.move(q) != 1
    weak = R.board(7, 7, [([(3, 2), (3, 1), (3, 0)], 1), ([(3, 4), (3, 5)], 3)], food=[(0, 3)])        # the same against a shorter snake
    assert T.parts(T.scores(7, 7, weak, 0)[1])[3] > 0 and T.parts(T.scores(7, 7, weak, 1)[1])[3] == 0


# ---- hungry ----------------------------------------------------------------------------------------------------------------------------
def test_the_food_term_counts_from_the_hungry_threshold_down():
    st = R.board(7, 7, [([(3, 3), (4, 3), (5, 3)], 0), ([(6, 6), (6, 5)], 1)], food=[(3, 0), (0, 3)])
    st["health"][0] = 37
    at, below = T.scores(7, 7, st, 0, R.ALL, 37), T.scores(7, 7, st, 0, R.ALL, 36)
    foods = [12, 12, 10]                                      # tests/test_script_cpu.py's board D: worked out by hand there
    assert [a - b for a, b in zip(at, below)] == [f * 512 for f in foods]
    assert [T.parts(z)[2] for z in at] == foods and [T.parts(z)[2] for z in below] == [0, 0, 0]
    assert at == T.scores(7, 7, st, 0) == T.scores(7, 7, st, 0, R.ALL, 100)
    assert below == T.scores(7, 7, st, 0, R.ALL, 0) == T.scores(7, 7, st, 0, R.SPACE | R.HEADS)
    assert T.scores(7, 7, st, 1, R.ALL, 37) == T.scores(7, 7, st, 1, R.ALL, 89) != T.scores(7, 7, st, 1, R.ALL, 90)     # health 90


@pytest.mark.parametrize("flags", range(8))
def test_each_flag_subset(flags):
    st = corridor(6, 5)
    st["food"][0 * 7 + 4] = 1
    room, safe, food, fill = T.parts(T.scores(7, 7, st, 0, flags)[1])
    assert (room, fill) == ((3, 3) if flags & R.SPACE else (0, 0)) and safe == 1 and food == (14 - 3 if flags & R.FOOD else 0)
    heads = R.board(7, 7, [([(3, 2), (3, 1)], 1), ([(3, 4), (3, 5), (3, 6)], 3)])
    assert T.parts(T.scores(7, 7, heads, 0, flags)[1])[1] == (0 if flags & R.HEADS else 1)


# ---- a reading of the statement against the plain script ---------------------------------------------------------------------------
def test_the_statement_plays_the_plain_script_to_the_end():
    """RefTerritory() against RefScripted(), one snake each, on the sixteen recorded 7x7x2 start boards with the food of
    RandomState(47).  The counts pin the statement as it was first computed; they are no threshold of strength"""
    out = T.reference("duel-7x7x2")
    n = T.N_DUEL
    wins = sum(w == 0 for w in out["winners"])
    losses = sum(w == 1 for w in out["winners"])
    draws = sum(w is None for w in out["winners"])
    print(f"RefTerritory() v RefScripted() on {n} 7x7x2 boards: wins {wins}, draws {draws}, losses {losses}, {out['turns']} turns")
    assert wins + draws + losses == n == len(out["lengths"]) and out["turns"] == max(out["lengths"])
    assert (wins, draws, losses, out["turns"]) == PIN


PIN = (12, 0, 4, 85)                                  # wins, draws, losses of the territory side; turns of the longest game


# ---- the ABI and the Python layer (nothing is launched) -----------------------------------------------------------------------------
def test_the_entry_point_is_exported_with_its_prototype():
    import snake_engine
    from conftest import REPO
    from snake_engine import _lib
    L = snake_engine.lib()
    assert hasattr(L, "snk_pit_territory_values")
    restype, args = _lib.PROTOTYPES["snk_pit_territory_values"]
    assert len(args) == 7 and len(_lib.PROTOTYPES["snk_pit_script_values"][1]) == 6
    txt = open(os.path.join(REPO, "include", "snake_engine.h")).read()
    assert "int snk_pit_territory_values(const snk_engine *e, const int32_t *d_pairs, int m, uint32_t flags, int hungry, float *d_q," in txt
    assert "#define SNK_ABI_VERSION 113 " in txt and L.snk_version() == 113


def test_territory_is_a_scripted_with_its_refusals():
    from snake_engine.arena import Arena, Scripted, Searcher, Territory
    s = Territory()
    assert isinstance(s, Scripted) and not hasattr(s, "v_device") and vars(s) == {"flags": 7, "hungry": 100}
    t = Territory(5, 40)
    assert (t.flags, t.hungry) == (5, 40) and Territory(hungry=0).hungry == 0 and Territory(0).flags == 0
    for bad in (dict(flags=8), dict(hungry=101), dict(hungry=-1), dict(flags=-1)):
        with pytest.raises(ValueError):
            Territory(**bad)
    with pytest.raises(TypeError):
        Searcher(Territory())
    net = type("Net", (), {"v_device": lambda self, planes, mask: None})()
    a, b = Arena._sides(s, net, dict(breadth=8, depth=4), 3)
    assert a is s and isinstance(b, Searcher) and b.net is net


def test_the_tools_know_the_baseline_names():
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    for name in ("league.py", "search_pit.py", "script_time.py"):
        assert "Territory" in open(os.path.join(tools, name)).read(), name
