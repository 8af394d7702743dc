"""CPU tests of the pit's tally: the statement (tests/tally_ref.py) on every tick of the golden trajectories and corner cases the
unmodified reference recorded -- its deaths are the snakes that were alive before and not after, its counts per cause are the
differences of the reference's own counters, its food and lengths the reference's --, on hand-built ticks where the order of the
tests decides, Tally.by_owner / games / text on hand-made arrays, and the C ABI's declaration, binding, refusals and n = 0 no-op
(none of which reaches a device)."""
import os
import re

import numpy as np
import pytest

import script_ref as SC
import tally_ref as TR
from conftest import REPO, golden_state, load_golden
from snake_engine.tally import FATES       # the statement is the statement of this module: without it there is nothing to state

GOLDEN = ["5x5x2", "7x7x2", "9x9x3", "11x11x4", "11x11x4_dec9", "15x15x5", "16x16x6", "19x19x8"]


def golden_arrays(name):
    """a golden file with every array read once (the file object reads an array anew each time it is indexed)"""
    z = load_golden(name)
    return {k: z[k] for k in z.files}


# ---- 1. every recorded tick of the reference ------------------------------------------------------------------------------------
def check_tick(H, W, hd, pre, dense, post, what):
    """the four properties of one recorded tick; returns the fates"""
    got = TR.tick_fates(H, W, hd, pre, dense)
    assert got is not None, f"{what}: the reference ticked a board with fewer than two snakes alive"
    fate, eats, length = got
    before, after = np.asarray(pre["alive"]).astype(bool), np.asarray(post["alive"]).astype(bool)
    assert ((fate > 0) == (before & ~after)).all(), f"{what}: the dead are the snakes alive before and not after"
    assert not (after & ~before).any()
    delta = np.asarray(post["counters"]).astype(np.int64) - np.asarray(pre["counters"]).astype(np.int64)
    for code in (TR.WALL, TR.BODY, TR.HEAD, TR.STARVED):
        assert int((fate == code).sum()) == delta[code - 1], f"{what}: {TR.FATES[code]} deaths against the counters"
    assert int(eats.sum()) == delta[4], f"{what}: food eaten"
    assert delta[5] == 1
    assert (length[after] == np.asarray(post["length"])[after]).all(), f"{what}: a survivor's length"
    assert (length[~before] == 0).all() and (eats[~before] == 0).all()
    return fate


@pytest.mark.parametrize("cfg", GOLDEN)
def test_every_tick_of_the_golden_trajectories(cfg):
    z = golden_arrays(f"tic_{cfg}.npz")
    H, W, S, hd = int(z["H"]), int(z["W"]), int(z["S"]), int(z["health_dec"])
    ptr = z["ptr"]
    tick, seen = 0, np.zeros(5, np.int64)
    for g in range(len(ptr) - 1):
        for t in range(ptr[g + 1] - ptr[g] - 1):
            fate = check_tick(H, W, hd, golden_state(z, ptr[g] + t), z["moves"][tick], golden_state(z, ptr[g] + t + 1),
                              f"{cfg} game {g} tick {t}")
            seen += np.bincount(fate, minlength=5)
            tick += 1
    assert tick == len(z["moves"]) >= 50
    assert seen[1:].sum() >= 1, "a trajectory without a death checks nothing"


def test_every_tick_of_the_corner_cases():
    z = golden_arrays("corner.npz")
    ticks, seen = 0, np.zeros(5, np.int64)
    for i, name in enumerate(z["names"]):
        p = f"c{i}_"
        H, W, S, hd = (int(v) for v in z[p + "meta"])
        for t in range(len(z[p + "moves"])):
            fate = check_tick(H, W, hd, golden_state(z, t, p + "st_"), z[p + "moves"][t], golden_state(z, t + 1, p + "st_"),
                              f"{name} tick {t}")
            seen += np.bincount(fate, minlength=5)
            ticks += 1
    assert ticks >= len(z["names"]) >= 20
    assert (seen[1:] > 0).all(), "the corner cases hold every cause of death"


# ---- 2. hand-built ticks where the order of the tests matters ---------------------------------------------------------------------
H = W = 7


def _far():
    """a bystander that keeps the game going: it walks along the bottom row, from (6, 5) to (6, 4)"""
    return ([(6, 5), (6, 6)], 3)


def _case(snakes, moves, fate, eats, length, food=(), health=None, dead=()):
    st = SC.board(H, W, snakes, food, dead)
    for s, h in (health or {}).items():
        st["health"][s] = h
    return dict(board=st, moves=np.array(moves, np.uint8), fate=fate, eats=eats, length=length)


# headings: 0 = y-1, 1 = x+1, 2 = y+1, 3 = x-1; move 1 is straight on, 0 a left turn, 2 a right turn.  fate / eats / length: what
# the tick gives every snake id, worked out by hand from game.py:87-165
CASES = {
    # two heads leave the board side by side.  An off-board head has no cell, and a kernel that keeps "none" as one value for both
    # must not read two of them as one shared cell: wall for both, not head-on, though their lengths are equal
    "two-off-board": _case([([(0, 2), (1, 2)], 0), ([(0, 3), (1, 3)], 0), _far()], [1, 1, 1],
                           fate=[1, 1, 0], eats=[0, 0, 0], length=[2, 2, 2]),
    # an off-board head whose cell index would wrap onto another head: snake 0 leaves row 3 to the right, (3, 7), which as
    # y * W + x is the cell (4, 0) that snake 1 enters.  Wall for snake 0, and snake 1 has the cell to itself
    "off-board-would-be-head-on": _case([([(3, 6), (3, 5)], 1), ([(5, 0), (6, 0)], 0), _far()], [1, 1, 1],
                                        fate=[1, 0, 0], eats=[0, 0, 0], length=[2, 2, 2]),
    # snakes 0 and 1 both enter (2, 4), a body cell of snake 2: body for both, not head-on, though their lengths differ
    "two-heads-into-a-body": _case([([(2, 3), (2, 2)], 1), ([(2, 5), (2, 6), (1, 6)], 3), ([(1, 4), (2, 4), (3, 4)], 0)], [1, 1, 1],
                                   fate=[2, 2, 0], eats=[0, 0, 0], length=[2, 3, 3]),
    # equal lengths on one cell: both die
    "head-on-equal": _case([([(3, 2), (3, 1)], 1), ([(3, 4), (3, 5)], 3), _far()], [1, 1, 1],
                           fate=[3, 3, 0], eats=[0, 0, 0], length=[2, 2, 2]),
    # unequal: the shorter one only
    "head-on-unequal": _case([([(3, 2), (3, 1)], 1), ([(3, 4), (3, 5), (3, 6)], 3), _far()], [1, 1, 1],
                             fate=[3, 0, 0], eats=[0, 0, 0], length=[2, 3, 2]),
    # three on one cell, lengths 2, 3, 3: nobody is strictly the longest, all die
    "head-on-three": _case([([(3, 2), (3, 1)], 1), ([(3, 4), (3, 5), (3, 6)], 3), ([(2, 3), (1, 3), (0, 3)], 2)], [1, 1, 1],
                           fate=[3, 3, 3], eats=[0, 0, 0], length=[2, 3, 3]),
    # equal lengths and food on the cell: the lower id eats, is the longer one from then on and survives
    "head-on-first-ate": _case([([(3, 2), (3, 1)], 1), ([(3, 4), (3, 5)], 3), _far()], [1, 1, 1], food=[(3, 3)],
                               fate=[0, 3, 0], eats=[1, 0, 0], length=[3, 2, 2]),
    # the same with the longer snake on the higher id: snake 0 eats and draws level, both die; the food is eaten all the same
    "head-on-ate-and-drew-level": _case([([(3, 2), (3, 1)], 1), ([(3, 4), (3, 5), (3, 6)], 3), _far()], [1, 1, 1], food=[(3, 3)],
                                        fate=[3, 3, 0], eats=[1, 0, 0], length=[3, 3, 2]),
    # health 1 going onto a food cell: health is 100 again before the starvation test.  Snake 1 with health 1 and no food starves
    "starving-on-food": _case([([(3, 3), (3, 2)], 1), ([(0, 0), (0, 1)], 2), _far()], [1, 1, 1], food=[(3, 4)], health={0: 1, 1: 1},
                              fate=[0, 4, 0], eats=[1, 0, 0], length=[3, 2, 2]),
    # a head-on survivor with no health left is not tested for starvation (the elif chain of game.py:156-163)
    "head-on-survivor-skips-starvation": _case([([(3, 2), (3, 1)], 1), ([(3, 4), (3, 5), (3, 6)], 3), _far()], [1, 1, 1],
                                               health={1: 1}, fate=[3, 0, 0], eats=[0, 0, 0], length=[2, 3, 2]),
    # snake 0 has just eaten: its tail (3, 1) is doubled, so this tick's pop leaves the cell a body cell; snake 1 enters it
    "doubled-tail-entered": _case([([(3, 3), (3, 2), (3, 1), (3, 1)], 1), ([(4, 1), (5, 1)], 0), _far()], [1, 1, 1],
                                  fate=[0, 2, 0], eats=[0, 0, 0], length=[4, 2, 2]),
    # the same without the doubling: the tail leaves (3, 1) on this tick and snake 1 lives there
    "tail-cell-just-left": _case([([(3, 3), (3, 2), (3, 1)], 1), ([(4, 1), (5, 1)], 0), _far()], [1, 1, 1],
                                 fate=[0, 0, 0], eats=[0, 0, 0], length=[3, 2, 2]),
    # a length-5 snake, curled up, turns right into its own fourth node
    "own-body": _case([([(3, 3), (3, 4), (2, 4), (2, 3), (2, 2)], 3), _far()], [2, 1],
                      fate=[2, 0], eats=[0, 0], length=[5, 2]),
    # a dead snake's stale nodes are no body cells and its stale head is no head: snake 0 walks over them
    "dead-snake-is-no-obstacle": _case([([(3, 2), (3, 1)], 1), ([(3, 3), (3, 4)], 3), _far()], [1, 1, 1], dead=[1],
                                       fate=[0, 0, 0], eats=[0, 0, 0], length=[2, 0, 2]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_hand_built_ticks(name, oracle):
    case = CASES[name]
    fate, eats, length = TR.tick_fates(H, W, 1, case["board"], case["moves"])
    assert fate.tolist() == case["fate"], f"{name}: fates"
    assert eats.tolist() == case["eats"], f"{name}: eats"
    assert length.tolist() == case["length"], f"{name}: lengths"
    # and the reference's own tick (the C transcription the goldens pin) kills the same snakes
    game = oracle.Game.from_compact(H, W, len(case["moves"]), 1, 0.0, case["board"])
    game.tic(case["moves"])
    post = game.compact()
    assert ((np.array(case["fate"]) > 0) == (case["board"]["alive"].astype(bool) & ~post["alive"].astype(bool))).all(), name
    delta = post["counters"].astype(np.int64) - case["board"]["counters"].astype(np.int64)
    assert [int((fate == c).sum()) for c in (1, 2, 3, 4)] == delta[:4].tolist() and int(eats.sum()) == delta[4], name


def test_a_board_that_stands_still_has_no_fates():
    st = SC.board(H, W, [([(3, 3), (3, 2)], 1), ([(0, 0), (0, 1)], 1)], dead=[1])
    assert TR.tick_fates(H, W, 1, st, np.array([1, 1], np.uint8)) is None


# ---- 3. Tally on hand-made arrays ------------------------------------------------------------------------------------------------------
def _tally():
    """three games of three seats, two owners and a third that holds no seat"""
    from snake_engine.tally import Tally
    fate = [[1, 0, 3], [2, 4, 0], [0, 3, 3]]
    died = [[2, 0, 5], [1, 7, 0], [0, 4, 4]]
    food = [[0, 2, 1], [0, 3, 4], [1, 0, 0]]
    length = [[3, 5, 4], [3, 6, 7], [4, 3, 3]]
    owners = [[0, 1, 1], [1, 0, 0], [0, 0, 1]]
    return Tally.from_arrays(fate, died, food, length, owners, 3, [5, 9, 4])


def test_by_owner_counts_every_seat_once():
    from snake_engine.tally import TallyRows
    assert FATES == ("alive", "wall", "body", "head", "starved") == TR.FATES
    t = _tally()
    assert all(a.dtype == np.int32 and a.shape == (3, 3) for a in (t.fate, t.died, t.food, t.length))
    rows = t.by_owner()
    assert isinstance(rows, TallyRows) and rows._fields == ("seats", "fates", "food", "length", "turns")
    # owner 0 holds (0,0) wall@2, (1,1) starved@7, (1,2) alive (game length 9), (2,0) alive (4), (2,1) head@4
    # owner 1 holds (0,1) alive (5), (0,2) head@5, (1,0) body@1, (2,2) head@4
    assert rows.seats.tolist() == [5, 4, 0]
    assert rows.fates.tolist() == [[2, 1, 0, 1, 1], [1, 0, 1, 2, 0], [0, 0, 0, 0, 0]]
    assert rows.food.tolist() == [0 + 3 + 4 + 1 + 0, 2 + 1 + 0 + 0, 0]
    assert rows.length[:2].tolist() == [(3 + 6 + 7 + 4 + 3) / 5, (5 + 4 + 3 + 3) / 4]
    assert rows.turns[:2].tolist() == [(2 + 7 + 9 + 4 + 4) / 5, (5 + 5 + 1 + 4) / 4]
    assert np.isnan(rows.length[2]) and np.isnan(rows.turns[2])
    assert rows.fates.sum() == 9 and (rows.fates.sum(axis=1) == rows.seats).all()


def test_games_by_owner_and_fate():
    t = _tally()
    assert t.games().tolist() == [0, 1, 2]
    assert t.games(fate="head").tolist() == [0, 2] == t.games(fate=3).tolist()
    assert t.games(owner=0, fate="head").tolist() == [2]
    assert t.games(owner=1, fate="head").tolist() == [0, 2]
    assert t.games(owner=1, fate="starved").tolist() == []
    assert t.games(owner=0, fate="alive").tolist() == [1, 2]
    assert t.games(owner=2).tolist() == [] and t.games(owner=1).tolist() == [0, 1, 2]
    assert t.games(fate="wall").dtype.kind == "i"
    for bad in ("eaten", 5, -1, 1.5, True):
        with pytest.raises(ValueError):
            t.games(fate=bad)
    with pytest.raises(ValueError):
        t.games(owner=3)


def test_text_is_a_line_per_side():
    t = _tally()
    lines = t.text(["gen0", "scripted", "nobody"]).splitlines()
    assert len(lines) == 4
    assert lines[0].split() == ["side", "seats", "alive", "wall", "body", "head", "starved", "food", "length", "turns"]
    assert lines[1].split() == ["gen0", "5", "2", "1", "0", "1", "1", "8", "4.60", "5.2"]
    assert lines[2].split() == ["scripted", "4", "1", "0", "1", "2", "0", "3", "3.75", "3.8"]
    assert lines[3].split() == ["nobody", "0", "0", "0", "0", "0", "0", "0", "nan", "nan"]
    assert t.text().splitlines()[1].split()[0] == "0"
    with pytest.raises(ValueError):
        t.text(["a", "b"])


def test_a_tally_is_empty_until_its_match_is_played_and_checks_its_shapes():
    from snake_engine.arena import Arena
    from snake_engine.league import League
    from snake_engine.tally import Tally
    for cls in (Arena, League):
        host = cls.__new__(cls)                                        # without an engine: tally() must not need one
        host.game_cnt, host.snake_cnt, host._tallier = 6, 4, None
        t = host.tally()
        assert isinstance(t, Tally) and host._tallier is t and (t.game_cnt, t.snake_cnt) == (6, 4) and t.fate is None
        for read in (t.by_owner, t.games, t.text):
            with pytest.raises(RuntimeError):
                read()
    z = np.zeros((2, 3), np.int32)
    with pytest.raises(ValueError):
        Tally.from_arrays(z, z, z, z, np.zeros((2, 2), np.uint8), 1, [1, 1])
    with pytest.raises(ValueError):
        Tally.from_arrays(z, z, z, z, np.full((2, 3), 2, np.uint8), 2, [1, 1])
    with pytest.raises(ValueError):
        Tally.from_arrays(z, z, z, z, np.zeros((2, 3), np.uint8), 1, [1, 1, 1])


def test_the_owner_hooks():
    """Arena: snakes 0 .. a_cnt-1 are team A's (owner 0); League: the checked table itself"""
    from snake_engine.arena import Arena
    from snake_engine.league import League
    arena = Arena.__new__(Arena)
    arena.game_cnt, arena.snake_cnt = 3, 4
    for a_cnt in (0, 1, 2, 4):
        own = arena._owners((a_cnt, None, None))
        assert own.dtype == np.uint8 and own.shape == (3, 4) and (own == (np.arange(4) >= a_cnt)[None, :]).all()
    table = np.arange(12, dtype=np.uint8).reshape(3, 4) % 5
    assert League._owners(League.__new__(League), (None, 5, None, 5, 0, None, table)) is table


# ---- 4. the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_entry():
    from snake_engine import _lib
    header = open(os.path.join(REPO, "include", "snake_engine.h")).read()
    assert re.search(r"#define SNK_ABI_VERSION 113\b", header) and _lib.ABI_VERSION == 113
    comment = header[header.index("#define SNK_ABI_VERSION"):header.index("int snk_version(void);")]
    L = _lib.lib()
    assert L.snk_version() == 113
    assert re.search(r"\bint snk_pit_tally\(", header), "snk_pit_tally is not declared"
    assert "snk_pit_tally" in comment, "snk_pit_tally is missing from the list of what was added under 113"
    res, args = _lib.PROTOTYPES["snk_pit_tally"]
    fn = L.snk_pit_tally
    assert fn.restype is res and list(fn.argtypes) == args and len(args) == 10
    section = header[header.index("the tally of a pit match"):header.index("int snk_pit_tally(")]
    for lines in ("game.py:90-165", "game.py:92", "game.py:121-127", "game.py:147-165", "game.py:354-356"):
        assert lines in section


def test_refusals_and_the_no_op_without_a_device():
    """n = 0 returns before anything is looked at; a negative n and NULL arrays are refused with a message -- no engine, no buffer
    and no device exists here, so none of these calls can have launched anything"""
    from snake_engine import lib
    L = lib()
    assert L.snk_pit_tally(None, None, 0, None, 1, None, None, None, None, None) == 0
    for n, word in ((-1, "n=-1"), (-300, "n=-300"), (1, "NULL"), (5, "NULL")):
        assert L.snk_pit_tally(None, None, n, None, 1, None, None, None, None, None) == -1
        assert word in L.snk_last_error().decode()
