"""CPU tests of territory at the leaf: the statement (tests/leaf_ref.py) on recorded boards -- with the script as its row-scoring
function it is look_ref / deep_ref / playout_ref exactly, depth 1 is the lookahead, a lone snake's rows are RefTerritory's --, a
hand-built position on which the two leaves part, a whole match of the statement, the Python side's refusals, the tools' names and
the library's symbols.  No compute calls: there is no GPU here."""
import importlib.util
import os
import re

import numpy as np
import pytest

import deep_ref as D
import leaf_ref as F
import look_ref as K
import playout_ref as P
import script_ref as R
import territory_ref as T
from conftest import REPO

CFGS = ("7x7x2", "11x11x4_dec9")
HUNGRY = F.HUNGRY


def _terr(hungry, flags=R.ALL):
    return F.scorer(T.RefTerritory(flags, hungry))


# ---- 1. the identities of the statement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS)
def test_with_the_script_the_statement_is_the_three_statements_it_is_built_on(cfg):
    H, W, S, hd, boards = F.recorded(cfg)
    for flags in (R.ALL, R.SPACE | R.FOOD):
        for i, st in enumerate(boards):
            assert F.board_look_scores(H, W, S, hd, st, flags) == K.board_look_scores(H, W, S, hd, st, flags), (cfg, i)
    for i in F.deep_boards(cfg)[-3:] if cfg != "7x7x2" else F.deep_boards(cfg):          # 11x11x4: not the board with four alive
        assert F.board_deep_scores(H, W, S, hd, boards[i], 2) == D.board_deep_scores(H, W, S, hd, boards[i], 2), (cfg, i)
    for g, st in enumerate(boards[::4]):
        for eps in (0, 64):
            assert F.board_playout_scores(H, W, S, hd, st, g, 2, 3, eps, 5) == P.board_playout_scores(H, W, S, hd, st, g, 2, 3, eps, 5), (cfg, g)
    assert F.scorer(None) is F.scorer(R.RefScripted()) and F.leaf_args(None) == F.leaf_args(R.RefScripted(5)) == (0, 100)
    assert F.leaf_args(T.RefTerritory(hungry=HUNGRY)) == (1, HUNGRY)


@pytest.mark.parametrize("cfg", CFGS)
def test_depth_one_is_the_lookahead_and_only_restricts_the_rows(cfg):
    H, W, S, hd, boards = F.recorded(cfg)
    for hungry in (100, HUNGRY):
        look = F.look_scores(cfg, R.ALL, hungry)
        for i, st in enumerate(boards):
            assert F.board_deep_scores(H, W, S, hd, st, 1, R.ALL, _terr(hungry)) == look[i], (cfg, i)
    st = boards[0]
    whole = F.board_deep_scores(H, W, S, hd, st, 1, R.ALL, _terr(HUNGRY))
    assert F.board_deep_scores(H, W, S, hd, st, 1, R.ALL, _terr(HUNGRY), only=[1]) == {1: whole[1]}


@pytest.mark.parametrize("cfg", CFGS + ("19x19x8",))
def test_a_fallback_row_gets_the_territory_scores(cfg):
    """A < 2: the lookahead, the deep search and the playout give RefTerritory's scores; A > 4: the first two do, the playout
    plays on"""
    H, W, S, hd, boards = F.recorded(cfg)
    alive = [int(st["alive"].sum()) for st in boards]
    assert alive[-1] == 1 and (cfg != "19x19x8" or max(alive) > 4)
    seen = 0
    for g, st in enumerate(boards):
        if 2 <= alive[g] <= 4:
            continue
        seen += 1
        for hungry, flags in ((100, R.ALL), (HUNGRY, R.ALL), (HUNGRY, R.SPACE | R.FOOD)):
            want = T.board_scores(H, W, st, flags, hungry)
            assert len(want) == alive[g]
            assert F.board_look_scores(H, W, S, hd, st, flags, _terr(hungry, flags)) == want
            assert F.board_deep_scores(H, W, S, hd, st, 2, flags, _terr(hungry, flags)) == want
            if alive[g] < 2 or (seen == 1 and hungry == 100):     # above four alive: one board, one snake (8 snakes, 361 cells)
                s = min(want)
                got = F.board_playout_scores(H, W, S, hd, st, g, 2, 3, 64, 0, flags, _terr(hungry, flags), only=[s])
                assert (got == {s: want[s]}) == (alive[g] < 2)
    assert seen >= (3 if cfg == "19x19x8" else 1)


def test_the_threshold_and_the_leaf_change_scores_on_the_recorded_boards():
    """the recorded boards do tell the leaves and the thresholds apart (what the GPU test compares is not all the same numbers)"""
    for cfg in CFGS:
        script, full, hungry = F.look_scores(cfg), F.look_scores(cfg, R.ALL, 100), F.look_scores(cfg, R.ALL, HUNGRY)
        assert script != full and full != hungry
    H, W, S, hd, boards = F.recorded("11x11x4_dec9")
    healths = [int(st["health"][s]) for st in boards for s in range(S) if st["alive"][s]]
    assert min(healths) <= HUNGRY < max(healths) and hd == 9


# ---- 2. a position on which the leaves part -----------------------------------------------------------------------------------------
def test_the_territory_leaf_takes_the_move_that_is_not_cut_off():
    """7x7.  Snake 1 (length 3) has run east along row 5 into the edge: its head is on (5, 6), straight on leaves the board, left is
    north to (4, 6), right is south to (6, 6).  Snake 0 (length 5) comes down column 3 behind it, its head on (4, 3) heading south.
    Nobody having moved, both of snake 1's moves reach the same 41 free cells, so the script at the leaf scores them alike and the
    tie order takes the later move: south, into the bottom row.  But snake 0 is on (5, 3) after this tick and reaches every cell of
    rows 5 and 6 west of column 6 before snake 1 can turn round: south leaves one cell that snake 1 reaches first, less than its
    length -- it is cut off --, north leaves four.  The territory leaf sees that one tick deep; hungry does not matter, there is
    no food"""
    H = W = 7
    st = R.board(H, W, [([(4, 3), (3, 3), (3, 2), (4, 2), (4, 1)], 2), ([(5, 6), (5, 5), (5, 4)], 1)])
    length = int(st["length"][1])
    plain = F.board_look_scores(H, W, 2, 1, st)[1]
    assert K.board_look_scores(H, W, 2, 1, st)[1] == plain
    assert plain[1] < -1 and plain[0] == plain[2] > 0 and T.parts(plain[0])[3] == 41 and R.move(plain) == 2       # south
    for hungry in (100, HUNGRY):
        terr = F.board_look_scores(H, W, 2, 1, st, R.ALL, _terr(hungry))[1]
        assert R.move(terr) == 0 and terr[1] == plain[1]                                                         # north
        north, south = T.parts(terr[0]), T.parts(terr[2])
        assert north[0] == length and north[3] == 4 and south[0] == south[3] == 1 < length
    # the same read off the children themselves: after the move, whatever snake 0 replies, the best territory left to snake 1
    children, alive = K.child_boards(H, W, 2, 1, st)
    assert alive == [0, 1]
    left = {a: [max(t for t in T.territories(H, W, c, 1) if t is not None) for j, c in enumerate(children)
                if j // 3 == a and c["alive"][0] and c["alive"][1]] for a in (0, 2)}
    assert min(left[0]) == 4 >= length > max(left[2]) == 1 and len(left[0]) == len(left[2]) == 2


# ---- 3. a whole match of the statement ------------------------------------------------------------------------------------------------
def test_deep_over_territory_against_territory_plays_to_the_end():
    """RefDeep(2, leaf = territory, hungry 40) against RefTerritory(hungry=40) on the sixteen 7x7x2 start boards: the match ends,
    and every move of every turn is a move of a snake that was alive, 0, 1 or 2.  (Who wins is a reading)"""
    want = F.reference("deep-7x7x2")
    n = F.N_DUEL
    assert want["open"] == [] and len(want["winners"]) == n and max(want["lengths"]) == want["turns"] == len(want["moves"])
    assert all(1 <= length <= want["turns"] for length in want["lengths"])
    for turn, (dense, rows) in enumerate(zip(want["moves"], want["counts"])):
        assert rows[0] == rows[1] == len(dense) > 0               # a duel: both sides move in every open game
        for g, mv in dense.items():
            assert want["lengths"][g] > turn and mv.shape == (2,) and set(mv.tolist()) <= {0, 1, 2}
    assert all(w in (None, 0, 1) for w in want["winner_owner"])
    for st in want["boards"]:
        assert int(st["alive"].sum()) <= 1


# ---- 4. the Python side ---------------------------------------------------------------------------------------------------------------
def test_the_leaf_keyword_of_the_three_players():
    from snake_engine import arena as A
    terr = A.Territory(hungry=HUNGRY)
    for make in (A.Lookahead, lambda **kw: A.Deep(depth=2, **kw), lambda **kw: A.Playout(playouts=2, horizon=3, **kw)):
        assert make().leaf is None and make(leaf=None).leaf is None and make(leaf=A.Scripted()).leaf is None
        side = make(leaf=terr)
        assert side.leaf is terr and side.leaf.hungry == HUNGRY and side.flags == terr.flags == 7
        assert isinstance(side, A.Scripted) and not hasattr(side, "v_device")
        with pytest.raises(TypeError):
            A.Searcher(side)
        assert make(flags=5, leaf=A.Territory(5)).leaf.flags == 5
        for bad in (A.Lookahead(), A.Deep(), A.Playout(), make(leaf=terr), object(), 7, "terr", A.Territory):
            with pytest.raises(TypeError):
                make(leaf=bad)

        class Mine(A.Territory):
            pass
        with pytest.raises(TypeError):
            make(leaf=Mine())
        with pytest.raises(ValueError, match="flags"):
            make(flags=5, leaf=terr)
        with pytest.raises(ValueError, match="flags"):
            make(leaf=A.Scripted(5))
        with pytest.raises(ValueError):
            make(flags=8, leaf=terr)
    with pytest.raises(ValueError, match="hungry"):
        A.Lookahead(leaf=A.Territory(hungry=101))
    assert (A.LEAF_SCRIPT, A.LEAF_TERRITORY) == (F.LEAF_SCRIPT, F.LEAF_TERRITORY) == (0, 1)


def test_the_league_needs_no_word_about_leaves():
    """snake_engine/league.py takes a territory-leaf player as the Scripted it is: it does not name the leaf, and the one dispatch
    of mixed_values is isinstance(side, Scripted)"""
    import inspect
    from snake_engine import arena as A
    pkg = os.path.join(REPO, "alphasnake-zero_amd", "snake_engine")
    assert "leaf" not in open(os.path.join(pkg, "league.py")).read().lower()
    src = inspect.getsource(A.mixed_values)
    assert src.count("isinstance(sides[o], Scripted)") == 1 and "leaf" not in src


# ---- 5. the tools and the library -----------------------------------------------------------------------------------------------------
def test_the_baseline_names():
    tools = os.path.join(REPO, "tools")
    import sys
    sys.path.insert(0, tools)
    try:
        spec = importlib.util.spec_from_file_location("leaf_names", os.path.join(tools, "leaf_names.py"))
        names = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(names)
    finally:
        sys.path.remove(tools)
    assert names.parse("lookt") == ("look", {}, 100) and names.parse("lookth40") == ("look", {}, 40)
    assert names.parse("deep2t") == ("deep", dict(depth=2), 100) and names.parse("deep3t") == ("deep", dict(depth=3), 100)
    assert names.parse("deep2th40") == ("deep", dict(depth=2), 40)
    assert names.parse("playt") == ("play", {}, 100) and names.parse("playth40") == ("play", {}, 40)
    assert names.parse("play8x16th0") == ("play", dict(playouts=8, horizon=16), 0)
    for other in ("look", "look5", "deep2", "play", "play8x16", "terr", "terrh40", "7", "lookth101", "deept", "lookt5", "t"):
        assert names.parse(other) is None, other
    from snake_engine import arena as A
    side = names.player("deep2th40", A)
    assert type(side) is A.Deep and side.depth == 2 and type(side.leaf) is A.Territory and side.leaf.hungry == 40
    side = names.player("play4x6t", A)
    assert type(side) is A.Playout and (side.playouts, side.horizon, side.leaf.hungry) == (4, 6, 100)
    assert type(names.player("lookt", A)) is A.Lookahead and names.player("look", A) is None
    for tool in ("league.py", "search_pit.py", "script_time.py"):
        assert "leaf_names" in open(os.path.join(tools, tool)).read(), tool


def test_the_three_entry_points_are_declared_exported_and_bound():
    import snake_engine
    from snake_engine import _lib
    header = open(os.path.join(REPO, "include", "snake_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = snake_engine.lib()
    for name, args in (("snk_pit_look_values_leaf", 10), ("snk_pit_deep_values_leaf", 11), ("snk_pit_playout_values_leaf", 14)):
        decl = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", code)
        assert decl and decl.group(1).count(",") + 1 == args == len(_lib.PROTOTYPES[name][1]), name
        assert "int leaf, int hungry" in " ".join(decl.group(1).split())
        assert hasattr(L, name)
        old = name[:-len("_leaf")]
        assert len(_lib.PROTOTYPES[old][1]) == args - 2 and re.search(r"\bint " + old + r"\s*\(", code)
    assert "#define SNK_LEAF_SCRIPT 0" in code and "#define SNK_LEAF_TERRITORY 1" in code
    assert L.snk_version() == _lib.ABI_VERSION == 113 and "#define SNK_ABI_VERSION 113" in code
    # a refusal needs no device: the leaf and hungry are asked before anything is touched
    for call in (lambda leaf, hungry: L.snk_pit_look_values_leaf(None, None, None, 0, 7, leaf, hungry, None, None, None),
                 lambda leaf, hungry: L.snk_pit_deep_values_leaf(None, None, 1, None, 0, 7, leaf, hungry, None, None, None),
                 lambda leaf, hungry: L.snk_pit_playout_values_leaf(None, None, None, 0, 7, leaf, hungry, 2, 3, 64, 0, None, None, None)):
        for leaf, hungry in ((2, 100), (-1, 100), (0, 40), (1, 101), (1, -1)):
            assert call(leaf, hungry) == -1 and b"leaf=" in L.snk_last_error() and b"_leaf" in L.snk_last_error()
        assert call(1, 40) == -1 and b"NULL" in L.snk_last_error()


def test_a_refusal_names_the_leaf_entry_point_it_came_through():
    """the six search entry points with a valid leaf and a NULL engine at m = 0: each is refused, and the message starts with the
    name of its own _leaf entry point -- the plain ones forward to it -- whichever body the refusal is written in.  No device:
    the call returns before any HIP call"""
    import snake_engine
    L = snake_engine.lib()
    calls = {"snk_pit_look_values": lambda: L.snk_pit_look_values(None, None, None, 0, 7, None, None, None),
             "snk_pit_look_values_leaf": lambda: L.snk_pit_look_values_leaf(None, None, None, 0, 7, 1, 40, None, None, None),
             "snk_pit_deep_values": lambda: L.snk_pit_deep_values(None, None, 1, None, 0, 7, None, None, None),
             "snk_pit_deep_values_leaf": lambda: L.snk_pit_deep_values_leaf(None, None, 1, None, 0, 7, 1, 40, None, None, None),
             "snk_pit_playout_values": lambda: L.snk_pit_playout_values(None, None, None, 0, 7, 2, 3, 64, 0, None, None, None),
             "snk_pit_playout_values_leaf": lambda: L.snk_pit_playout_values_leaf(None, None, None, 0, 7, 1, 40, 2, 3, 64, 0, None, None,
                                                                                  None)}
    for name, call in calls.items():
        leaf_name = name if name.endswith("_leaf") else name + "_leaf"
        assert call() == -1, name
        assert L.snk_last_error().startswith(leaf_name.encode() + b":"), (name, L.snk_last_error())
