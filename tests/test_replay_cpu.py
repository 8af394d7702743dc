"""CPU tests of the replay recorder: the statement (tests/replay_ref.py) against the text the unmodified reference recorded
(tests/golden/replay.npz) and on hand-built boards asserted cell by cell, the C ABI's declarations, bindings, refusals and r = 0
no-op (none of which reaches a device), the index checks of Arena.record / League.record, and Replay.text's form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import replay_ref as RR
import script_ref as SC
from conftest import REPO, load_golden

KEYS = ("alive", "health", "length", "dir", "nodes", "food", "rewards", "counters")
ENTRIES = ("snk_pit_record_stride", "snk_pit_record_slots", "snk_pit_record_moves", "snk_pit_record_boards")


# ---- 1. the reference's recorded text -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1])
def test_the_statement_gives_the_recorded_reference_text(ci, oracle):
    z = load_golden("replay.npz")
    p = f"r{ci}_"
    H, W, S, hd = (int(v) for v in z[p + "meta"])
    game = RR.Recording(oracle.Game.from_compact(H, W, S, hd, 0.15, {k: z[p + "init_" + k][0] for k in KEYS}))
    ticks = 0
    for t in range(len(z[p + "moves"])):
        ticks += 1
        if game.tic(z[p + "moves"][t][0], spawn_cell=int(z[p + "spawn"][t][0])):
            break
    want = z[p + "text"].tobytes()
    assert len(game.frames) == 2 * ticks and ticks >= 10
    assert RR.text(game.frames) == want
    assert want.count(b"\n\n") == 2 * ticks


# ---- 2. hand-built boards -------------------------------------------------------------------------------------------------------
H = W = 7          # 49 cells: no multiple of four


def _far():
    """a bystander that keeps the game going: it walks along the bottom row, from (6, 5) to (6, 4)"""
    return ([(6, 5), (6, 6)], 3)


def _case(snakes, moves, food=(), spawn=-1, dead=(), mid=None, post=None):
    return dict(board=SC.board(H, W, snakes, food, dead), moves=np.array(moves, np.uint8), spawn=spawn, mid=mid, post=post)


# every case: the cells of both frames that are not 0, worked out by hand.  Headings: 0 = y-1, 1 = x+1, 2 = y+1, 3 = x-1; move 1
# is straight on, 0 a left turn, 2 a right turn
CASES = {
    # snake 0 (length 2) and snake 1 (length 3) both enter (3, 3): the longer one is drawn last; the shorter one dies
    "heads-unequal": _case([([(3, 2), (3, 1)], 1), ([(3, 4), (3, 5), (3, 6)], 3)], [1, 1],
                           mid={(3, 3): -2, (3, 2): 1, (3, 4): 2, (3, 5): 2}, post={(3, 3): -2, (3, 4): 2, (3, 5): 2}),
    # the same with the lengths swapped: now the lower id is the longer snake and stays visible
    "heads-unequal-swapped": _case([([(3, 2), (3, 1), (3, 0)], 1), ([(3, 4), (3, 5)], 3)], [1, 1],
                                   mid={(3, 3): -1, (3, 2): 1, (3, 1): 1, (3, 4): 2}, post={(3, 3): -1, (3, 2): 1, (3, 1): 1}),
    # equal lengths: the stable sort leaves the higher id last; both die
    "heads-equal": _case([([(3, 2), (3, 1)], 1), ([(3, 4), (3, 5)], 3)], [1, 1],
                         mid={(3, 3): -2, (3, 2): 1, (3, 4): 2}, post={}),
    # equal lengths and food on the cell: snake 0 eats first, is the longer one from then on, is drawn last and survives
    "head-on-first-ate": _case([([(3, 2), (3, 1)], 1), ([(3, 4), (3, 5)], 3)], [1, 1], food=[(3, 3)],
                               mid={(3, 3): -1, (3, 2): 1, (3, 4): 2}, post={(3, 3): -1, (3, 2): 1}),
    # snake 0 runs into snake 1's body: the body is drawn over the head; snake 0 is in the mid board and gone from the post board
    "head-into-body": _case([([(2, 3), (2, 2)], 1), ([(1, 4), (2, 4), (3, 4)], 0)], [1, 1],
                            mid={(2, 4): 2, (2, 3): 1, (0, 4): -2, (1, 4): 2}, post={(0, 4): -2, (1, 4): 2, (2, 4): 2}),
    # a head off every edge: not drawn, and not wrapped into a neighbouring row either; the old heads are bodies
    "four-edges": _case([([(0, 1), (1, 1)], 0), ([(1, 6), (1, 5)], 1), ([(6, 5), (5, 5)], 2), ([(5, 0), (5, 1)], 3)], [1, 1, 1, 1],
                        mid={(0, 1): 1, (1, 6): 2, (6, 5): 3, (5, 0): 4}, post={}),
    # a snake that has just eaten (its tail doubled) turns left, beside a dead snake's stale nodes and a bystander
    "doubled-tail": _case([([(3, 3), (3, 2), (3, 2)], 1), ([(0, 0), (0, 1)], 1), _far()], [0, 1, 1], dead=[1],
                          mid={(2, 3): -1, (3, 3): 1, (3, 2): 1, (6, 4): -3, (6, 5): 3},
                          post={(2, 3): -1, (3, 3): 1, (3, 2): 1, (6, 4): -3, (6, 5): 3}),
    # food spawned this tick is in both boards; food that stays stays; a snake eats and its post-state tail is doubled
    "spawned-food": _case([([(3, 3), (3, 2)], 1), _far()], [1, 1], food=[(3, 4), (0, 6)], spawn=0,
                          mid={(0, 0): 9, (0, 6): 9, (3, 4): -1, (3, 3): 1, (6, 4): -2, (6, 5): 2},
                          post={(0, 0): 9, (0, 6): 9, (3, 4): -1, (3, 3): 1, (6, 4): -2, (6, 5): 2}),
    # one snake left and the live flag still set: the step leaves the game alone and both frames show it as it stands
    "not-moved": _case([([(3, 3), (3, 2)], 1), ([(0, 0), (0, 1)], 1)], [1, 1], food=[(5, 5)], dead=[1],
                       mid={(3, 3): -1, (3, 2): 1, (5, 5): 9}, post={(3, 3): -1, (3, 2): 1, (5, 5): 9}),
}


def frame_of(cells):
    out = np.zeros((H, W), np.int8)
    for (y, x), v in cells.items():
        out[y, x] = v
    return out


def post_state(case):
    """the board after the tick, by the oracle; a game with fewer than two snakes alive is not ticked (the engine leaves it)"""
    from oracle import snake_oracle
    if int(case["board"]["alive"].sum()) < 2:
        return case["board"]
    game = snake_oracle.Game.from_compact(H, W, len(case["moves"]), 1, 0.15, case["board"])
    game.tic(case["moves"], spawn_cell=case["spawn"])
    return game.compact()


@pytest.mark.parametrize("name", list(CASES))
def test_hand_built_boards_cell_by_cell(name, oracle):
    case = CASES[name]
    post = post_state(case)
    mid_f, post_f = RR.tick_frames(H, W, case["board"], case["moves"], post)
    for got, want, which in ((mid_f, frame_of(case["mid"]), "mid"), (post_f, frame_of(case["post"]), "post")):
        for y in range(H):
            for x in range(W):
                assert got[y, x] == want[y, x], f"{name}: cell ({y}, {x}) of the {which}-tick board"
    if name == "head-into-body":
        assert not post["alive"][0] and mid_f[2, 3] == 1 and post_f[2, 3] == 0
    if name == "spawned-food":
        assert post["length"][0] == 3 and post["nodes"][0][1] == post["nodes"][0][2]


# ---- 3. the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_entries():
    from snake_engine import _lib
    header = open(os.path.join(REPO, "include", "snake_engine.h")).read()
    assert re.search(r"#define SNK_ABI_VERSION 113\b", header) and _lib.ABI_VERSION == 113
    comment = header[header.index("#define SNK_ABI_VERSION"):header.index("int snk_version(void);")]
    L = _lib.lib()
    assert L.snk_version() == 113
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), f"{name} is not declared"
        assert name in comment, f"{name} is missing from the list of what was added under 113"
        res, args = _lib.PROTOTYPES[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args and len(args) >= 2
    section = header[header.index("replays of chosen games"):header.index("int snk_pit_record_stride")]
    for lines in ("game.py:281-300", "game.py:140-141", "194-195", "game.py:121-127"):
        assert lines in section


def test_the_stride_is_the_cell_count_rounded_up_to_sixteen():
    from snake_engine import lib
    L = lib()
    for hw in range(5, 20):
        assert L.snk_pit_record_stride(hw, hw) == (hw * hw + 15) // 16 * 16
    for h, w in ((4, 4), (20, 20), (7, 9), (0, 0), (-1, -1)):
        assert L.snk_pit_record_stride(h, w) == -1


def test_refusals_and_the_no_op_without_a_device():
    """r = 0 returns before anything is looked at; a negative r and NULL arrays are refused with a message -- no engine, no
    buffer and no device exists here, so none of these calls can have launched or copied anything"""
    from snake_engine import lib
    L = lib()
    assert L.snk_pit_record_slots(None, None, 0, None, None) == 0
    assert L.snk_pit_record_moves(None, None, None, 0, None, None, None) == 0
    assert L.snk_pit_record_boards(None, None, None, 0, None, None) == 0
    one = (C.c_int32 * 1)(0)
    for call, word in ((lambda: L.snk_pit_record_slots(None, None, -1, None, None), "r=-1"),
                       (lambda: L.snk_pit_record_moves(None, None, None, -3, None, None, None), "r=-3"),
                       (lambda: L.snk_pit_record_boards(None, None, None, -1, None, None), "r=-1"),
                       (lambda: L.snk_pit_record_slots(None, C.addressof(one), 1, None, None), "NULL"),
                       (lambda: L.snk_pit_record_moves(None, None, None, 1, None, None, None), "NULL"),
                       (lambda: L.snk_pit_record_boards(None, None, None, 1, None, None), "NULL")):
        assert call() == -1
        assert word in L.snk_last_error().decode()


# ---- 4. Arena.record / League.record and Replay ------------------------------------------------------------------------------------
def _bare(cls, game_cnt):
    """an arena or league without an engine: record must not need one"""
    self = cls.__new__(cls)
    self.height, self.width, self.game_cnt, self._recorder = 7, 7, game_cnt, None
    return self


@pytest.mark.parametrize("kind", ["arena", "league"])
def test_record_refuses_bad_index_lists_before_touching_the_device(kind):
    from snake_engine.arena import Arena
    from snake_engine.league import League
    from snake_engine.replay import Replay
    host = _bare(Arena if kind == "arena" else League, 10)
    for bad in ([10], [-1], [3, 3], [0, 1, 2, 1], [1.5], range(11)):
        with pytest.raises(ValueError):
            host.record(bad)
        assert host._recorder is None
    rep = host.record(iter([7, 0, 3]))
    assert isinstance(rep, Replay) and host._recorder is rep and rep.games.tolist() == [7, 0, 3] and rep.games.dtype == np.int32
    assert host.record([]).games.tolist() == []
    with pytest.raises(RuntimeError):
        rep.frames(7)


def test_replay_text_is_the_str_of_a_list_per_row(tmp_path):
    from snake_engine.replay import Replay
    rep = Replay([4, 2], 5, 5, 6)
    assert rep.stride == 32
    frames = np.zeros((2, 5, 5), np.int8)
    frames[0, 0] = [0, 9, -1, 1, 1]
    frames[0, 4] = [-8, 8, 0, 0, 9]
    frames[1, 2, 2] = -3
    host = np.full((1, 2, 2, rep.stride), 77, np.int8)          # one turn, two recorded games, padding that must not show
    host[0, 1, :, :25] = frames.reshape(2, 25)
    rep._host, rep.lengths = host, np.array([0, 1], np.int32)
    want = ("[0, 9, -1, 1, 1]\n" + "[0, 0, 0, 0, 0]\n" * 3 + "[-8, 8, 0, 0, 9]\n\n"
            + "[0, 0, 0, 0, 0]\n" * 2 + "[0, 0, -3, 0, 0]\n" + "[0, 0, 0, 0, 0]\n" * 2 + "\n").encode()
    assert rep.frames(2).dtype == np.int8 and np.array_equal(rep.frames(2), frames)
    assert rep.text(2) == want == RR.text(frames)
    assert rep.frames(4).shape == (0, 5, 5) and rep.text(4) == b""
    with pytest.raises(KeyError):
        rep.frames(0)
    path = tmp_path / "replay.rep"
    rep.write(2, str(path))
    rep.write(2, str(path))
    assert path.read_bytes() == want * 2
    rep.write(2, str(path), append=False)
    assert path.read_bytes() == want
