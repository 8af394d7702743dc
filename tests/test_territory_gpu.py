"""GPU tests of the territory opponent: snk_pit_territory_values against the CPU statement (tests/territory_ref.py: plain Python, a
queue for every distance), scores equal as integers -- on every board of the golden trajectories, on hand-built boards aimed at
the kernel's fronts (the two fronts meeting at an even and at an odd distance for each length relation, the meeting cell on either
side of every word boundary, a start cell at a row's end, an empty start set, a stale ring, eight snakes), on edge rows and sizes
and the refusals -- then whole matches through Arena.match and League.play against the statement's match player, with the
read-backs of a Scripted match."""
import functools

import numpy as np
import pytest

import script_ref as R
import search_pit_ref as SR
import territory_ref as T
import test_script_gpu as SG

pytestmark = pytest.mark.gpu

SENT = -7.0


def _values(eng, pairs, flags=R.ALL, hungry=100, extra=3):
    """snk_pit_territory_values over int pairs [m][2] -> int64[m][3]; the `extra` sentinel rows past m must stay as they are"""
    import torch
    from snake_engine._lib import check
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    m = len(pairs)
    d_pairs = torch.as_tensor(pairs, device="cuda") if m else None
    q = torch.full((m + extra, 3), SENT, dtype=torch.float32, device="cuda")
    check(eng.L.snk_pit_territory_values(eng.h, d_pairs.data_ptr() if m else 0, m, flags, hungry, q.data_ptr(), 0))
    torch.cuda.synchronize()
    out = q.cpu().numpy()
    assert (out[m:] == SENT).all(), "a row past m was written"
    assert np.array_equal(out[:m], np.round(out[:m])), "a score is no integer"
    return out[:m].astype(np.int64)


def _want(H, W, boards, pairs, flags, hungry=100):
    per_board = {}
    out = []
    for g, s in pairs:
        if g not in per_board:
            per_board[g] = T.board_scores(H, W, boards[g], flags, hungry)
        out.append(per_board[g][s])
    return np.array(out, np.int64).reshape(-1, 3)


def _differ(got, want, pairs, what):
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(pairs)} rows differ, first {pairs[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"


# ---- 1. every board of the golden trajectories ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden(cfg):
    H, W, S, boards = T.golden(cfg)
    return H, W, S, boards, SG._engine_with(H, W, S, boards)


@pytest.mark.parametrize("cfg", SG.GOLDEN)
def test_every_alive_row_of_the_golden_trajectories(cfg):
    """one word (5x5, 7x7), two (9x9, 11x11), four and six with 16-bit ring entries; five and more snakes put snakes k and k + 4 on
    one lane.  hungry = 100, and a threshold that has recorded healths on both sides of it"""
    H, W, S, boards, eng = _golden(cfg)
    pairs = SG._alive_pairs(boards)
    assert len(pairs) > 100
    split = T.golden_hungry(cfg)
    health = np.array([int(boards[g]["health"][s]) for g, s in pairs])
    assert (health <= split).any() and (health > split).any() and 0 <= split < 100
    differs = False
    for flags in (range(8) if H <= 9 else (R.ALL,)):
        for hungry in (100, split):
            got = _values(eng, pairs, flags, hungry)
            want = np.array([z for of in T.golden_scores(cfg, flags, hungry) for s, z in sorted(of.items())], np.int64)
            _differ(got, want, pairs, f"{cfg} flags {flags} hungry {hungry}")
        differs |= (got != _values(eng, pairs, flags, 100)).any()
    assert differs, "the threshold changes no score"
    if cfg == "11x11x4":
        plain = SG._values(eng, pairs)
        assert (got == -1).any() and ((got == -1) == (plain == -1)).all() and (got % 512 <= plain % 512).all()
        assert (got % 512 < plain % 512).any()


# ---- 2. hand-built boards aimed at the fronts -------------------------------------------------------------------------------------
S_HAND = 4


def _board(hw, snakes, dead=(), food=()):
    """script_ref.board of up to S_HAND snakes, filled up to S_HAND with dead snakes whose stale nodes lie across the middle row
    (a dead snake occupies nothing and has no front)"""
    assert len(snakes) <= S_HAND
    stale = [(hw // 2, x) for x in range(hw)]
    n = len(snakes)
    return R.board(hw, hw, list(snakes) + [(stale, 1)] * (S_HAND - n), food=food, dead=list(dead) + list(range(n, S_HAND)))


def _snakes_of(st, W):
    """the live snakes of a compact board as script_ref.board takes them"""
    return [([divmod(int(c), W) for c in st["nodes"][t][:int(st["length"][t])]], int(st["dir"][t]))
            for t in range(len(st["alive"])) if st["alive"][t]]


def _free_run(st, hw, length, avoid):
    """the first horizontal run of `length` free cells, scanning the rows from the middle outwards, that keeps clear of the cells
    `avoid`: a place for one more snake, heading east, its head at the run's east end"""
    occupied = T._occupied(st) | {y * hw + x for y, x in avoid}
    for y in sorted(range(hw), key=lambda y: (abs(y - hw // 2), y)):
        for x in range(hw - length + 1):
            if all(y * hw + xx not in occupied for xx in range(x, x + length)):
                return [(y, xx) for xx in range(x + length - 1, x - 1, -1)]
    raise AssertionError("no room for one more snake")


def _contested(st, hw, length):
    """the two-snake board st of tests/test_script_gpu.py with a third live snake of `length` cells in its open part: shorter than,
    as long as or longer than the mover (length 2)"""
    mover = _snakes_of(st, hw)[0][0]
    near = {(y + dy, x + dx) for y, x in mover for dy in (-1, 0, 1) for dx in (-1, 0, 1)}
    return _board(hw, _snakes_of(st, hw) + [(_free_run(st, hw, length, near), 1)])


def _serpentine(hw, h, length):
    """test_script_gpu's serpentine -- ONE corridor through the whole board -- with a snake of `length` cells at its far end: in the
    last row, its head h cells from the corridor's dead end and heading back up the corridor, its body towards the dead end.
    Above it is wall and below it the edge: its start set is the one cell in front of it.  The wall snake's head (1, 0) heads
    north between the mover's tail and wall: an EMPTY start set.  The mover's front and the third snake's run towards each other
    along the corridor; h and h + 1 give the two parities"""
    st = SG._serpentine(hw)
    if (hw - 2) // 2 % 2 == 0:                              # the last wall's door is at the east end: the dead end is (hw - 1, 0)
        cells, d = [(hw - 1, x) for x in range(h, h - length, -1)], 1
    else:
        cells, d = [(hw - 1, hw - 1 - x) for x in range(h, h - length, -1)], 3
    return _board(hw, _snakes_of(st, hw) + [(cells, d)])


def _corridor_length(hw):
    return (hw + 1) // 2 * hw + (hw - 1) // 2 - 2           # test_script_gpu: the even rows, a door per wall, less the mover


def _u_path(hw, y):
    """a corridor of hw + 8 cells: row y from edge to edge and four cells up (or, near the top, down) either edge column"""
    up = -1 if y >= 4 else 1
    return ([(y + up * k, 0) for k in range(4, 0, -1)] + [(y, x) for x in range(hw)] + [(y + up * k, hw - 1) for k in range(1, 5)])


def _meeting(hw, c, even, length):
    """a board that is wall but for the corridor _u_path through cell c's row.  The mover (snake 0, length 2) stands in it heading
    along it, a snake of `length` cells faces it, and the free cells between them are so many that -- even -- the cell c is the
    tie, as far from the mover's target as from the other's start cell, or -- odd -- c is the last cell nearer the mover and
    its neighbour along the corridor the first one nearer the other snake.  Everything else is one wall snake, whose head is a
    wall cell with wall or the edge on all three sides: an empty start set"""
    y, x = divmod(c, hw)
    path = _u_path(hw, y)
    i = path.index((y, x))
    r = min(i - 2, len(path) - 4 - i - (0 if even else 1), 3)
    assert r >= 1
    p, q = i - r - 1, i + r + (1 if even else 2)            # the mover's head, the other's head: targets path[p + 1], path[q - 1]
    mover = [path[p], path[p - 1]]
    other = path[q:q + length]
    assert p >= 1 and len(other) == length
    heading = lambda a, b: R.STEP.index((b[0] - a[0], b[1] - a[1]))
    taken = set(path)
    wall = [(yy, xx) for yy in range(hw) for xx in range(hw) if (yy, xx) not in taken]
    inner = lambda yy, xx: all(not (0 <= yy + dy < hw and 0 <= xx + dx < hw) or (yy + dy, xx + dx) not in taken
                               for dy, dx in (R.STEP[3], R.STEP[0], R.STEP[1]))
    head = next(w for w in wall if inner(*w))
    wall.remove(head)
    st = _board(hw, [(mover, heading(path[p], path[p + 1])), ([head] + wall, 0), (other, heading(path[q], path[q - 1]))])
    occupied = T._occupied(st)
    assert T.start_set(hw, hw, st, 1, occupied) == []
    assert set(T.start_set(hw, hw, st, 2, occupied)) - set(path[q + 1:]) == {path[q - 1]}      # a corner behind a one-cell snake is a dead end
    assert [t for t in T.targets(hw, hw, st, 0) if 0 <= t[0] < hw and 0 <= t[1] < hw and t[0] * hw + t[1] not in occupied] == [path[p + 1]]
    return st, r + 1                                        # the cells nearer the mover, c among them when it is no tie


def _row_end(hw, y, length):
    """a leak across a row's end.  Snake 1 heads east at (y, hw - 2): (y, hw - 1), the row's LAST column, is in its start set, and
    one bit further lies (y + 1, 0), hw steps away on the board.  The mover heads west at (y + 1, 2): its target (y + 1, 1) is
    one step from (y + 1, 0), which a front shifted across the row end would reach in one step too.  The mirror image stands in
    the rows above: snake 2 heads west at (y - 2, 1) with (y - 2, 0) in its start set, one bit after (y - 3, hw - 1)"""
    east = [(y, x) for x in range(hw - 2, hw - 2 - length, -1)]
    west = [(y - 2, x) for x in range(1, 1 + length)]
    return _board(hw, [([(y + 1, 2), (y + 1, 3)], 3), (east, 1), (west, 3)])


def _hand_boards(hw):
    """(boards, notes): note[g] says what board g must show, for the assertions beside the comparison with the statement"""
    boards, notes = [], []
    for h in (2, 3):
        for length in (1, 2, 3):
            boards.append(_serpentine(hw, h, length))
            notes.append(("serpentine", h, length))
    for st in [SG._empty(hw)] + SG._edge_pockets(hw) + SG._word_pockets(hw):
        for length in (1, 3):
            boards.append(_contested(st, hw, length))
            notes.append(("contested", None, length))
    for c in range(64, hw * hw, 64):
        for cell in (c - 1, c):
            for even in (True, False):
                for length in (1, 2, 3):
                    st, mine = _meeting(hw, cell, even, length)
                    boards.append(st)
                    notes.append(("meeting", (mine, even), length))
    for y in (3, hw - 2):
        for length in (1, 3):
            boards.append(_row_end(hw, y, length))
            notes.append(("row-end", y, length))
    return boards, notes


@pytest.mark.parametrize("hw", [7, 9, 11, 19])
def test_hand_built_boards_through_import_states(hw):
    nc = hw * hw
    boards, notes = _hand_boards(hw)
    assert sum(n[0] == "meeting" for n in notes) == 12 * ((nc - 1) // 64)    # 7x7: none; 9x9, 11x11: one boundary; 19x19: five
    pairs = SG._alive_pairs(boards)
    cap = 1 << (nc + 1).bit_length()                                          # the ring's size: the power of two from NC + 2 up
    for ring_start in (0, cap - 1, cap - 40):                                 # laid out from the ring's start, and wrapping past its end
        eng = SG._engine_with(hw, hw, S_HAND, boards, ring_start)
        for flags, hungry in [(f, 100) for f in range(8)] + [(R.ALL, 89)] if ring_start == 0 else [(R.ALL, 100)]:
            got = _values(eng, pairs, flags, hungry)
            _differ(got, _want(hw, hw, boards, pairs, flags, hungry), pairs, f"{hw} ring {ring_start} flags {flags} hungry {hungry}")
    row = {tuple(p): got[i] for i, p in enumerate(pairs)}
    fill = lambda g: int(row[(g, 0)][1] % 512)                                # the mover's straight move
    serp = {(n[1], n[2]): fill(g) for g, n in enumerate(notes) if n[0] == "serpentine"}
    for h in (2, 3):
        between = _corridor_length(hw) - (h + 1)                              # free cells from the mover's target to the other's start cell
        half = between // 2
        if between % 2:                                                       # a middle cell: the longer snake's, or nobody's
            assert (serp[(h, 1)], serp[(h, 2)], serp[(h, 3)]) == (half + 1, half, half), (h, serp)
        else:
            assert serp[(h, 1)] == serp[(h, 2)] == serp[(h, 3)] == half, (h, serp)
    for g, n in enumerate(notes):
        if n[0] == "meeting":
            (mine, even), length = n[1], n[2]
            assert fill(g) == (mine if length < 2 or not even else mine - 1), (g, n, fill(g))
        if n[0] == "row-end":
            assert row[(g, 0)][1] % 512 > 0


def test_eight_live_snakes_on_19x19():
    """every lane of the quad walks two rings and sets two snakes' start cells; lengths 1 .. 8 make every row see strong and weak
    fronts (but the longest and the shortest)"""
    snakes = []
    for k in range(8):
        y, x0 = 2 + 2 * k, (3 * k) % 9
        cells = [(y, x) for x in range(x0 + k, x0 - 1, -1)] if k % 2 == 0 else [(y, x) for x in range(18 - x0 - k, 19 - x0)]
        snakes.append((cells, 1 if k % 2 == 0 else 3))
    st = R.board(19, 19, snakes, food=[(0, 0), (18, 18), (9, 9)])
    st["health"][:] = [100, 60, 40, 39, 41, 1, 90, 40]
    assert sorted(int(v) for v in st["length"]) == list(range(1, 9)) and len(T._occupied(st)) == 36
    eng = SG._engine_with(19, 19, 8, [st])
    pairs = SG._alive_pairs([st])
    assert len(pairs) == 8
    for flags, hungry in ((R.ALL, 100), (R.ALL, 40), (R.SPACE, 100), (R.SPACE | R.HEADS, 0)):
        got = _values(eng, pairs, flags, hungry)
        _differ(got, _want(19, 19, [st], pairs, flags, hungry), pairs, f"flags {flags} hungry {hungry}")
    plain = SG._values(eng, pairs, R.SPACE)
    assert (got % 512 < plain % 512)[got >= 0].all() and (got >= 0).sum() >= 16


# ---- 3. edge rows, sizes and refusals -----------------------------------------------------------------------------------------------
def test_dead_and_out_of_range_pairs_and_row_counts():
    H, W, S, boards, eng = _golden("11x11x4")
    n = len(boards)
    dead = np.array([(g, s) for g, st in enumerate(boards) for s in range(S) if not st["alive"][s]], np.int32)
    assert len(dead) > 100
    assert (_values(eng, dead) == -1).all()
    bad = np.array([(-1, 0), (n, 0), (0, S), (0, -1), (1 << 30, 1), (-(1 << 31), 2), (3, 1 << 30), (0, 8)], np.int32)
    assert (_values(eng, bad) == -1).all()
    want_of = T.golden_scores("11x11x4")
    rng = np.random.RandomState(5)
    for m in (0, 1, 3, 63, 64, 65, 4099):
        pairs = np.stack([rng.randint(0, n, m), rng.randint(0, S, m)], 1).astype(np.int32)
        hit = rng.rand(m) < 0.1
        pairs[hit] = bad[rng.randint(0, len(bad), int(hit.sum()))]
        want = np.array([want_of[g].get(s, [-1] * 3) if 0 <= g < n and 0 <= s < S else [-1] * 3 for g, s in pairs], np.int64)
        assert np.array_equal(_values(eng, pairs), want.reshape(-1, 3)), m


def test_refusals_of_the_entry_point():
    import torch
    from snake_engine import EngineError
    from snake_engine._lib import check
    H, W, S, boards, eng = _golden("7x7x2")
    pairs = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    q = torch.full((1, 3), SENT, dtype=torch.float32, device="cuda")
    call = eng.L.snk_pit_territory_values
    for flags in (8, 15, 1 << 31):
        with pytest.raises(EngineError, match="snk_pit_territory_values: unknown flag"):
            check(call(eng.h, pairs.data_ptr(), 1, flags, 100, q.data_ptr(), 0))
    for hungry in (101, -1, 1 << 20):
        with pytest.raises(EngineError, match="snk_pit_territory_values: hungry"):
            check(call(eng.h, pairs.data_ptr(), 1, 7, hungry, q.data_ptr(), 0))
    for d_pairs, d_q in ((0, q.data_ptr()), (pairs.data_ptr(), 0)):
        with pytest.raises(EngineError, match="snk_pit_territory_values: NULL argument"):
            check(call(eng.h, d_pairs, 1, 7, 100, d_q, 0))
    with pytest.raises(EngineError, match="snk_pit_territory_values: m=-1"):
        check(call(eng.h, pairs.data_ptr(), -1, 7, 100, q.data_ptr(), 0))
    with pytest.raises(EngineError, match="snk_pit_territory_values: engine is NULL"):
        check(call(0, pairs.data_ptr(), 1, 7, 100, q.data_ptr(), 0))
    torch.cuda.synchronize()
    assert (q.cpu().numpy() == SENT).all()
    check(call(eng.h, 0, 0, 7, 100, 0, 0))                                    # m = 0 is a no-op, its buffers may be NULL
    check(call(eng.h, 0, 0, 0, 0, 0, 0))


# ---- 4. whole matches against the statement -------------------------------------------------------------------------------------
def _counted(monkeypatch, play):
    """play() -> (its result, the Tensor.cpu / .item / .tolist / .numpy calls it made): tests/test_script_gpu.py's count"""
    import torch
    count = [0]

    def counted(orig):
        def f(self, *a, **k):
            count[0] += 1
            return orig(self, *a, **k)
        return f
    torch.cuda.synchronize()
    with monkeypatch.context() as mp:
        for name in ("cpu", "item", "tolist", "numpy"):
            mp.setattr(torch.Tensor, name, counted(getattr(torch.Tensor, name)))
        res = play()
    return res, count[0]


@pytest.mark.parametrize("name, board, n, side_a, flags_b", [("duel-7x7x2", "7x7x2", T.N_DUEL, (R.ALL, 100), R.ALL),
                                                             ("1v3-11x11x4", "11x11x4", T.N_FOUR, (R.ALL, T.HUNGRY_FOUR), R.HEADS)])
def test_territory_against_scripted_through_arena_match(monkeypatch, name, board, n, side_a, flags_b):
    from snake_engine.arena import Arena, Scripted, Territory
    from snake_engine.engine import compact_from_state
    want = T.reference(name)
    H, W, S, hd = want["geometry"]
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(SR.start_states(board, n))
    res, reads = _counted(monkeypatch, lambda: arena.match(Territory(*side_a), Scripted(flags_b), 1, spawn_tape=SG._spawn(want)))
    SG._check_match(res, want, [compact_from_state(s) for s in arena.engine.export()])
    assert res.wins_a + res.wins_b + res.draws == n
    plain = Arena(H, W, S, hd, n, seed=1)                                     # the same seats, all scripted: its read-backs per turn
    plain.import_states(SR.start_states(board, n))
    res_p, reads_p = _counted(monkeypatch, lambda: plain.match(Scripted(), Scripted(flags_b), 1))
    assert res_p.turns >= 3 and reads - res.turns == reads_p - res_p.turns, (reads, res.turns, reads_p, res_p.turns)


def test_a_territory_owner_a_scripted_owner_and_a_stub_net_through_league_play(monkeypatch):
    from stubnet_device import DeviceStubNNet
    from snake_engine.arena import Scripted, Territory
    from snake_engine.engine import compact_from_state
    from snake_engine.league import League
    want = T.reference("league-11x11x4")
    H, W, S, hd = want["geometry"]
    n, counts = T.N_LEAGUE, []
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(SR.start_states("11x11x4", n))
    res, reads = _counted(monkeypatch, lambda: league.play([Territory(), Scripted(), DeviceStubNNet()], R.three_owner_table(n),
                                                           counts_log=counts, spawn_tape=SG._spawn(want)))
    SG._check_match(res, want, [compact_from_state(s) for s in league.engine.export()], res.winner_owner)
    assert counts == want["counts"]
    assert all(c > 0 for c in want["counts"][0]) and len(set(want["winner_owner"])) >= 2
    plain = League(H, W, S, hd, n, seed=1)
    plain.import_states(SR.start_states("11x11x4", n))
    res_p, reads_p = _counted(monkeypatch, lambda: plain.play([Scripted(), Scripted(), DeviceStubNNet()], R.three_owner_table(n)))
    assert res_p.turns >= 3 and reads - res.turns == reads_p - res_p.turns, (reads, res.turns, reads_p, res_p.turns)
