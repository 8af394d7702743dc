"""GPU tests of the pit's tally (snake_engine/tally.py; snk_pit_tally).  The kernel alone, cell for cell as integers against the CPU
statement (tests/tally_ref.py): every tick of the golden trajectories of the eight geometries played through
snk_engine_step_active_tape and the hand-built ticks of tests/test_tally_cpu.py, with rings laid out from their start, their last
and their third-last entry; after each step the engine's own alive flags against the tally's deaths; n around a block's four
wavefronts with a sentinel in every cell that must not be written; the refusals.  Then whole matches through Arena.match,
League.play and League.play_search -- stub nets, a Searcher, a Scripted -- against the statement's players and against the same
match without a tally, the engine's counters and exported lengths, a recorder beside the tally, and the launch and read-back
counts."""
import functools
import sys

import numpy as np
import pytest

import league_ref as LR
import league_search_ref as LSR
import replay_ref as RR
import script_ref as SC
import search_pit_ref as SR
import tally_ref as TR
import test_tally_cpu as TC
from conftest import golden_state, load_golden
from pit_calls import Calls as _Calls

pytestmark = pytest.mark.gpu

SENTINEL = -7
GUARD = 8           # rows past the engine's games, which must keep the sentinel
GOLDEN = ["5x5x2", "7x7x2", "9x9x3", "11x11x4", "11x11x4_dec9", "15x15x5", "16x16x6", "19x19x8"]
FIELDS = ("fate", "died", "food", "length")


# ---- the kernel through the entry point alone ---------------------------------------------------------------------------------------
def _engine_with(H, W, S, boards, ring_start=0, health_dec=1, chance=0.15):
    from snake_engine import Engine
    from snake_engine.engine import state_from_compact
    eng = Engine(len(boards), H, W, S, health_dec, chance, seed=1)
    eng.import_states([state_from_compact(H, W, S, st) for st in boards], ring_start=ring_start)
    return eng


def _boards(eng):
    from snake_engine.engine import compact_from_state
    return [compact_from_state(s) for s in eng.export()]


def _wrapped(H, W, ring_start):
    cap = 1 << (H * W + 1).bit_length()
    assert cap // 2 < H * W + 2 <= cap
    return ring_start % cap


def tally_ticks(eng, ticks, n=None):
    """the tally's turn, once per entry of ticks = (live uint8[n_slots], moves uint8[n_slots][S], spawn int16[n_slots] or None):
    snk_pit_tally over the first n games into four fresh arrays int32[n_slots + GUARD][S] that hold SENTINEL, then the step over
    all games.  Returns (int32[T][4][n_slots + GUARD][S], the engine's alive flags uint8[T][n_slots][S] after each step); the
    tick with index t is given turn number t + 1"""
    import torch
    from snake_engine._lib import check
    L, N, S = eng.L, eng.n_slots, eng.S
    n = N if n is None else n
    done = torch.zeros((N,), dtype=torch.uint8, device="cuda")
    out, flags = [], []
    for t, (live, moves, spawn) in enumerate(ticks):
        d_live = torch.as_tensor(np.ascontiguousarray(live, np.uint8), device="cuda")
        d_moves = torch.as_tensor(np.ascontiguousarray(moves, np.uint8).reshape(N, S), device="cuda")
        d_spawn = None if spawn is None else torch.as_tensor(np.ascontiguousarray(spawn, np.int16), device="cuda")
        a = torch.full((4, N + GUARD, S), SENTINEL, dtype=torch.int32, device="cuda")
        check(L.snk_pit_tally(eng.h, d_live.data_ptr(), n, d_moves.data_ptr(), t + 1, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(),
                              a[3].data_ptr(), 0))
        check(L.snk_engine_step_active_tape(eng.h, d_live.data_ptr(), N, d_moves.data_ptr(), 0 if spawn is None else d_spawn.data_ptr(),
                                            done.data_ptr(), None, 0))
        out.append(a)
        flags.append(eng.alive())
    torch.cuda.synchronize()
    return torch.stack(out).cpu().numpy(), torch.stack(flags).cpu().numpy()


def expected_cells(H, W, hd, pre, dense, turn, handled):
    """what one launch leaves in a game's four rows that held SENTINEL -> int32[4][S]"""
    S = len(pre["alive"])
    want = np.full((4, S), SENTINEL, np.int32)
    got = TR.tick_fates(H, W, hd, pre, dense) if handled else None
    if got is not None:
        fate, eats, length = got
        was = np.asarray(pre["alive"]).astype(bool)
        want[0][fate > 0] = fate[fate > 0]
        want[1][fate > 0] = turn
        want[2][was] = SENTINEL + eats[was]
        want[3][was] = length[was]
    return want


def _compare(got, want, what):
    for k, name in enumerate(FIELDS):
        assert got[k].tolist() == want[k].tolist(), f"{what}: {name}"


@functools.lru_cache(maxsize=None)
def _golden(cfg):
    """the trajectories of a file in lock step, one game each, and what the statement says of every tick: computed once, shared
    by the ring starts.  -> (geometry, start boards, ticks, want int32[T][G][4][S], alive before each tick bool[T][G][S])"""
    z = TC.golden_arrays(f"tic_{cfg}.npz")
    H, W, S, hd = int(z["H"]), int(z["W"]), int(z["S"]), int(z["health_dec"])
    ptr = z["ptr"]
    G = len(ptr) - 1
    T = [int(ptr[g + 1] - ptr[g] - 1) for g in range(G)]
    ticks = []
    for t in range(max(T)):
        live = np.array([t < T[g] for g in range(G)], np.uint8)
        idx = [int(ptr[g] - g + min(t, T[g] - 1)) for g in range(G)]
        ticks.append((live, z["moves"][idx], z["spawn"][idx]))
    want = np.zeros((max(T), G, 4, S), np.int32)
    before = np.zeros((max(T), G, S), bool)
    for t in range(max(T)):
        for g in range(G):
            pre = golden_state(z, ptr[g] + min(t, T[g]))            # a trajectory that is over stays on its last board
            want[t, g] = expected_cells(H, W, hd, pre, ticks[t][1][g], t + 1, t < T[g])
            before[t, g] = pre["alive"]
    for a in (want, before):
        a.setflags(write=False)
    return (H, W, S, hd, float(z["food_chance"])), [golden_state(z, ptr[g]) for g in range(G)], ticks, want, before, sum(T)


@pytest.mark.parametrize("ring_start", [0, -1, -3])
@pytest.mark.parametrize("cfg", GOLDEN)
def test_every_tick_of_the_golden_trajectories(cfg, ring_start):
    """a trajectory that is over is a closed game: its rows keep the sentinel"""
    (H, W, S, hd, chance), boards, ticks, want, before, played = _golden(cfg)
    G = len(boards)
    eng = _engine_with(H, W, S, boards, _wrapped(H, W, ring_start), hd, chance)
    got, flags = tally_ticks(eng, ticks)
    assert (got[:, :, G:] == SENTINEL).all(), "a row past n was written"
    got = got[:, :, :G].transpose(0, 2, 1, 3)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{cfg}, ring start {ring_start}: tick {bad[0][0]} game {bad[0][1]} {FIELDS[bad[0][2]]} of seat {bad[0][3]} is "
                           f"{got[tuple(bad[0])]}, the statement has {want[tuple(bad[0])]}")
    died = (want[:, :, 0] > 0)
    assert (flags.astype(bool) == (before & ~died)).all(), "the engine's alive flags after each step against the tally's deaths"
    handled = (want[:, :, 3] != SENTINEL).any(axis=2)
    assert handled.sum() == played >= 50 and died.sum() >= 1


@pytest.mark.parametrize("ring_start", [0, -1, -3])
def test_hand_built_ticks_and_wrapped_rings(ring_start):
    """the ticks of tests/test_tally_cpu.py and the fates worked out by hand there"""
    H, W = TC.H, TC.W
    for S in (2, 3):
        names = [k for k, c in TC.CASES.items() if len(c["moves"]) == S]
        eng = _engine_with(H, W, S, [TC.CASES[k]["board"] for k in names], _wrapped(H, W, ring_start), 1, 0.0)
        live = np.ones(len(names), np.uint8)
        got, flags = tally_ticks(eng, [(live, np.stack([TC.CASES[k]["moves"] for k in names]), None)])
        for i, k in enumerate(names):
            case = TC.CASES[k]
            was = case["board"]["alive"].astype(bool)
            fate, eats, length = (np.array(case[f]) for f in ("fate", "eats", "length"))
            _compare(got[0, :, i], expected_cells(H, W, 1, case["board"], case["moves"], 1, True), f"{k}, ring start {ring_start}")
            assert np.where(got[0, 0, i] == SENTINEL, 0, got[0, 0, i]).tolist() == fate.tolist(), f"{k}: the fates worked out by hand"
            assert (got[0, 2, i][was] - SENTINEL).tolist() == eats[was].tolist() and got[0, 3, i][was].tolist() == length[was].tolist(), k
            assert (flags[0, i].astype(bool) == (was & (fate == 0))).all(), f"{k}: the engine's alive flags after the step"
    assert sum(len(c["moves"]) in (2, 3) for c in TC.CASES.values()) == len(TC.CASES)


@functools.lru_cache(maxsize=None)
def _played(n=300):
    """n 11x11 games of four snakes a few random ticks into play: some over, some with dead seats, some with food eaten.  They are
    put in an order in which the first three are a game with a dead seat that still moves, one that stands still (fewer than
    two snakes alive) and one with every seat alive, so that the smallest n of the test below meets each kind"""
    import torch
    from snake_engine import Engine
    from snake_engine.engine import compact_from_state
    eng = Engine(n, 11, 11, 4, 1, 0.15, seed=9)
    eng.reset()
    rng = np.random.RandomState(2)
    for _ in range(7):
        eng.step(torch.as_tensor(rng.randint(0, 3, size=(n, 4)).astype(np.uint8), device="cuda"))
    states = eng.export()
    alive = np.array([int(compact_from_state(st)["alive"].sum()) for st in states])
    first = [int(np.flatnonzero(pick)[0]) for pick in ((alive == 2) | (alive == 3), alive < 2, alive == 4)]
    order = first + [g for g in range(n) if g not in first]
    eng.import_states([states[g] for g in order])
    return eng


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_short_last_blocks_closed_games_and_dead_seats_keep_the_sentinel(n):
    """a block holds four wavefronts, so these n end in a block with one, three, none, one and one.  The games are read, never
    stepped on from here, by every case alike: the statement is given the boards as they stand"""
    import torch
    from snake_engine._lib import check
    eng = _played()
    N, S = eng.n_slots, eng.S
    pre = _boards(eng)
    rng = np.random.RandomState(50 + n)
    live = (rng.rand(N) < 0.8).astype(np.uint8)
    live[:5] = 1, 1, 1, 0, 1                                             # a closed game in front of the block's last wavefront
    moves = rng.randint(0, 3, size=(N, S)).astype(np.uint8)
    a = torch.full((4, N + GUARD, S), SENTINEL, dtype=torch.int32, device="cuda")
    d_live, d_moves = torch.as_tensor(live, device="cuda"), torch.as_tensor(moves, device="cuda")
    check(eng.L.snk_pit_tally(eng.h, d_live.data_ptr(), n, d_moves.data_ptr(), 40, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(),
                              a[3].data_ptr(), 0))
    torch.cuda.synchronize()
    got = a.cpu().numpy()
    assert (got[:, n:] == SENTINEL).all(), "a row past n was written"
    kinds = dict(closed=0, still=0, dead_seat=0, moved=0)
    for g in range(n):
        alive = pre[g]["alive"].astype(bool)
        _compare(got[:, g], expected_cells(11, 11, 1, pre[g], moves[g], 40, bool(live[g])), f"n = {n}, game {g}")
        if not live[g]:
            kinds["closed"] += 1
            assert (got[:, g] == SENTINEL).all()
        elif alive.sum() < 2:
            kinds["still"] += 1
            assert (got[:, g] == SENTINEL).all()
        else:
            kinds["moved"] += 1
            kinds["dead_seat"] += int((~alive).any())
            assert (got[:, g][:, ~alive] == SENTINEL).all() and (got[3, g][alive] >= 3).all()
    assert kinds["moved"] >= 1 and kinds["dead_seat"] >= 1
    if n >= 3:
        assert kinds["still"] >= 1
    if n >= 4:
        assert kinds["closed"] >= 1
    if n == 257:
        assert all(v >= 5 for v in kinds.values()), kinds


def test_the_refusals():
    import torch
    from snake_engine import EngineError
    from snake_engine._lib import check
    eng = _played()
    N, S = eng.n_slots, eng.S
    a = torch.full((4, N, S), SENTINEL, dtype=torch.int32, device="cuda")
    d_live = torch.ones((N,), dtype=torch.uint8, device="cuda")
    d_moves = torch.ones((N, S), dtype=torch.uint8, device="cuda")
    good = [eng.h, d_live.data_ptr(), N, d_moves.data_ptr(), 1, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), 0]
    for at in (0, 1, 3, 5, 6, 7, 8):
        args = list(good)
        args[at] = None
        with pytest.raises(EngineError, match="NULL"):
            check(eng.L.snk_pit_tally(*args))
    for n, word in ((-1, "n=-1"), (N + 1, "exceeds")):
        args = list(good)
        args[2] = n
        with pytest.raises(EngineError, match=word):
            check(eng.L.snk_pit_tally(*args))
    check(eng.L.snk_pit_tally(eng.h, 0, 0, 0, 1, 0, 0, 0, 0, 0))
    torch.cuda.synchronize()
    assert (a.cpu().numpy() == SENTINEL).all(), "a refused call or the n = 0 no-op wrote"


# ---- whole matches -----------------------------------------------------------------------------------------------------------------
def _spawn(log):
    return lambda turn: np.maximum(log[turn - 1], -1)


def _reads(monkeypatch, play):
    """play() -> (its result, what every .tolist() made in arena.py / league.py brought: the turns' read-backs)"""
    import torch
    reads = []
    tolist = torch.Tensor.tolist

    def noted(self):
        out = tolist(self)
        if sys._getframe(1).f_code.co_filename.endswith(("arena.py", "league.py")):
            reads.append(out)
        return out
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "tolist", noted)
        res = play()
    return res, reads


def _twice(monkeypatch, make, play, recorded=None):
    """the match without a tally, then the same match on a new pit with one (and with a recorder): winners, lengths, turns and
    every turn's read-back are the same.  make() -> a pit on the start boards, play(pit) -> the result.  Returns the second pit,
    its tally, its Replay or None, its result and the sum of the engine's counters before the match"""
    plain, reads0 = _reads(monkeypatch, lambda: play(make()))
    pit = make()
    before = np.array(pit.engine.sum_counters())
    tal = pit.tally()
    rep = None if recorded is None else pit.record(recorded, first_turns=2)
    res, reads1 = _reads(monkeypatch, lambda: play(pit))
    assert pit._tallier is None, "the tally is dropped when the match ends"
    assert res.turns == plain.turns and reads1 == reads0 and len(reads1) == res.turns + 1
    for a, b in zip(res, plain):
        assert np.array_equal(np.asarray(a), np.asarray(b)), "a match with a tally differs from the one without"
    return pit, tal, rep, res, before


def _check_tally(tal, res, games, pit, before, owners, K):
    """every cell against the statement's players; the causes and the food against the engine's own counters; the final lengths
    and the alive flags against the exported boards"""
    eng = pit.engine
    n, S = eng.n_slots, eng.S
    for name in FIELDS:
        got, want = getattr(tal, name), np.stack([getattr(g, name) for g in games])
        assert got.dtype == np.int32 and got.shape == (n, S)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{name}: game {bad[0][0]} seat {bad[0][1]} is {got[tuple(bad[0])]}, the statement has {want[tuple(bad[0])]}"
    delta = np.array(eng.sum_counters()) - before
    assert [int((tal.fate == c).sum()) for c in (1, 2, 3, 4)] == delta[:4].tolist(), "deaths per cause against the engine's counters"
    assert int(tal.food.sum()) == delta[4], "food eaten against the engine's counter"
    assert delta[:4].sum() >= 1
    boards = _boards(eng)
    alive = np.stack([b["alive"] for b in boards]).astype(bool)
    length = np.stack([b["length"] for b in boards])
    assert ((tal.fate == 0) == alive).all(), "a seat without a fate is alive on the board of its game's verdict"
    assert (tal.length[alive] == length[alive]).all()
    assert (tal.died[alive] == 0).all() and (tal.died[~alive] >= 1).all() and (tal.died <= res.lengths[:, None]).all()
    assert (tal.died.max(axis=1) == res.lengths)[(~alive).any(axis=1)].all(), "a game's last death is its verdict turn"
    assert np.array_equal(tal.owners, owners) and tal.n_owners == K and np.array_equal(tal.lengths, res.lengths)
    rows = tal.by_owner()
    assert rows.seats.sum() == n * S and (rows.fates.sum(axis=1) == rows.seats).all() and rows.food.sum() == delta[4]
    assert rows.seats.tolist() == np.bincount(owners.reshape(-1), minlength=K).tolist()
    for c in range(5):
        assert tal.games(fate=c).tolist() == np.flatnonzero((tal.fate == c).any(axis=1)).tolist()
    assert len(tal.text().splitlines()) == K + 1


def _check_replay(rep, res, games, recorded):
    for g in recorded:
        got, want = rep.frames(g), np.stack(games[g].frames)
        assert got.shape == (2 * int(res.lengths[g]),) + want.shape[1:] == want.shape and np.array_equal(got, want), f"game {g}: the replay"


def test_a_recorded_reference_pit_through_arena_match_with_a_recorder_beside_the_tally(monkeypatch):
    from oracle.obs_key import StubNet
    from oracle.pit_oracle import pit_run
    from snake_engine.arena import Arena
    z, p, H, W, S, hd, n, a_cnt = LR.meta(2)
    games = [TR.Counting(RR.Recording(g)) for g in LR.start_games(2)]
    winners, lengths = pit_run(games, StubNet(0), StubNet(1), a_cnt, spawn_tape=lambda turn: z[p + "spawn"][turn - 1])

    def make():
        arena = Arena(H, W, S, hd, n, seed=1)
        arena.import_states(LR.start_states(2))
        return arena
    recorded = [11, 2, 7]
    arena, tal, rep, res, before = _twice(monkeypatch, make, lambda a: a.match(
        LR.DeviceStub(0), LR.DeviceStub(1), a_cnt, spawn_tape=lambda turn: z[p + "spawn"][turn - 1]), recorded)
    assert res.lengths.tolist() == lengths and res.winners.tolist() == [-1 if w is None else w for w in winners] and res.turns >= 8
    _check_tally(tal, res, games, arena, before, LR.two_team_table(n, S, a_cnt), 2)
    _check_replay(rep, res, games, recorded)


def test_a_match_with_a_searcher(monkeypatch):
    from oracle.obs_key import StubNet
    from snake_engine.arena import Arena, Searcher
    board, n, breadth, searching, seed = SR.CASES["7x7x2-b8-search-v-greedy"]
    bare, (H, W, S, hd) = SR.start_games(board, n)
    games = [TR.Counting(g) for g in bare]
    want = SR.search_pit_run(games, (StubNet(0), StubNet(1)), searching, 1, seed + 1000, SR.uniform_tape(seed), 4, breadth)
    SR.check_well_posed(want)

    def make():
        arena = Arena(H, W, S, hd, n, seed=1)
        arena.import_states(SR.start_states(board, n))
        return arena

    def play(arena):
        side = Searcher(SR.DeviceStub(0), breadth, 4, 100, seed=5, sequential=True, tape_u=SR.uniform_tape(seed))
        return arena.match(side, SR.DeviceStub(1), 1, spawn_tape=_spawn(want["spawn_log"]))
    arena, tal, _, res, before = _twice(monkeypatch, make, play)
    assert res.lengths.tolist() == want["lengths"] and res.turns == want["turns"]
    _check_tally(tal, res, games, arena, before, LR.two_team_table(n, S, 1), 2)


def test_a_match_with_a_scripted_side(monkeypatch):
    from snake_engine.arena import Arena, Scripted
    n = SC.N_DUEL
    bare, (H, W, S, hd) = SR.start_games("7x7x2", n)
    games = [TR.Counting(g) for g in bare]
    want = SC.script_run(games, [SC.RefScripted(), LR.RefStub(0)], LR.two_team_table(n, 2, 1), SC.SPAWN_SEED)

    def make():
        arena = Arena(H, W, S, hd, n, seed=1)
        arena.import_states(SR.start_states("7x7x2", n))
        return arena
    arena, tal, _, res, before = _twice(monkeypatch, make, lambda a: a.match(Scripted(), LR.DeviceStub(0), 1,
                                                                             spawn_tape=_spawn(want["spawn_log"])))
    assert res.lengths.tolist() == want["lengths"] and res.turns == want["turns"] >= 5
    _check_tally(tal, res, games, arena, before, LR.two_team_table(n, S, 1), 2)


def test_league_play_with_three_stub_owners(monkeypatch):
    from snake_engine.league import League
    z, p, H, W, S, hd, n, _ = LR.meta(2)
    games = [TR.Counting(RR.Recording(g)) for g in LR.start_games(2)]
    owner = LR.six_owner_table(n) % 3
    want = LR.league_run(games, [LR.RefStub(k) for k in range(3)], owner, food_seed=LR.FOOD_SEED)

    def make():
        league = League(H, W, S, hd, n, seed=1)
        league.import_states(LR.start_states(2))
        return league
    recorded = [9, 1, 15, 4]
    league, tal, rep, res, before = _twice(monkeypatch, make, lambda lg: lg.play(
        [LR.DeviceStub(k) for k in range(3)], owner, spawn_tape=_spawn(want["spawn_log"])), recorded)
    assert res.lengths.tolist() == want["lengths"] and res.turns == want["turns"] >= 5
    _check_tally(tal, res, games, league, before, owner.astype(np.uint8), 3)
    _check_replay(rep, res, games, recorded)
    rows = tal.by_owner()
    assert (rows.seats > 0).all() and not np.isnan(rows.turns).any()


def test_league_play_search(monkeypatch):
    from snake_engine.arena import Searcher
    from snake_engine.league import League
    board, breadth, searching, seed = LSR.CASES["7x7x2-b8-gsg"]
    table = LSR.TABLES[board]()
    n, K = len(table), len(searching)
    bare, (H, W, S, hd) = SR.start_games(board, n)
    games = [TR.Counting(g) for g in bare]
    tapes = LSR.tapes(seed, K)
    want = LSR.league_search_run(games, [LR.RefStub(o) for o in range(K)], searching, table, seed + 1000, tapes, 4, breadth)
    LSR.check_well_posed(want)
    net = lambda o: SR.DeviceStub(o) if o < 2 else LR.DeviceStub(o)      # noqa: E731

    def make():
        league = League(H, W, S, hd, n, seed=1)
        league.import_states(SR.start_states(board, n))
        return league

    def play(league):
        sides = [Searcher(net(o), breadth, 4, 100, seed=5 + o, sequential=True, tape_u=tapes[o]) if s else net(o)
                 for o, s in enumerate(searching)]
        return league.play_search(sides, table, spawn_tape=_spawn(want["spawn_log"]))
    league, tal, _, res, before = _twice(monkeypatch, make, play)
    assert res.lengths.tolist() == want["lengths"] and res.turns == want["turns"]
    _check_tally(tal, res, games, league, before, np.asarray(table, np.uint8), K)


# ---- launches and read-backs ---------------------------------------------------------------------------------------------------------
def test_launch_and_read_back_counts(monkeypatch):
    """four matches on the same start boards with the device's own food: before tally() was ever called, with a tally, with a
    tally and a recorder, and after them.  The first and the last issue the same sequence of library calls; the second issues
    that sequence plus one launch per turn, directly before the step, reads back once per turn as before and copies once after
    the last turn; in the third the tally's launch stands between the recorder's and the step"""
    import torch
    from snake_engine.arena import Arena, Scripted
    n = 24
    arena = Arena(11, 11, 4, 1, n, seed=3)
    start = arena.engine.export()
    calls = arena.engine.L = _Calls(arena.engine.L)
    runs = []
    for tallied, recorded in ((False, None), (True, None), (True, [20, 3, 8]), (False, None)):
        arena.import_states(start)
        tal = arena.tally() if tallied else None
        if recorded is not None:
            arena.record(recorded)
        del calls.names[:]
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
            res = arena.match(Scripted(), Scripted(SC.FOOD), 1)
        runs.append((res, list(calls.names), count[0], tal))
    (res0, seq0, reads0, _), (res1, seq1, reads1, tal1), (res2, seq2, reads2, tal2), (res3, seq3, reads3, _) = runs
    assert res0.turns == res1.turns == res2.turns == res3.turns >= 10
    assert res0.lengths.tolist() == res1.lengths.tolist() == res2.lengths.tolist() == res3.lengths.tolist()
    assert res0.winners.tolist() == res1.winners.tolist() == res2.winners.tolist()
    assert seq0 == seq3 and reads0 == reads3 == res0.turns + 1 + 4
    assert "snk_pit_tally" not in seq0
    assert [c for c in seq1 if c != "snk_pit_tally"] == seq0
    assert seq1.count("snk_pit_tally") == res1.turns, "one launch per turn"
    assert all(seq1[i + 1] == "snk_engine_step_active_tape" for i, c in enumerate(seq1) if c == "snk_pit_tally")
    assert reads1 == reads0 + 2, "the tally's one copy: .cpu() and .numpy()"
    at = seq2.index("snk_engine_step_active_tape")
    assert seq2[at - 2:at + 2] == ["snk_pit_record_moves", "snk_pit_tally", "snk_engine_step_active_tape", "snk_pit_record_boards"]
    assert [c for c in seq2 if c != "snk_pit_tally" and not c.startswith("snk_pit_record_")] == seq0
    assert seq2.count("snk_pit_tally") == res2.turns and reads2 == reads0 + 4
    for name in FIELDS:
        assert np.array_equal(getattr(tal1, name), getattr(tal2, name))
    assert (tal1.fate > 0).sum() >= n and tal1.died.max() == res1.turns
