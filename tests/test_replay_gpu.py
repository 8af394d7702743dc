"""GPU tests of the replay recorder (snake_engine/replay.py; snk_pit_record_slots / _moves / _boards).  The kernels alone: the two
replays the unmodified reference recorded (tests/golden/replay.npz) byte for byte, every tick of the golden trajectories and the
hand-built boards of tests/test_replay_cpu.py against the CPU statement (tests/replay_ref.py), wrapped rings, slot lists of every
size around a wavefront's and a block's, closed games, and canaries around the log and in the stride padding.  Then whole matches
through Arena.match, League.play and League.play_search -- stub nets, a Searcher, a Scripted -- against the statement's players
with every frame of every recorded game exact, the log's growth, and the launch and read-back counts."""
import functools

import numpy as np
import pytest

import league_ref as LR
import league_search_ref as LSR
import replay_ref as RR
import script_ref as SC
import search_pit_ref as SR
import test_replay_cpu as TC
from conftest import golden_state, load_golden
from pit_calls import Calls as _Calls

pytestmark = pytest.mark.gpu

CANARY = 85
GUARD = 256
GOLDEN = ["5x5x2", "7x7x2", "9x9x3", "11x11x4", "11x11x4_dec9", "15x15x5", "16x16x6", "19x19x8"]
KEYS = LR.KEYS


# ---- the kernels through the entry points alone ---------------------------------------------------------------------------------
def _engine_with(H, W, S, boards, ring_start=0):
    from snake_engine import Engine
    from snake_engine.engine import state_from_compact
    eng = Engine(len(boards), H, W, S, 1, 0.15, seed=1)
    eng.import_states([state_from_compact(H, W, S, st) for st in boards], ring_start=ring_start)
    return eng


def _boards(eng):
    from snake_engine.engine import compact_from_state
    return [compact_from_state(s) for s in eng.export()]


def record_ticks(eng, slots, ticks):
    """the recorder's turn, `ticks` times: ticks yields (live uint8[n], moves uint8[n][S], spawn int16[n] or None).  Returns
    int8[T][r][2][H*W] with CANARY wherever nothing was written.  The log lies between two guard zones and its frames keep
    their stride padding: both must still hold the canary afterwards, and so must both frames of a game whose flag was 0"""
    import torch
    from snake_engine._lib import check
    L, n, S, nc = eng.L, eng.n_slots, eng.S, eng.H * eng.W
    stride = L.snk_pit_record_stride(eng.H, eng.W)
    assert stride == (nc + 15) // 16 * 16
    ticks = list(ticks)
    T, r = len(ticks), len(slots)
    h_slots = np.ascontiguousarray(slots, np.int32)
    d_slots = torch.full((r + 2,), -99, dtype=torch.int32, device="cuda")
    check(L.snk_pit_record_slots(eng.h, h_slots.ctypes.data, r, d_slots.data_ptr(), 0))
    buf = torch.full((GUARD + T * r * 2 * stride + GUARD,), CANARY, dtype=torch.int8, device="cuda")
    done = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    for t, (live, moves, spawn) in enumerate(ticks):
        d_live = torch.as_tensor(np.ascontiguousarray(live, np.uint8), device="cuda")
        d_moves = torch.as_tensor(np.ascontiguousarray(moves, np.uint8).reshape(n, S), device="cuda")
        d_spawn = None if spawn is None else torch.as_tensor(np.ascontiguousarray(spawn, np.int16), device="cuda")
        frames = buf.data_ptr() + GUARD + t * r * 2 * stride
        check(L.snk_pit_record_moves(eng.h, d_live.data_ptr(), d_slots.data_ptr(), r, d_moves.data_ptr(), frames, 0))
        check(L.snk_engine_step_active_tape(eng.h, d_live.data_ptr(), n, d_moves.data_ptr(), 0 if spawn is None else d_spawn.data_ptr(),
                                            done.data_ptr(), None, 0))
        check(L.snk_pit_record_boards(eng.h, d_live.data_ptr(), d_slots.data_ptr(), r, frames, 0))
    torch.cuda.synchronize()
    assert d_slots.cpu().numpy().tolist() == list(h_slots) + [-99, -99]
    host = buf.cpu().numpy()
    assert (host[:GUARD] == CANARY).all() and (host[-GUARD:] == CANARY).all(), "a byte outside the log was written"
    log = host[GUARD:-GUARD].reshape(T, r, 2, stride)
    assert (log[..., nc:] == CANARY).all(), "the stride padding was written"
    for t, (live, _, _) in enumerate(ticks):
        for i, g in enumerate(slots):
            if not live[g]:
                assert (log[t, i] == CANARY).all(), f"tick {t}: the frames of closed game {g} were touched"
    return log[..., :nc]


def _shaped(frames, H, W):
    return np.asarray(frames, np.int8).reshape(-1, H, W)


@pytest.mark.parametrize("ci", [0, 1])
def test_the_recorded_reference_replays_through_the_entry_points(ci):
    from snake_engine.replay import frames_text
    z = load_golden("replay.npz")
    p = f"r{ci}_"
    H, W, S, hd = (int(v) for v in z[p + "meta"])
    want = z[p + "text"].tobytes()
    T = want.count(b"\n\n") // 2
    assert 10 <= T <= len(z[p + "moves"])
    eng = _engine_with(H, W, S, [{k: z[p + "init_" + k][0] for k in KEYS}])
    eng.set_params(hd, 0.15)
    log = record_ticks(eng, [0], [(np.ones(1, np.uint8), z[p + "moves"][t], z[p + "spawn"][t]) for t in range(T)])
    frames = _shaped(log, H, W)
    assert frames_text(frames) == want and RR.text(frames) == want


@pytest.mark.parametrize("cfg", GOLDEN)
def test_every_tick_of_the_golden_trajectories(cfg):
    """the trajectories of a file in lock step, one game each, recorded in descending slot order; a trajectory that is over is a
    closed game among the recorded ones"""
    z = load_golden(f"tic_{cfg}.npz")
    H, W, S, hd = int(z["H"]), int(z["W"]), int(z["S"]), int(z["health_dec"])
    ptr = z["ptr"]
    G = len(ptr) - 1
    T = [int(ptr[g + 1] - ptr[g] - 1) for g in range(G)]
    eng = _engine_with(H, W, S, [golden_state(z, ptr[g]) for g in range(G)])
    eng.set_params(hd, float(z["food_chance"]))
    ticks = []
    for t in range(max(T)):
        live = np.array([t < T[g] for g in range(G)], np.uint8)
        idx = [int(ptr[g] - g + min(t, T[g] - 1)) for g in range(G)]
        ticks.append((live, z["moves"][idx], z["spawn"][idx]))
    slots = list(range(G))[::-1]
    log = record_ticks(eng, slots, ticks)
    checked = 0
    for t in range(max(T)):
        for i, g in enumerate(slots):
            if t < T[g]:
                mid, post = RR.tick_frames(H, W, golden_state(z, ptr[g] + t), ticks[t][1][g], golden_state(z, ptr[g] + t + 1))
                assert np.array_equal(log[t, i, 0].reshape(H, W), mid), f"{cfg} game {g} tick {t}: the mid-tick board"
                assert np.array_equal(log[t, i, 1].reshape(H, W), post), f"{cfg} game {g} tick {t}: the post-tick board"
                checked += 1
    assert checked == sum(T) >= 50


@pytest.mark.parametrize("ring_start", [0, -1, -3])
def test_hand_built_boards_and_wrapped_rings(ring_start):
    """the boards of tests/test_replay_cpu.py and the cells worked out by hand there; laid out from the ring's start, and from
    its last and third-last entry, so that every body wraps across the ring's end"""
    H, W = TC.H, TC.W
    cap = 1 << (H * W + 1).bit_length()
    assert cap // 2 < H * W + 2 <= cap
    for S in (2, 3, 4):
        names = [k for k, c in TC.CASES.items() if len(c["moves"]) == S]
        eng = _engine_with(H, W, S, [TC.CASES[k]["board"] for k in names], ring_start % cap)
        live = np.ones(len(names), np.uint8)
        log = record_ticks(eng, list(range(len(names))), [(live, np.stack([TC.CASES[k]["moves"] for k in names]),
                                                           np.array([TC.CASES[k]["spawn"] for k in names], np.int16))])
        for i, k in enumerate(names):
            for f, which in ((0, "mid"), (1, "post")):
                got, cells = log[0, i, f].reshape(H, W), TC.frame_of(TC.CASES[k][which])
                for y in range(H):
                    for x in range(W):
                        assert got[y, x] == cells[y, x], f"{k}: cell ({y}, {x}) of the {which}-tick board, ring start {ring_start}"
    assert sum(len(c["moves"]) in (2, 3, 4) for c in TC.CASES.values()) == len(TC.CASES)


@functools.lru_cache(maxsize=None)
def _played(n=150):
    """n 7x7 duels a few random ticks into play (some over, some with food eaten) -> the engine"""
    import torch
    from snake_engine import Engine
    eng = Engine(n, 7, 7, 2, 1, 0.15, seed=9)
    eng.reset()
    rng = np.random.RandomState(2)
    for _ in range(5):
        eng.step(torch.as_tensor(rng.randint(0, 3, size=(n, 2)).astype(np.uint8), device="cuda"))
    return eng


@pytest.mark.parametrize("r", [1, 2, 63, 64, 65])
def test_slot_lists_unsorted_subsets_and_closed_games(r):
    eng = _played()
    n = eng.n_slots
    rng = np.random.RandomState(100 + r)
    slots = sorted(rng.permutation(n)[:r].tolist(), reverse=True)       # a strict subset of the engine's games, descending
    if r > 2:
        slots[1], slots[-1] = slots[-1], slots[1]                        # and neither ascending nor descending
    live = (rng.rand(n) < 0.8).astype(np.uint8)
    live[slots[0]] = 0 if r > 1 else 1                                   # a closed game among the recorded ones
    moves = rng.randint(0, 3, size=(n, 2)).astype(np.uint8)
    pre = _boards(eng)
    log = record_ticks(eng, slots, [(live, moves, None)])
    post = _boards(eng)
    drawn = 0
    for i, g in enumerate(slots):
        if live[g]:
            mid, last = RR.tick_frames(7, 7, pre[g], moves[g], post[g])
            assert np.array_equal(log[0, i, 0].reshape(7, 7), mid) and np.array_equal(log[0, i, 1].reshape(7, 7), last), (r, g)
            drawn += 1
    assert drawn >= 1


def test_a_slot_outside_the_engine_or_given_twice_is_refused():
    import torch
    from snake_engine import EngineError
    from snake_engine._lib import check
    eng = _played()
    n = eng.n_slots
    d_slots = torch.full((4,), -99, dtype=torch.int32, device="cuda")
    for bad, word in (([0, n], "outside"), ([-1], "outside"), ([3, 5, 3], "twice"), (list(range(n)) + [0], "exceeds")):
        h = np.array(bad, np.int32)
        with pytest.raises(EngineError, match=word):
            check(eng.L.snk_pit_record_slots(eng.h, h.ctypes.data, len(bad), d_slots.data_ptr(), 0))
    with pytest.raises(EngineError, match="NULL"):
        check(eng.L.snk_pit_record_moves(eng.h, 0, d_slots.data_ptr(), 1, 0, 0, 0))
    check(eng.L.snk_pit_record_moves(eng.h, 0, 0, 0, 0, 0, 0))
    check(eng.L.snk_pit_record_boards(eng.h, 0, 0, 0, 0, 0))
    torch.cuda.synchronize()
    assert (d_slots.cpu().numpy() == -99).all()


# ---- whole matches against the statement --------------------------------------------------------------------------------------------
def _check_replay(rep, res, games, engine, recorded):
    """every frame of every recorded game against the statement's; 2 * lengths[g] frames; the last one draws the verdict board"""
    H, W = engine.H, engine.W
    boards = _boards(engine)
    assert rep.games.tolist() == list(recorded)
    for g in recorded:
        got, want = rep.frames(g), np.stack(games[g].frames)
        assert got.dtype == np.int8 and got.shape == (2 * int(res.lengths[g]), H, W) == want.shape, f"game {g}"
        bad = np.flatnonzero((got != want).any(axis=(1, 2)))
        assert len(bad) == 0, f"game {g}: frame {bad[0]} of {len(got)} differs"
        assert np.array_equal(got[-1], RR.draw(H, W, RR.food_of(W, boards[g]), RR.snakes_of(W, boards[g]))), f"game {g}: the verdict board"
        assert rep.text(g) == RR.text(want)
    with pytest.raises(KeyError):
        rep.frames(-5)


def _spawn(log):
    return lambda turn: np.maximum(log[turn - 1], -1)


@functools.lru_cache(maxsize=None)
def _pit_statement(ci=2):
    from oracle.obs_key import StubNet
    from oracle.pit_oracle import pit_run
    z, p, H, W, S, hd, n, a_cnt = LR.meta(ci)
    games = [RR.Recording(g) for g in LR.start_games(ci)]
    winners, lengths = pit_run(games, StubNet(0), StubNet(1), a_cnt, spawn_tape=lambda turn: z[p + "spawn"][turn - 1])
    return games, winners, lengths


def _pit_match(recorded, first_turns):
    from snake_engine.arena import Arena
    z, p, H, W, S, hd, n, a_cnt = LR.meta(2)
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(LR.start_states(2))
    rep = arena.record(recorded, first_turns=first_turns)
    res = arena.match(LR.DeviceStub(0), LR.DeviceStub(1), a_cnt, spawn_tape=lambda turn: z[p + "spawn"][turn - 1])
    assert arena._recorder is None, "the recorder is dropped when the match ends"
    return arena, rep, res


def test_a_recorded_reference_pit_through_arena_match_and_the_logs_growth():
    """recorded pit 2 of tests/golden/pit.npz with every game recorded and a log that starts at ONE turn; then the same match
    with an unsorted third of the games recorded: the shared games have the same frames"""
    games, winners, lengths = _pit_statement()
    n = len(games)
    arena, rep, res = _pit_match(range(n), 1)
    assert res.lengths.tolist() == lengths and res.winners.tolist() == [-1 if w is None else w for w in winners]
    assert res.turns >= 8 and rep.grown >= 3 and 2 ** rep.grown >= res.turns, "the log was doubled from one turn on"
    _check_replay(rep, res, games, arena.engine, list(range(n)))
    third = [11, 2, 7, 14, 0]
    arena2, rep2, res2 = _pit_match(third, 64)
    assert rep2.grown == 0 and res2.lengths.tolist() == lengths
    _check_replay(rep2, res2, games, arena2.engine, third)
    for g in third:
        assert np.array_equal(rep2.frames(g), rep.frames(g))


def test_a_match_with_a_searcher():
    """a committed seed of tests/search_pit_ref.py: team A searches, team B is greedy"""
    from oracle.obs_key import StubNet
    from snake_engine.arena import Arena, Searcher
    name = "7x7x2-b8-search-v-greedy"
    board, n, breadth, searching, seed = SR.CASES[name]
    bare, (H, W, S, hd) = SR.start_games(board, n)
    games = [RR.Recording(g) for g in bare]
    want = SR.search_pit_run(games, (StubNet(0), StubNet(1)), searching, 1, seed + 1000, SR.uniform_tape(seed), 4, breadth)
    SR.check_well_posed(want)
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(SR.start_states(board, n))
    rep = arena.record([5, 0, 3], first_turns=2)
    sides = (Searcher(SR.DeviceStub(0), breadth, 4, 100, seed=5, sequential=True, tape_u=SR.uniform_tape(seed)), SR.DeviceStub(1))
    res = arena.match(sides[0], sides[1], 1, spawn_tape=_spawn(want["spawn_log"]))
    assert res.lengths.tolist() == want["lengths"] and res.turns == want["turns"] and sides[0].tape_pos == want["tape_pos"][0]
    _check_replay(rep, res, games, arena.engine, [5, 0, 3])


def test_a_match_with_a_scripted_side():
    from snake_engine.arena import Arena, Scripted
    n = SC.N_DUEL
    bare, (H, W, S, hd) = SR.start_games("7x7x2", n)
    games = [RR.Recording(g) for g in bare]
    want = SC.script_run(games, [SC.RefScripted(), LR.RefStub(0)], LR.two_team_table(n, 2, 1), SC.SPAWN_SEED)
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(SR.start_states("7x7x2", n))
    recorded = list(range(n))[::-1]
    rep = arena.record(recorded)
    res = arena.match(Scripted(), LR.DeviceStub(0), 1, spawn_tape=_spawn(want["spawn_log"]))
    assert res.lengths.tolist() == want["lengths"] and res.turns == want["turns"] >= 5
    _check_replay(rep, res, games, arena.engine, recorded)


def test_league_play_with_three_stub_owners():
    from snake_engine.league import League
    z, p, H, W, S, hd, n, _ = LR.meta(2)
    games = [RR.Recording(g) for g in LR.start_games(2)]
    owner = LR.six_owner_table(n) % 3
    want = LR.league_run(games, [LR.RefStub(k) for k in range(3)], owner, food_seed=LR.FOOD_SEED)
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(LR.start_states(2))
    recorded = [9, 1, 15, 4]
    rep = league.record(recorded, first_turns=3)
    res = league.play([LR.DeviceStub(k) for k in range(3)], owner, spawn_tape=_spawn(want["spawn_log"]))
    assert league._recorder is None
    assert res.lengths.tolist() == want["lengths"] and res.turns == want["turns"] >= 5
    _check_replay(rep, res, games, league.engine, recorded)


def test_league_play_search():
    from snake_engine.arena import Searcher
    from snake_engine.league import League
    board, breadth, searching, seed = LSR.CASES["7x7x2-b8-gsg"]
    table = LSR.TABLES[board]()
    n, K = len(table), len(searching)
    bare, (H, W, S, hd) = SR.start_games(board, n)
    games = [RR.Recording(g) for g in bare]
    tapes = LSR.tapes(seed, K)
    want = LSR.league_search_run(games, [LR.RefStub(o) for o in range(K)], searching, table, seed + 1000, tapes, 4, breadth)
    LSR.check_well_posed(want)
    net = lambda o: SR.DeviceStub(o) if o < 2 else LR.DeviceStub(o)      # noqa: E731
    sides = [Searcher(net(o), breadth, 4, 100, seed=5 + o, sequential=True, tape_u=tapes[o]) if s else net(o)
             for o, s in enumerate(searching)]
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(SR.start_states(board, n))
    recorded = [4, 5, 1]
    rep = league.record(recorded, first_turns=1)
    res = league.play_search(sides, table, spawn_tape=_spawn(want["spawn_log"]))
    assert res.lengths.tolist() == want["lengths"] and res.turns == want["turns"]
    _check_replay(rep, res, games, league.engine, recorded)


# ---- launches and read-backs ---------------------------------------------------------------------------------------------------------
def test_launch_and_read_back_counts(monkeypatch):
    """three matches on the same start boards with the device's own food: before record was ever called, with a recorder, and
    after it.  The first and the third issue the same sequence of library calls; the second issues that sequence plus the slot
    list once and two launches per turn, and reads back once per turn as before plus the log's one copy at the end"""
    import torch
    from snake_engine.arena import Arena, Scripted
    n = 24
    arena = Arena(11, 11, 4, 1, n, seed=3)
    start = arena.engine.export()
    calls = arena.engine.L = _Calls(arena.engine.L)
    runs = []
    for recorded in (None, [20, 3, 8], None):
        arena.import_states(start)
        rep = None if recorded is None else arena.record(recorded, first_turns=1)
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
        runs.append((res, list(calls.names), count[0], rep))
    (res0, seq0, reads0, _), (res1, seq1, reads1, rep), (res2, seq2, reads2, _) = runs
    assert res0.turns == res1.turns == res2.turns >= 10
    assert res0.lengths.tolist() == res1.lengths.tolist() == res2.lengths.tolist()
    assert seq0 == seq2 and reads0 == reads2 == res0.turns + 1 + 4
    added = [c for c in seq1 if c.startswith("snk_pit_record_")]
    assert [c for c in seq1 if not c.startswith("snk_pit_record_")] == seq0
    assert added == ["snk_pit_record_slots"] + ["snk_pit_record_moves", "snk_pit_record_boards"] * res1.turns
    assert reads1 == reads0 + 2, "the log's one copy: .cpu() and .numpy()"
    at = seq1.index("snk_engine_step_active_tape")
    assert seq1[at - 1] == "snk_pit_record_moves" and seq1[at + 1] == "snk_pit_record_boards" and seq1[at + 3] == "snk_pit_verdict"
    assert rep.grown >= 4 and all(len(rep.frames(g)) == 2 * res1.lengths[g] for g in (20, 3, 8))
