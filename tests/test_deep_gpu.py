"""GPU tests of the deep opponent: snk_pit_deep_values against the CPU statement (tests/deep_ref.py), scores equal as integers --
depth 1 against snk_pit_look_values bit for bit; depth 2 on boards taken from the golden trajectories, imported at a ring start that
wraps; depths 3 and 4; every flag subset; edge rows, sizes and row orders, the sharing of the children, the refusals -- then whole
matches through Arena.match and League.play against the statement's match player, and the launch and read-back counts.

Matches on 11x11x4 are cut at a turn cap the statement shares: the spawn tape of the turn after the cap raises, which leaves the
device boards where the statement's stand (the turn loop has no cap of its own)."""
import ctypes as C
import functools
import sys

import numpy as np
import pytest

import deep_ref as D
import league_ref as LR
import look_ref as K
import script_ref as R
import search_pit_ref as SR
from pit_calls import Calls

pytestmark = pytest.mark.gpu

HOST_ONLY = ("snk_pit_look_fanout", "snk_pit_deep_fanout", "snk_pit_deep_scratch_elems")      # sizes asked of the library: no launch
BAD = [(-1, 0), (1 << 20, 0), (0, 2), (0, -1), (1 << 30, 1), (-(1 << 31), 1), (3, 1 << 30), (0, 8)]


def _engine_of(H, W, S, hd, boards, wrap=True):
    """boards in an engine, every ring laid out so that it runs across the ring's end"""
    from snake_engine import Engine
    from snake_engine.engine import state_from_compact
    cap = 1 << (H * W + 1).bit_length()
    assert cap // 2 < H * W + 2 <= cap
    eng = Engine(len(boards), H, W, S, hd, 0.15, seed=1)
    eng.import_states([state_from_compact(H, W, S, st) for st in boards], ring_start=cap - 2 if wrap else 0)
    return eng


@functools.lru_cache(maxsize=None)
def _engine_with(cfg):
    return _engine_of(*D.sampled(cfg))


def _subs(eng, groups, depth):
    """sub-engines of exactly groups * F^k slots"""
    from snake_engine import Engine
    F = eng.L.snk_pit_look_fanout(eng.S)
    return [Engine(max(groups, 1) * F ** k, eng.H, eng.W, eng.S, eng.health_dec, 0, seed=0) for k in range(1, depth + 1)]


def _call(eng, subs, depth, d_pairs, m, flags, d_scratch, d_q, L=None):
    from snake_engine._lib import check
    handles = (C.c_void_p * len(subs))(*[None if s is None else s.h.value for s in subs])
    check((L or eng.L).snk_pit_deep_values(eng.h, handles, depth, d_pairs, m, flags, d_scratch, d_q, 0))


def _raw(eng, subs, depth, pairs, flags=R.ALL, extra=3):
    """snk_pit_deep_values over int pairs [m][2] -> float32[m][3]; the `extra` NaN rows past m must stay NaN"""
    import torch
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    m = len(pairs)
    d_pairs = torch.as_tensor(pairs, device="cuda") if m else None
    elems = eng.L.snk_pit_deep_scratch_elems(m, eng.S, depth)
    assert elems >= 0
    scratch = torch.empty((max(elems, 1),), dtype=torch.int32, device="cuda")
    q = torch.full((m + extra, 3), float("nan"), dtype=torch.float32, device="cuda")
    _call(eng, subs, depth, d_pairs.data_ptr() if m else 0, m, flags, scratch.data_ptr() if m else 0, q.data_ptr() if m else 0)
    torch.cuda.synchronize()
    out = q.cpu().numpy()
    assert np.isnan(out[m:]).all(), "a row past m was written"
    return out[:m]


def _values(eng, subs, depth, pairs, flags=R.ALL):
    out = _raw(eng, subs, depth, pairs, flags)
    assert np.array_equal(out, np.round(out)), "a score is no integer"
    return out.astype(np.int64)


def _alive_pairs(boards):
    return np.array([(g, s) for g, st in enumerate(boards) for s in range(len(st["alive"])) if st["alive"][s]], np.int32)


def _want(cfg, depth, pairs, flags=R.ALL):
    """the statement's rows; -1, -1, -1 for a dead snake and for a slot or id out of range"""
    boards = D.sampled(cfg)[4]
    scores = D.sampled_scores(cfg, depth, flags)
    return np.array([scores[g].get(s, [-1] * 3) if 0 <= g < len(boards) else [-1] * 3 for g, s in np.asarray(pairs).tolist()],
                    np.int64).reshape(-1, 3)


def _same(got, want, pairs, what):
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(pairs)} rows differ, first {pairs[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"


# ---- 1. depth 1 is the lookahead, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["7x7x2", "9x9x3", "11x11x4"])
def test_depth_one_is_snk_pit_look_values_bit_for_bit(cfg):
    """the two entry points run one body since the lookahead became the deep search at depth 1, so this compares a path with
    itself (two names, two argument lists); the exact pin of the scores is the integer comparison with look_ref in test_look_gpu"""
    import torch
    from snake_engine._lib import check
    H, W, S, hd, boards = K.sampled(cfg)
    eng = _engine_of(H, W, S, hd, boards)
    subs = _subs(eng, len(boards), 1)
    pairs = np.concatenate([_alive_pairs(boards), np.array(BAD, np.int32)])
    m = len(pairs)
    got = _raw(eng, subs, 1, pairs)
    d_pairs = torch.as_tensor(pairs, device="cuda")
    scratch = torch.empty((eng.L.snk_pit_look_scratch_elems(m, S),), dtype=torch.int32, device="cuda")
    q = torch.full((m, 3), float("nan"), dtype=torch.float32, device="cuda")
    check(eng.L.snk_pit_look_values(eng.h, subs[0].h, d_pairs.data_ptr(), m, R.ALL, scratch.data_ptr(), q.data_ptr(), 0))
    torch.cuda.synchronize()
    assert got.tobytes() == q.cpu().numpy().tobytes() and (got[:-len(BAD)] != -1).any()


# ---- 2. depth 2 against the statement, cell for cell ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["7x7x2", "5x5x2", "9x9x3", "11x11x4", "16x16x6"])
def test_depth_two_on_golden_boards(cfg):
    """7x7x2 and 5x5x2: 81 children a board; 9x9x3: 729; 11x11x4 and the first 16x16x6 board, four alive: 6 561; the second
    16x16x6 board has five alive and gets the plain scores"""
    H, W, S, hd, boards = D.sampled(cfg)
    eng = _engine_with(cfg)
    assert eng.L.snk_pit_deep_fanout(S, 2) == D.fanout(S, 2) == K.fanout(S) ** 2
    pairs = _alive_pairs(boards)
    got, want = _values(eng, _subs(eng, len(boards), 2), 2, pairs), _want(cfg, 2, pairs)
    _same(got, want, pairs, cfg)
    assert got.min() >= D.low(2) and got.max() <= D.WIN
    if cfg == "16x16x6":
        assert [int(np.count_nonzero(st["alive"])) for st in boards] == [4, 5]
        plain = np.array([R.scores(H, W, boards[1], s) for g, s in pairs if g == 1], np.int64)
        assert np.array_equal(got[pairs[:, 0] == 1], plain)
    elif cfg in ("7x7x2", "9x9x3"):
        assert (got <= -35).any() and (got >= 0).any()


@pytest.mark.parametrize("depth", [3, 4])
def test_depths_three_and_four_on_four_boards(depth):
    H, W, S, hd, boards = D.sampled("7x7x2")
    pick = [0, 9, 18, 27]
    few = [boards[i] for i in pick]
    eng = _engine_of(H, W, S, hd, few)
    pairs = _alive_pairs(few)
    want = np.array([D.deep_scores(H, W, S, hd, few[g], s, depth) for g, s in pairs.tolist()], np.int64)
    got = _values(eng, _subs(eng, len(few), depth), depth, pairs)
    _same(got, want, pairs, f"depth {depth}")
    assert got.min() >= D.low(depth) and len(pairs) >= 6


def test_every_flag_subset_at_depth_two():
    H, W, S, hd, boards = D.sampled("7x7x2")
    eng = _engine_with("7x7x2")
    subs = _subs(eng, len(boards), 2)
    pairs = _alive_pairs(boards)
    seen = set()
    for flags in range(8):
        got = _values(eng, subs, 2, pairs, flags)
        _same(got, _want("7x7x2", 2, pairs, flags), pairs, f"flags {flags}")
        seen.add(got.tobytes())
    assert len(seen) == 8


# ---- 3. sentinels, edge inputs, row orders -----------------------------------------------------------------------------------------
CFG = "7x7x2"


@functools.lru_cache(maxsize=None)
def _edge():
    eng = _engine_with(CFG)
    return eng, _subs(eng, 257, 2)


@pytest.mark.parametrize("m", [0, 1, 2, 255, 256, 257])
def test_row_counts_with_dead_and_out_of_range_pairs(m):
    """random rows, dead snakes among them, a tenth of them out of range; almost every row is a group of its own.  The source
    engine's records are the same bytes afterwards"""
    H, W, S, hd, boards = D.sampled(CFG)
    eng, subs = _edge()
    n = len(boards)
    rng = np.random.RandomState(5 + m)
    pairs = np.stack([rng.randint(0, n, m), rng.randint(0, S, m)], 1).astype(np.int32)
    hit = rng.rand(m) < 0.1
    pairs[hit] = np.array(BAD, np.int32)[rng.randint(0, len(BAD), int(hit.sum()))]
    before = bytes(eng.export())
    got = _values(eng, subs, 2, pairs)
    assert bytes(eng.export()) == before, "the source engine was written"
    assert np.array_equal(got, _want(CFG, 2, pairs)), m
    if m >= 255:
        dead = np.array([not (0 <= g < n and 0 <= s < S and boards[g]["alive"][s]) for g, s in pairs.tolist()])
        assert dead.any() and (got[dead] == -1).all() and (got[~dead] != -1).any()


def test_only_dead_and_out_of_range_pairs():
    H, W, S, hd, boards = K.sampled(CFG)                    # look_ref's boards: the ends of the games are among them
    eng = _engine_of(H, W, S, hd, boards)
    subs = _subs(eng, len(boards), 2)
    dead = np.array([(g, s) for g, st in enumerate(boards) for s in range(S) if not st["alive"][s]], np.int32)
    assert len(dead) >= 5
    assert (_values(eng, subs, 2, dead) == -1).all()
    assert (_values(eng, subs, 2, np.array(BAD, np.int32)) == -1).all()


def test_three_teammates_share_the_children_of_their_game():
    """a 1 v 3: the rows of snakes 1, 2 and 3 of every board, sub-engines of exactly boards * F^k slots -- three rows a group"""
    H, W, S, hd, boards = D.sampled("11x11x4")
    eng = _engine_with("11x11x4")
    pairs = np.array([(g, s) for g, st in enumerate(boards) for s in (1, 2, 3) if st["alive"][s]], np.int32)
    assert len(pairs) > len(boards) >= 2 and any(np.count_nonzero(st["alive"]) == 4 for st in boards)
    subs = _subs(eng, len(boards), 2)
    assert [s.n_slots for s in subs] == [len(boards) * 81, len(boards) * 6561]
    _same(_values(eng, subs, 2, pairs), _want("11x11x4", 2, pairs), pairs, "teammates")


def test_a_slot_repeated_later_and_split_slots_give_the_same_scores():
    """the rows ordered by snake id first: every slot stands in two places and is cloned for each"""
    H, W, S, hd, boards = D.sampled(CFG)
    eng, subs = _edge()
    pairs = _alive_pairs(boards)
    split = pairs[np.lexsort((pairs[:, 0], pairs[:, 1]))]
    assert (np.diff(split[:, 0]) < 0).sum() >= 1 and len(split) <= 257
    _same(_values(eng, subs, 2, split), _want(CFG, 2, split), split, "split")
    twice = np.concatenate([pairs[:20], pairs[:20]])
    _same(_values(eng, subs, 2, twice), _want(CFG, 2, twice), twice, "repeated")


def test_groups_beyond_the_sub_engines_get_minus_one():
    """the documented limit: the list names every slot twice, the sub-engines hold one group per slot"""
    H, W, S, hd, boards = D.sampled(CFG)
    eng = _edge()[0]
    pairs = _alive_pairs(boards)
    got = _values(eng, _subs(eng, len(boards), 2), 2, np.concatenate([pairs, pairs]))
    assert np.array_equal(got[:len(pairs)], _want(CFG, 2, pairs)) and (got[len(pairs):] == -1).all()


def test_a_chunk_boundary_inside_a_game(monkeypatch):
    """Deep.q_rows with a budget of five rows a call: boundaries fall inside games, which are cloned again"""
    import torch
    from snake_engine import arena as A
    H, W, S, hd, boards = D.sampled(CFG)
    eng = _edge()[0]
    pairs = torch.as_tensor(_alive_pairs(boards), device="cuda")
    whole = A.Deep()
    one = whole.q_rows(eng, pairs)
    assert [s.n_slots for s in whole._subs] == [len(boards) * 9, len(boards) * 81]
    budget = 5 * (9 + 81) * eng.slot_bytes + 7
    monkeypatch.setattr(A, "DEEP_BYTE_BUDGET", budget)
    small = A.Deep()
    many = small.q_rows(eng, pairs)
    torch.cuda.synchronize()
    assert [s.n_slots for s in small._subs] == [5 * 9, 5 * 81] and sum(s.n_slots * s.slot_bytes for s in small._subs) <= budget
    assert all(s.food_spawn_chance == 0 for s in small._subs)
    assert torch.equal(one, many) and np.array_equal(one.cpu().numpy().astype(np.int64), _want(CFG, 2, pairs.cpu().numpy()))
    per_game = np.bincount(pairs[:, 0].cpu().numpy())
    assert (np.cumsum(per_game) % 5 != 0).any() and per_game.max() >= 2


def test_a_depth_the_board_cannot_have_is_refused_at_first_use():
    import torch
    from snake_engine import EngineError
    from snake_engine.arena import Deep
    eng = _engine_with("9x9x3")
    pairs = torch.as_tensor(_alive_pairs(D.sampled("9x9x3")[4]), device="cuda")
    with pytest.raises(EngineError, match="depth"):
        Deep(depth=3).q_rows(eng, pairs)


def test_refusals():
    """every refusal is an error before any launch: the scores stay NaN and the sub-engines' records are the bytes they were"""
    import torch
    from snake_engine import Engine, EngineError
    H, W, S, hd, boards = D.sampled(CFG)
    eng = _edge()[0]
    n, F = len(boards), 9
    pairs = torch.as_tensor(_alive_pairs(boards), device="cuda")
    m = int(pairs.shape[0])
    assert m > n
    scratch = torch.empty((eng.L.snk_pit_deep_scratch_elems(m, S, 2),), dtype=torch.int32, device="cuda")
    q = torch.full((m, 3), float("nan"), dtype=torch.float32, device="cuda")
    ok = _subs(eng, n, 2)
    held = [bytes(s.export()) for s in ok]
    calls = Calls(eng.L)
    args = (pairs.data_ptr(), m, R.ALL, scratch.data_ptr(), q.data_ptr())
    mk = lambda slots, h=H, s=S, dec=hd, food=0: Engine(slots, h, h, s, dec, food, seed=0)
    for subs, what in (([mk(n * F - 1), ok[1]], "slots"), ([ok[0], mk(n * F * F - 1)], "slots"),     # one slot too small
                       ([mk(n * F, h=9), ok[1]], "geometry"), ([ok[0], mk(n * F * F, s=3)], "geometry"),
                       ([ok[0], mk(n * F * F, food=0.15)], "food"), ([mk(n * F, dec=hd + 1), ok[1]], "health_dec"),
                       ([eng, ok[1]], "itself"), ([ok[0], eng], "itself"), ([ok[1], ok[1]], "same"), ([ok[0], None], "NULL")):
        with pytest.raises(EngineError, match=what):
            _call(eng, subs, 2, *args, L=calls)
    for depth in (0, -1, 5):
        with pytest.raises(EngineError, match="depth"):
            _call(eng, (ok * 3)[:max(depth, 1)], depth, *args, L=calls)
    for bad in ((0, m, R.ALL, scratch.data_ptr(), q.data_ptr()), (pairs.data_ptr(), m, R.ALL, 0, q.data_ptr()),
                (pairs.data_ptr(), m, R.ALL, scratch.data_ptr(), 0), (pairs.data_ptr(), -1, R.ALL, scratch.data_ptr(), q.data_ptr()),
                (pairs.data_ptr(), m, 8, scratch.data_ptr(), q.data_ptr()), (pairs.data_ptr(), m, 1 << 31, scratch.data_ptr(), q.data_ptr())):
        with pytest.raises(EngineError):
            _call(eng, ok, 2, *bad, L=calls)
    from snake_engine._lib import check
    with pytest.raises(EngineError):
        check(calls.snk_pit_deep_values(eng.h, None, 2, *args, 0))
    torch.cuda.synchronize()
    assert calls.names == ["snk_pit_deep_values"] * 20, "a refused call went on to another entry point"
    assert np.isnan(q.cpu().numpy()).all(), "a refused call wrote"
    assert [bytes(s.export()) for s in ok] == held, "a refused call launched on a sub-engine"
    _call(eng, ok, 2, 0, 0, R.ALL, 0, 0)                                      # m = 0 is a no-op, its buffers may be NULL
    _call(eng, ok, 2, *args)                                                  # and the call still works after the refusals
    torch.cuda.synchronize()
    assert np.array_equal(q.cpu().numpy().astype(np.int64), _want(CFG, 2, pairs.cpu().numpy()))


# ---- 4. whole matches against the statement -------------------------------------------------------------------------------------
class _Cut(Exception):
    pass


def _spawn(want, cap=None):
    log = want["spawn_log"]

    def tape(turn):
        if cap is not None and turn > cap:
            raise _Cut
        return np.maximum(log[turn - 1], -1)
    return tape


def _check_boards(boards, want):
    for g, (a, b) in enumerate(zip(boards, want["boards"])):
        for k in R.KEYS:
            assert np.array_equal(a[k], b[k]), f"game {g} ({want['lengths'][g]} turns): {k}"


def _reads(monkeypatch, play):
    """play() -> (its result, the read-backs made in arena.py / league.py)"""
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


def test_deep_against_lookahead_through_arena_match(monkeypatch):
    from snake_engine.arena import Arena, Deep, Lookahead
    from snake_engine.engine import compact_from_state
    want = D.reference("duel-7x7x2")
    H, W, S, hd = want["geometry"]
    n = D.N_DUEL
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(SR.start_states("7x7x2", n))
    res, reads = _reads(monkeypatch, lambda: arena.match(Deep(depth=2), Lookahead(), 1, spawn_tape=_spawn(want)))
    assert res.turns == want["turns"] >= 10
    assert res.winners.tolist() == [-1 if w is None else w for w in want["winners"]]
    assert res.lengths.tolist() == want["lengths"]
    _check_boards([compact_from_state(s) for s in arena.engine.export()], want)
    assert reads[:-1] == want["counts"] and not any(reads[-1]), "a turn's read-back"
    assert res.wins_a + res.wins_b + res.draws == n


def _after_the_cut(pit, want):
    """the pit's own state where the cut left it: the boards, and the verdicts that came in before the cap"""
    from snake_engine.engine import compact_from_state
    _check_boards([compact_from_state(s) for s in pit.engine.export()], want)
    closed = [g for g in range(len(want["lengths"])) if g not in want["open"]]
    assert pit._winner.cpu().numpy()[closed].tolist() == [-1 if want["winners"][g] is None else want["winners"][g] for g in closed]
    assert pit._length.cpu().numpy()[closed].tolist() == [want["lengths"][g] for g in closed]
    assert pit._live.cpu().numpy().astype(bool).tolist() == [g in want["open"] for g in range(len(want["lengths"]))]


def test_one_deep_against_three_scripted_through_arena_match():
    from snake_engine.arena import Arena, Deep, Scripted
    want = D.reference("1v3-11x11x4")
    H, W, S, hd = want["geometry"]
    n, cap = D.N_FOUR, D.CAP_FOUR
    assert want["turns"] == cap
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(SR.start_states("11x11x4", n))
    with pytest.raises(_Cut):
        arena.match(Deep(depth=2), Scripted(), 1, spawn_tape=_spawn(want, cap))
    _after_the_cut(arena, want)


def test_a_deep_owner_a_scripted_owner_and_a_stub_net_through_league_play():
    """with a recorder and a tally beside it (their launches run every turn; the cut comes before their one copy)"""
    from stubnet_device import DeviceStubNNet
    from snake_engine.arena import Deep, Scripted
    from snake_engine.league import League
    want = D.reference("league-11x11x4")
    H, W, S, hd = want["geometry"]
    n, cap = D.N_LEAGUE, D.CAP_LEAGUE
    counts = []
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(SR.start_states("11x11x4", n))
    league.record([0, n - 1]), league.tally()
    with pytest.raises(_Cut):
        league.play([Deep(depth=2), Scripted(R.SPACE), DeviceStubNNet()], R.three_owner_table(n), counts_log=counts,
                    spawn_tape=_spawn(want, cap))
    assert counts[:cap] == want["counts"] and len(counts) == cap + 1 and all(c > 0 for c in want["counts"][0])
    _after_the_cut(league, want)


# ---- 5. launches and read-backs ---------------------------------------------------------------------------------------------------
def test_the_calls_and_read_backs_of_a_deep_match(monkeypatch):
    """Deep against Deep: per turn the row list, one snk_pit_deep_values per side, snk_pit_moves, the tick and the verdict -- no
    observe launch, no net; one .tolist() per turn and the one that sees nothing left; and over the whole match no Tensor.cpu /
    .item / .tolist / .numpy but those and the result's"""
    import torch
    from snake_engine.arena import Arena, Deep
    n = 24
    arena = Arena(7, 7, 2, 1, n, seed=3)
    calls = arena.engine.L = Calls(arena.engine.L)
    sides = (Deep(), Deep(R.FOOD, 3))
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
        res = arena.match(sides[0], sides[1], 1)
    turn = ["snk_pit_rows", "snk_pit_deep_values", "snk_pit_deep_values", "snk_pit_moves", "snk_engine_step_active_tape",
            "snk_engine_rewards", "snk_pit_verdict"]
    assert res.turns >= 5 and [c for c in calls.names if c not in HOST_ONLY] == turn * res.turns + ["snk_pit_rows"]
    assert count[0] == res.turns + 1 + 4, "the turn's read-back, the one that sees nothing left, winners and lengths"
    assert res.wins_a + res.wins_b + res.draws == n and res.lengths.max() == res.turns
    assert [s.n_slots for s in sides[0]._subs] == [n * 9, n * 81] and [s.n_slots for s in sides[1]._subs] == [n * 9, n * 81, n * 729]
