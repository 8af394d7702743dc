"""GPU tests of the lookahead opponent: snk_pit_look_values against the CPU statement (tests/look_ref.py: the C game of oracle/ for
the children, the queue flood fill of tests/script_ref.py for the leaves), scores equal as integers -- on boards taken at a stride
from the golden trajectories, imported at a ring start that wraps; on edge rows, sizes and row orders, with the refusals -- then
whole matches through Arena.match and League.play against the statement's match player, and the launch and read-back counts."""
import ctypes as C
import functools
import sys

import numpy as np
import pytest

import league_ref as LR
import look_ref as K
import script_ref as R
import search_pit_ref as SR
from pit_calls import Calls

pytestmark = pytest.mark.gpu

HOST_ONLY = ("snk_pit_look_fanout", "snk_pit_look_scratch_elems")      # sizes asked of the library: no launch, no device work


def _engine_with(cfg, wrap=True):
    """the sampled boards of a golden configuration in an engine, every ring laid out so that it runs across the ring's end"""
    from snake_engine import Engine
    from snake_engine.engine import state_from_compact
    H, W, S, hd, boards = K.sampled(cfg)
    cap = 1 << (H * W + 1).bit_length()
    assert cap // 2 < H * W + 2 <= cap
    eng = Engine(len(boards), H, W, S, hd, 0.15, seed=1)
    eng.import_states([state_from_compact(H, W, S, st) for st in boards], ring_start=cap - 2 if wrap else 0)
    return eng


def _sub(eng, groups):
    from snake_engine import Engine
    F = eng.L.snk_pit_look_fanout(eng.S)
    return Engine(max(groups, 1) * F, eng.H, eng.W, eng.S, eng.health_dec, 0, seed=0)


def _call(eng, sub, d_pairs, m, flags, d_scratch, d_q):
    from snake_engine._lib import check
    check(eng.L.snk_pit_look_values(eng.h, sub.h, d_pairs, m, flags, d_scratch, d_q, 0))


def _values(eng, sub, pairs, flags=R.ALL, extra=3):
    """snk_pit_look_values over int pairs [m][2] -> int64[m][3]; the `extra` NaN rows past m must stay NaN"""
    import torch
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    m = len(pairs)
    d_pairs = torch.as_tensor(pairs, device="cuda") if m else None
    elems = eng.L.snk_pit_look_scratch_elems(m, eng.S)
    assert elems >= 0
    scratch = torch.empty((max(elems, 1),), dtype=torch.int32, device="cuda")
    q = torch.full((m + extra, 3), float("nan"), dtype=torch.float32, device="cuda")
    _call(eng, sub, d_pairs.data_ptr() if m else 0, m, flags, scratch.data_ptr() if m else 0, q.data_ptr() if m else 0)
    torch.cuda.synchronize()
    out = q.cpu().numpy()
    assert np.isnan(out[m:]).all(), "a row past m was written"
    assert np.array_equal(out[:m], np.round(out[:m])), "a score is no integer"
    return out[:m].astype(np.int64)


def _alive_pairs(boards):
    return np.array([(g, s) for g, st in enumerate(boards) for s in range(len(st["alive"])) if st["alive"][s]], np.int32)


def _want(cfg, pairs, flags=R.ALL):
    """the statement's rows; -1, -1, -1 for a dead snake and for a slot or id out of range"""
    H, W, S, hd, boards = K.sampled(cfg)
    scores = K.sampled_scores(cfg, flags)
    return np.array([scores[g].get(s, [-1] * 3) if 0 <= g < len(boards) else [-1] * 3 for g, s in np.asarray(pairs).tolist()],
                    np.int64).reshape(-1, 3)


# ---- 1. the entry point against the statement, cell for cell ---------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(K.STRIDE))
def test_sampled_golden_boards(cfg):
    """7x7x2: F = 9 and every flag subset; 9x9x3: F = 27; 11x11x4: F = 81; 15x15x5 and 19x19x8: the plain scores while more than
    four snakes live, F = 81 afterwards"""
    H, W, S, hd, boards = K.sampled(cfg)
    eng = _engine_with(cfg)
    assert eng.L.snk_pit_look_fanout(S) == K.fanout(S)
    sub = _sub(eng, len(boards))
    pairs = _alive_pairs(boards)
    assert len(pairs) >= 60
    for flags in (range(8) if cfg == "7x7x2" else (R.ALL,)):
        got, want = _values(eng, sub, pairs, flags), _want(cfg, pairs, flags)
        bad = np.flatnonzero((got != want).any(1))
        assert len(bad) == 0, f"{cfg} flags {flags}: {len(bad)} of {len(pairs)} rows differ, first {pairs[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"
    assert got.min() >= K.LOW and got.max() <= K.HIGH and (got <= -3).any() and (got >= 0).any()
    alive = np.array([np.count_nonzero(st["alive"]) for st in boards])
    if S > 4:
        many = np.isin(pairs[:, 0], np.flatnonzero(alive > 4))
        assert many.any() and (~many).any(), "both the fallback and the full fanout"
        plain = np.array([R.scores(H, W, boards[g], s) for g, s in pairs[many]], np.int64)
        assert np.array_equal(got[many], plain) and (got[~many] <= -3).any()


# ---- 2. sentinels and edge inputs ---------------------------------------------------------------------------------------------------
CFG = "11x11x4"
BAD = [(-1, 0), (1 << 20, 0), (0, 4), (0, -1), (1 << 30, 1), (-(1 << 31), 2), (3, 1 << 30), (0, 8)]


@functools.lru_cache(maxsize=None)
def _edge():
    eng = _engine_with(CFG)
    return eng, _sub(eng, 1000)


@pytest.mark.parametrize("m", [0, 1, 2, 63, 64, 65, 1000])
def test_row_counts_with_dead_and_out_of_range_pairs(m):
    """random rows, dead snakes among them, a tenth of them out of range; almost every row is a group of its own.  The source
    engine's records are the same bytes afterwards"""
    H, W, S, hd, boards = K.sampled(CFG)
    eng, sub = _edge()
    n = len(boards)
    rng = np.random.RandomState(5 + m)
    pairs = np.stack([rng.randint(0, n, m), rng.randint(0, S, m)], 1).astype(np.int32)
    hit = rng.rand(m) < 0.1
    pairs[hit] = np.array(BAD, np.int32)[rng.randint(0, len(BAD), int(hit.sum()))]
    before = bytes(eng.export())
    got = _values(eng, sub, pairs)
    assert bytes(eng.export()) == before, "the source engine was written"
    assert np.array_equal(got, _want(CFG, pairs)), m
    if m >= 63:
        dead = np.array([not (0 <= g < n and 0 <= s < S and boards[g]["alive"][s]) for g, s in pairs.tolist()])
        assert dead.any() and (got[dead] == -1).all() and (got[~dead] != -1).any()


def test_only_dead_and_out_of_range_pairs():
    H, W, S, hd, boards = K.sampled(CFG)
    eng, sub = _edge()
    dead = np.array([(g, s) for g, st in enumerate(boards) for s in range(S) if not st["alive"][s]], np.int32)
    assert len(dead) >= 20
    assert (_values(eng, sub, dead) == -1).all()
    assert (_values(eng, sub, np.array(BAD, np.int32)) == -1).all()


def test_a_slot_whose_rows_are_split_gives_the_same_scores():
    """the rows ordered by snake id first: the rows of one slot stand in up to four places and the slot is cloned for each"""
    H, W, S, hd, boards = K.sampled(CFG)
    eng, sub = _edge()
    pairs = _alive_pairs(boards)
    split = pairs[np.lexsort((pairs[:, 0], pairs[:, 1]))]
    assert (np.diff(split[:, 0]) < 0).sum() >= 3 and len(split) <= 1000
    assert np.array_equal(_values(eng, sub, split), _want(CFG, split))
    assert np.array_equal(_values(eng, _sub(eng, len(boards)), pairs), _want(CFG, pairs))      # together: one group per slot


def test_groups_beyond_the_sub_engine_get_minus_one():
    """the documented limit: the list names every slot twice, the sub-engine holds one group per slot -- the second pass's groups
    lie beyond it, which no error can report without a read-back"""
    H, W, S, hd, boards = K.sampled(CFG)
    eng = _edge()[0]
    pairs = _alive_pairs(boards)
    got = _values(eng, _sub(eng, len(boards)), np.concatenate([pairs, pairs]))
    assert np.array_equal(got[:len(pairs)], _want(CFG, pairs)) and (got[len(pairs):] == -1).all()


def _four_kinds(cfg):
    """a pair list with every kind of row the fold tells apart, and the groups it forms: a dead pair, an out-of-range pair and
    (-1, -1), a group each, then every alive row, a group per board"""
    H, W, S, hd, boards = K.sampled(cfg)
    dead = [(g, s) for g, st in enumerate(boards) for s in range(S) if not st["alive"][s]][-1]
    pairs = np.concatenate([np.array([dead, (1 << 20, 0), (-1, -1)], np.int32), _alive_pairs(boards)])
    groups = 1 + int(np.count_nonzero(np.diff(pairs[:, 0])))
    return pairs, groups


@pytest.mark.parametrize("cfg", ["7x7x2", CFG])
def test_every_kind_of_row_in_one_call_through_a_sub_engine_one_group_short(cfg):
    """searched rows, rows that fall back (dead, out of range, (-1, -1), a lone survivor) and rows whose group the sub-engine
    does not hold, in one list: the last board's rows are not served and get -1, every other row the statement's integers"""
    H, W, S, hd, boards = K.sampled(cfg)
    pairs, groups = _four_kinds(cfg)
    assert groups == len(boards) + 3
    eng = _engine_with(cfg)
    got = _values(eng, _sub(eng, groups - 1), pairs)
    want = _want(cfg, pairs)
    last = pairs[:, 0] == len(boards) - 1
    last[0] = False                                                           # the dead pair may name the last board: it is group 0
    assert last.any() and (want[last] != -1).any() and (want[:3] == -1).all()
    alive = np.array([np.count_nonzero(st["alive"]) for st in boards])
    assert ((alive >= 2) & (alive <= 4))[:-1].any() and (alive < 2).any() == (cfg == "7x7x2"), "searched rows; 7x7x2: lone survivors too"
    want[last] = -1
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, f"{cfg}: {len(bad)} of {len(pairs)} rows differ, first {pairs[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"
    assert (got[~last] <= -3).any() and (got[~last] >= 0).any()


def test_refusals():
    import torch
    from snake_engine import Engine, EngineError
    H, W, S, hd, boards = K.sampled(CFG)
    eng = _edge()[0]
    n, F = len(boards), 81
    pairs = torch.as_tensor(_alive_pairs(boards), device="cuda")
    m = int(pairs.shape[0])
    assert m > n
    scratch = torch.empty((eng.L.snk_pit_look_scratch_elems(m, S),), dtype=torch.int32, device="cuda")
    q = torch.full((m, 3), float("nan"), dtype=torch.float32, device="cuda")
    ok = Engine(n * F, H, W, S, hd, 0, seed=0)
    args = (pairs.data_ptr(), m, R.ALL, scratch.data_ptr(), q.data_ptr())
    for sub, what in ((Engine(n * F - 1, H, W, S, hd, 0, seed=0), "slots"),              # one slot too small
                      (Engine(n * F, 9, 9, S, hd, 0, seed=0), "geometry"),
                      (Engine(n * F, H, W, 3, hd, 0, seed=0), "geometry"),
                      (Engine(n * F, H, W, S, hd, 0.15, seed=0), "food"),
                      (Engine(n * F, H, W, S, hd + 1, 0, seed=0), "health_dec"),
                      (eng, "itself")):
        with pytest.raises(EngineError, match=what):
            _call(eng, sub, *args)
    for bad in ((0, m, R.ALL, scratch.data_ptr(), q.data_ptr()), (pairs.data_ptr(), m, R.ALL, 0, q.data_ptr()),
                (pairs.data_ptr(), m, R.ALL, scratch.data_ptr(), 0), (pairs.data_ptr(), -1, R.ALL, scratch.data_ptr(), q.data_ptr()),
                (pairs.data_ptr(), m, 8, scratch.data_ptr(), q.data_ptr()), (pairs.data_ptr(), m, 1 << 31, scratch.data_ptr(), q.data_ptr())):
        with pytest.raises(EngineError):
            _call(eng, ok, *bad)
    torch.cuda.synchronize()
    assert np.isnan(q.cpu().numpy()).all(), "a refused call wrote"
    _call(eng, ok, 0, 0, R.ALL, 0, 0)                                         # m = 0 is a no-op, its buffers may be NULL
    _call(eng, ok, *args)                                                     # and the call still works after the refusals
    torch.cuda.synchronize()
    assert np.array_equal(q.cpu().numpy().astype(np.int64), _want(CFG, pairs.cpu().numpy()))


def test_a_chunk_boundary_inside_a_game(monkeypatch):
    """Lookahead.q_rows with a budget of five rows a call: boundaries fall inside games, which are cloned again"""
    import torch
    from snake_engine import arena as A
    H, W, S, hd, boards = K.sampled(CFG)
    eng = _edge()[0]
    pairs = torch.as_tensor(_alive_pairs(boards), device="cuda")
    whole = A.Lookahead()
    one = whole.q_rows(eng, pairs)
    assert whole._sub.n_slots == len(boards) * 81 <= A.LOOK_SLOT_BUDGET
    monkeypatch.setattr(A, "LOOK_SLOT_BUDGET", 5 * 81 + 7)
    small = A.Lookahead()
    many = small.q_rows(eng, pairs)
    torch.cuda.synchronize()
    assert small._sub.n_slots == 5 * 81
    assert torch.equal(one, many) and np.array_equal(one.cpu().numpy().astype(np.int64), _want(CFG, pairs.cpu().numpy()))
    per_game = np.bincount(pairs[:, 0].cpu().numpy())
    assert (np.cumsum(per_game) % 5 != 0).any() and per_game.max() >= 2


# ---- 3. whole matches against the statement -------------------------------------------------------------------------------------
def _check_match(res, want, boards, winner_owner=None):
    assert res.turns == want["turns"] >= 10
    assert res.winners.tolist() == [-1 if w is None else w for w in want["winners"]]
    assert res.lengths.tolist() == want["lengths"]
    if winner_owner is not None:
        assert winner_owner.tolist() == [-1 if w is None else w for w in want["winner_owner"]]
    for g, (a, b) in enumerate(zip(boards, want["boards"])):
        for k in R.KEYS:
            assert np.array_equal(a[k], b[k]), f"game {g} ({want['lengths'][g]} turns): {k}"


def _spawn(want):
    log = want["spawn_log"]
    return lambda turn: np.maximum(log[turn - 1], -1)


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


@pytest.mark.parametrize("name, board, n", [("duel-7x7x2", "7x7x2", K.N_DUEL), ("1v3-11x11x4", "11x11x4", K.N_FOUR)])
def test_lookahead_against_scripted_through_arena_match(monkeypatch, name, board, n):
    from snake_engine.arena import Arena, Lookahead, Scripted
    from snake_engine.engine import compact_from_state
    want = K.reference(name)
    H, W, S, hd = want["geometry"]
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(SR.start_states(board, n))
    res, reads = _reads(monkeypatch, lambda: arena.match(Lookahead(), Scripted(), 1, spawn_tape=_spawn(want)))
    _check_match(res, want, [compact_from_state(s) for s in arena.engine.export()])
    assert reads[:-1] == want["counts"] and not any(reads[-1]), "a turn's read-back"
    assert res.wins_a + res.wins_b + res.draws == n


def _league(want, n, attach=False):
    from stubnet_device import DeviceStubNNet
    from snake_engine.arena import Lookahead, Scripted
    from snake_engine.engine import compact_from_state
    from snake_engine.league import League
    H, W, S, hd = want["geometry"]
    counts = []
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(SR.start_states("11x11x4", n))
    rec, tal = (league.record([0, 5, n - 1]), league.tally()) if attach else (None, None)
    res = league.play([Lookahead(), Scripted(R.SPACE), DeviceStubNNet()], R.three_owner_table(n), counts_log=counts,
                      spawn_tape=_spawn(want))
    return res, counts, [compact_from_state(s) for s in league.engine.export()], rec, tal


def test_a_lookahead_owner_a_scripted_owner_and_a_stub_net_through_league_play():
    want = K.reference("league-11x11x4")
    res, counts, boards, _, _ = _league(want, K.N_LEAGUE)
    _check_match(res, want, boards, res.winner_owner)
    assert counts == want["counts"]
    assert all(c > 0 for c in want["counts"][0]) and len(set(want["winners"])) >= 3


def test_the_same_with_a_recorder_and_a_tally_attached():
    want = K.reference("league-11x11x4")
    n = K.N_LEAGUE
    res, counts, boards, rec, tal = _league(want, n, attach=True)
    _check_match(res, want, boards, res.winner_owner)
    assert counts == want["counts"]
    for g in (0, 5, n - 1):
        assert len(rec.frames(g)) == 2 * want["lengths"][g]
    assert tal.fate.shape == (n, 4) and tal.by_owner().seats.tolist() == np.bincount(R.three_owner_table(n).reshape(-1)).tolist()
    alive_at_end = np.array([st["alive"] for st in want["boards"]]).astype(bool)
    assert np.array_equal(tal.fate == 0, alive_at_end)


# ---- 4. launches and read-backs ---------------------------------------------------------------------------------------------------
def test_the_calls_and_read_backs_of_a_lookahead_match(monkeypatch):
    """Lookahead against Lookahead: per turn the row list, one snk_pit_look_values per side, snk_pit_moves, the tick and the
    verdict -- no observe launch, no net; one .tolist() per turn and the one that sees nothing left; and over the whole match no
    Tensor.cpu / .item / .tolist / .numpy but those and the result's"""
    import torch
    from snake_engine.arena import Arena, Lookahead
    n = 24
    arena = Arena(11, 11, 4, 1, n, seed=3)
    calls = arena.engine.L = Calls(arena.engine.L)
    sides = (Lookahead(), Lookahead(R.FOOD))
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
    turn = ["snk_pit_rows", "snk_pit_look_values", "snk_pit_look_values", "snk_pit_moves", "snk_engine_step_active_tape",
            "snk_engine_rewards", "snk_pit_verdict"]
    assert res.turns >= 10 and [c for c in calls.names if c not in HOST_ONLY] == turn * res.turns + ["snk_pit_rows"]
    assert count[0] == res.turns + 1 + 4, "the turn's read-back, the one that sees nothing left, winners and lengths"
    assert res.wins_a + res.wins_b + res.draws == n and res.lengths.max() == res.turns
    assert all(s._sub.n_slots <= n * 81 and s._sub.food_spawn_chance == 0 for s in sides)
