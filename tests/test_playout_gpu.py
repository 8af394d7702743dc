"""GPU tests of the playout opponent: snk_pit_playout_values against the CPU statement (tests/playout_ref.py), scores equal as
integers, on boards taken from the golden trajectories and on hand-built ones, imported at a ring start that wraps; every flag
subset; the exploration settings and seeds; the limits of P and T; edge rows, the independence of the row order and of the cut
into calls, the refusals -- then whole matches through Arena.match and League.play against the statement's match player, and the
launch and read-back counts.

A board stands in the slot of its index, since the draws are keyed by the slot.  Matches on 11x11x4 are cut at a turn cap the
statement shares: the spawn tape of the turn after the cap raises (the turn loop has no cap of its own)."""
import functools
import sys

import numpy as np
import pytest

import league_ref as LR
import playout_ref as M
import script_ref as R
import search_pit_ref as SR
from pit_calls import Calls
from test_deep_gpu import BAD

pytestmark = pytest.mark.gpu

HOST_ONLY = ("snk_pit_look_fanout", "snk_pit_look_scratch_elems", "snk_pit_playout_clones", "snk_pit_playout_scratch_elems")
P, T = 2, 3                                         # most cases: the statement costs P * 3 * T * A script evaluations a row


def _engine_of(H, W, S, hd, boards):
    """boards in an engine, every ring laid out so that it runs across the ring's end"""
    from snake_engine import Engine
    from snake_engine.engine import state_from_compact
    cap = 1 << (H * W + 1).bit_length()
    assert cap // 2 < H * W + 2 <= cap
    eng = Engine(len(boards), H, W, S, hd, 0.15, seed=1)
    eng.import_states([state_from_compact(H, W, S, st) for st in boards], ring_start=cap - 2)
    return eng


def _geometry(cfg):
    return M.HAND if cfg == "hand" else M.sampled(cfg)


@functools.lru_cache(maxsize=None)
def _engine_with(cfg):
    return _engine_of(*_geometry(cfg))


def _sub(eng, slots):
    from snake_engine import Engine
    return Engine(max(slots, 1), eng.H, eng.W, eng.S, eng.health_dec, 0, seed=0)


def _raw(eng, sub, pairs, P=P, T=T, eps=64, seed=0, flags=R.ALL, extra=3, L=None):
    """snk_pit_playout_values over int pairs [m][2] -> float32[m][3]; the `extra` NaN rows past m must stay NaN"""
    import torch
    from snake_engine._lib import check
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    m = len(pairs)
    d_pairs = torch.as_tensor(pairs, device="cuda") if m else None
    elems = eng.L.snk_pit_playout_scratch_elems(m, eng.S, P)
    assert elems >= 0
    scratch = torch.empty((max(elems, 1),), dtype=torch.int32, device="cuda")
    q = torch.full((m + extra, 3), float("nan"), dtype=torch.float32, device="cuda")
    check((L or eng.L).snk_pit_playout_values(eng.h, sub.h, d_pairs.data_ptr() if m else 0, m, flags, P, T, eps, seed,
                                              scratch.data_ptr() if m else 0, q.data_ptr() if m else 0, 0))
    torch.cuda.synchronize()
    out = q.cpu().numpy()
    assert np.isnan(out[m:]).all(), "a row past m was written"
    return out[:m]


def _values(eng, sub, pairs, **kw):
    out = _raw(eng, sub, pairs, **kw)
    assert np.array_equal(out, np.round(out)), "a score is no integer"
    return out.astype(np.int64)


def _alive_pairs(boards):
    return np.array([(g, s) for g, st in enumerate(boards) for s in range(len(st["alive"])) if st["alive"][s]], np.int32)


@functools.lru_cache(maxsize=None)
def _scores(cfg, P=P, T=T, eps=64, seed=0, flags=R.ALL):
    """[board g] -> {s: three scores}: the statement, computed once per setting and shared"""
    if cfg != "hand":
        return M.sampled_scores(cfg, P, T, eps, seed, flags)
    H, W, S, hd, boards = M.HAND
    return [M.board_playout_scores(H, W, S, hd, st, g, P, T, eps, seed, flags) for g, st in enumerate(boards)]


def _want(cfg, pairs, **kw):
    """the statement's rows; -1, -1, -1 for a dead snake and for a slot or id out of range"""
    scores = _scores(cfg, **kw)
    return np.array([scores[g].get(s, [-1] * 3) if 0 <= g < len(scores) else [-1] * 3 for g, s in np.asarray(pairs).tolist()],
                    np.int64).reshape(-1, 3)


def _same(got, want, pairs, what):
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(pairs)} rows differ, first {pairs[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"


# ---- 1. against the statement, cell for cell ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["5x5x2", "7x7x2", "9x9x3", "11x11x4", "16x16x6", "19x19x8", "hand"])
def test_scores_equal_the_statement_on_golden_and_hand_built_boards(cfg):
    """16x16x6 with five and six alive and 19x19x8 with six or more and eight: the boards where Lookahead and Deep fall back, and
    the flood planes of several words.  hand: a lone snake, one that starves at tick 1, two that meet head-on at tick 0"""
    H, W, S, hd, boards = _geometry(cfg)
    eng = _engine_with(cfg)
    pairs = _alive_pairs(boards)
    got = _values(eng, _sub(eng, len(pairs) * 3 * P), pairs)
    _same(got, _want(cfg, pairs), pairs, cfg)
    alive = [int(np.count_nonzero(st["alive"])) for st in boards]
    played = got[np.array([alive[g] >= 2 for g in pairs[:, 0]])]                # a lone snake's rows are plain scores
    assert played.min() >= -1 and played.max() <= M.high(P, T) and (played > 3).any()
    if cfg == "16x16x6":
        assert alive == [5, 6]
    elif cfg == "19x19x8":
        assert alive[0] >= 6 and alive[1] == 8
        plain = np.array([R.scores(H, W, boards[g], s) for g, s in pairs.tolist()], np.int64)
        assert (got != plain).any(), "above four snakes alive it is not the plain script"
    elif cfg == "hand":
        assert alive == [1, 2, 3]
        lone = pairs[:, 0] == M.LONE
        assert np.array_equal(got[lone], np.array([R.scores(H, W, boards[M.LONE], 0)], np.int64))
        assert (got[pairs[:, 0] == M.STARVE][0] // 4 == 2).all() and got[pairs[:, 0] == M.HEADON][0][1] // 4 == 0


def test_every_flag_subset():
    H, W, S, hd, boards = M.sampled("7x7x2")
    eng = _engine_with("7x7x2")
    pairs = _alive_pairs(boards)
    sub = _sub(eng, len(pairs) * 3 * P)
    seen = set()
    for flags in range(8):
        _same(_values(eng, sub, pairs, flags=flags), _want("7x7x2", pairs, flags=flags), pairs, f"flags {flags}")
        seen.add(_want("7x7x2", pairs, flags=flags).tobytes())
    assert len(seen) >= 2


@pytest.mark.parametrize("eps", [0, 64, 256])
def test_exploration_settings_with_two_seeds(eps):
    H, W, S, hd, boards = M.sampled("9x9x3")
    eng = _engine_with("9x9x3")
    pairs = _alive_pairs(boards)
    sub = _sub(eng, len(pairs) * 3 * P)
    seeds = (3, (1 << 63) + 5)
    got = [_values(eng, sub, pairs, eps=eps, seed=seed) for seed in seeds]
    for g, seed in zip(got, seeds):
        _same(g, _want("9x9x3", pairs, eps=eps, seed=seed), pairs, f"eps {eps} seed {seed}")
    assert np.array_equal(got[0], got[1]) == (eps == 0)


@pytest.mark.parametrize("P_, T_", [(64, 2), (2, 64)])
def test_the_limits_of_playouts_and_horizon(P_, T_):
    H, W, S, hd, boards = M.sampled("7x7x2")
    two = [g for g, st in enumerate(boards) if st["alive"].sum() == 2][:2]
    eng = _engine_with("7x7x2")
    pairs = np.array([(g, s) for g in two for s in range(2)], np.int32)
    want = np.array([M.playout_scores(H, W, S, hd, boards[g], g, s, P_, T_, 64, 1) for g, s in pairs.tolist()], np.int64)
    got = _values(eng, _sub(eng, len(pairs) * 3 * P_), pairs, P=P_, T=T_, seed=1)
    _same(got, want, pairs, f"P {P_} T {T_}")
    assert got.max() <= M.high(P_, T_) and got.max() > 4 * P_


# ---- 2. edge rows, row orders, cuts ----------------------------------------------------------------------------------------------------
CFG = "5x5x2"                                       # eleven boards, the last with a lone snake and a dead one


def test_bad_pairs_in_the_list_and_an_exactly_sized_sub_engine():
    """the BAD pairs of test_deep_gpu.py mixed into the list; the sub-engine has exactly m * 3 * P slots; e's records are the same
    bytes afterwards; two calls are bit-identical"""
    H, W, S, hd, boards = M.sampled(CFG)
    eng = _engine_with(CFG)
    alive = _alive_pairs(boards)
    dead = np.array([(g, s) for g, st in enumerate(boards) for s in range(S) if not st["alive"][s]], np.int32)
    assert len(dead) >= 1
    pairs = np.concatenate([alive[:3], np.array(BAD[:4], np.int32), dead, alive[3:], np.array(BAD[4:], np.int32)])
    sub = _sub(eng, len(pairs) * 3 * P)
    assert sub.n_slots == len(pairs) * 3 * P
    before = bytes(eng.export())
    one = _raw(eng, sub, pairs)
    two = _raw(eng, sub, pairs)
    assert bytes(eng.export()) == before, "the source engine was written"
    assert one.tobytes() == two.tobytes()
    _same(one.astype(np.int64), _want(CFG, pairs), pairs, "mixed")
    is_bad = np.array([not (0 <= g < len(boards) and 0 <= s < S and boards[g]["alive"][s]) for g, s in pairs.tolist()])
    assert is_bad.sum() == len(BAD) + len(dead) and (one[is_bad] == -1).all() and (one[~is_bad] != -1).any()
    assert (_values(eng, sub, np.array(BAD, np.int32)) == -1).all()


def test_m_zero_takes_null_buffers():
    eng = _engine_with(CFG)
    assert _raw(eng, _sub(eng, 1), np.zeros((0, 2), np.int32)).shape == (0, 3)


def test_the_order_of_the_rows_and_the_cut_into_calls_change_nothing():
    H, W, S, hd, boards = M.sampled(CFG)
    eng = _engine_with(CFG)
    pairs = _alive_pairs(boards)[:7]
    sub = _sub(eng, (len(pairs) + 1) * 3 * P)
    whole = _raw(eng, sub, pairs, eps=256, seed=11)
    _same(whole.astype(np.int64), _want(CFG, pairs, eps=256, seed=11), pairs, "whole")
    assert _raw(eng, sub, pairs[::-1], eps=256, seed=11).tobytes() == whole[::-1].tobytes(), "reversed"
    twice = np.concatenate([pairs[:3], pairs[1:2], pairs[3:]])
    assert _raw(eng, sub, twice, eps=256, seed=11).tobytes() == np.concatenate([whole[:3], whole[1:2], whole[3:]]).tobytes(), "a row repeated"
    for cut in range(len(pairs) + 1):
        parts = [_raw(eng, sub, pairs[:cut], eps=256, seed=11), _raw(eng, sub, pairs[cut:], eps=256, seed=11)]
        assert np.concatenate(parts).tobytes() == whole.tobytes(), f"cut at {cut}"


def test_q_rows_with_a_small_budget_gives_the_rows_of_one_call(monkeypatch):
    import torch
    from snake_engine import arena as A
    H, W, S, hd, boards = M.sampled(CFG)
    eng = _engine_with(CFG)
    pairs = torch.as_tensor(_alive_pairs(boards), device="cuda")
    m = int(pairs.shape[0])
    whole = A.Playout(playouts=P, horizon=T, explore=256, seed=11)
    one = whole.q_rows(eng, pairs)
    assert whole._sub.n_slots == m * 3 * P and whole._sub.food_spawn_chance == 0
    monkeypatch.setattr(A, "PLAYOUT_SLOT_BUDGET", 4 * (3 * P) + 2)
    small = A.Playout(playouts=P, horizon=T, explore=256, seed=11)
    many = small.q_rows(eng, pairs)
    monkeypatch.setattr(A, "PLAYOUT_SLOT_BUDGET", 1)
    rows = A.Playout(playouts=P, horizon=T, explore=256, seed=11)
    each = rows.q_rows(eng, pairs)
    torch.cuda.synchronize()
    assert small._sub.n_slots == 4 * 3 * P and rows._sub.n_slots == 3 * P and m % 4 != 0 and m > 8
    assert torch.equal(one, many) and torch.equal(one, each)
    assert np.array_equal(one.cpu().numpy().astype(np.int64), _want(CFG, pairs.cpu().numpy(), eps=256, seed=11))


def test_refusals():
    """every refusal is an error before any launch: no other entry point is called, the scores stay NaN and the sub-engine's
    records are the bytes they were"""
    import torch
    from snake_engine import Engine, EngineError
    from snake_engine._lib import check
    H, W, S, hd, boards = M.sampled(CFG)
    eng = _engine_with(CFG)
    pairs = torch.as_tensor(_alive_pairs(boards), device="cuda")
    m = int(pairs.shape[0])
    n = m * 3 * P
    scratch = torch.empty((eng.L.snk_pit_playout_scratch_elems(m, S, 64),), dtype=torch.int32, device="cuda")
    q = torch.full((m, 3), float("nan"), dtype=torch.float32, device="cuda")
    ok = _sub(eng, n)
    held = bytes(ok.export())
    calls = Calls(eng.L)
    mk = lambda slots, h=H, s=S, dec=hd, food=0: Engine(slots, h, h, s, dec, food, seed=0)

    def call(sub=ok, d_pairs=pairs.data_ptr(), rows=m, flags=R.ALL, P_=P, T_=T, eps=64, d_scratch=scratch.data_ptr(), d_q=q.data_ptr()):
        check(calls.snk_pit_playout_values(eng.h, None if sub is None else sub.h, d_pairs, rows, flags, P_, T_, eps, 5, d_scratch, d_q, 0))

    bad = [dict(sub=mk(n - 1)), dict(sub=mk(n, h=9)), dict(sub=mk(n, s=3)), dict(sub=mk(n, food=0.15)), dict(sub=mk(n, dec=hd + 1)),
           dict(sub=eng), dict(sub=None), dict(d_pairs=0), dict(d_scratch=0), dict(d_q=0), dict(rows=-1), dict(flags=8),
           dict(flags=1 << 31), dict(P_=0), dict(P_=65), dict(P_=-1), dict(T_=0), dict(T_=65), dict(eps=-1), dict(eps=257),
           dict(sub=mk(1), rows=0, P_=0), dict(sub=mk(1, h=9), rows=0)]
    for kw in bad:
        with pytest.raises(EngineError):
            call(**kw)
    with pytest.raises(EngineError, match="slots"):
        call(sub=mk(n - 1))
    with pytest.raises(EngineError):                      # the size limit: m * 3 * P * S above 2^28, asked before any buffer is touched
        call(sub=mk(1), rows=(1 << 28) // (3 * 64 * S) + 1, P_=64)
    torch.cuda.synchronize()
    assert calls.names == ["snk_pit_playout_values"] * (len(bad) + 2), "a refused call went on to another entry point"
    assert np.isnan(q.cpu().numpy()).all(), "a refused call wrote"
    assert bytes(ok.export()) == held, "a refused call launched on the sub-engine"
    call(rows=0, d_pairs=0, d_scratch=0, d_q=0)                               # m = 0 is a no-op, its buffers may be NULL
    assert np.isnan(q.cpu().numpy()).all()
    call()                                                                    # and the call still works after the refusals
    torch.cuda.synchronize()
    assert np.array_equal(q.cpu().numpy().astype(np.int64), _want(CFG, pairs.cpu().numpy(), seed=5))


# ---- 3. whole matches against the statement -------------------------------------------------------------------------------------
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


def test_playout_against_scripted_through_arena_match(monkeypatch):
    from snake_engine.arena import Arena, Playout, Scripted
    from snake_engine.engine import compact_from_state
    want = M.reference("duel-7x7x2")
    H, W, S, hd = want["geometry"]
    n = M.N_DUEL
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(SR.start_states("7x7x2", n))
    res, reads = _reads(monkeypatch, lambda: arena.match(Playout(playouts=M.MATCH_P, horizon=M.MATCH_T), Scripted(), 1,
                                                         spawn_tape=_spawn(want)))
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


def test_one_playout_against_three_scripted_through_arena_match():
    from snake_engine.arena import Arena, Playout, Scripted
    want = M.reference("1v3-11x11x4")
    H, W, S, hd = want["geometry"]
    n, cap = M.N_FOUR, M.CAP_FOUR
    assert want["turns"] == cap
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(SR.start_states("11x11x4", n))
    with pytest.raises(_Cut):
        arena.match(Playout(playouts=M.MATCH_P, horizon=M.MATCH_T), Scripted(), 1, spawn_tape=_spawn(want, cap))
    _after_the_cut(arena, want)


def test_playout_lookahead_and_scripted_owners_through_league_play():
    from snake_engine.arena import Lookahead, Playout, Scripted
    from snake_engine.league import League
    want = M.reference("league-11x11x4")
    H, W, S, hd = want["geometry"]
    n, cap = M.N_LEAGUE, M.CAP_LEAGUE
    counts = []
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(SR.start_states("11x11x4", n))
    with pytest.raises(_Cut):
        league.play([Playout(playouts=M.MATCH_P, horizon=M.MATCH_T, seed=9), Lookahead(), Scripted(R.SPACE)], R.three_owner_table(n),
                    counts_log=counts, spawn_tape=_spawn(want, cap))
    assert counts[:cap] == want["counts"] and len(counts) == cap + 1 and all(c > 0 for c in want["counts"][0])
    _after_the_cut(league, want)


# ---- 4. launches and read-backs ---------------------------------------------------------------------------------------------------
def test_the_calls_and_read_backs_of_a_playout_match(monkeypatch):
    """Playout against Playout: per turn the row list, one snk_pit_playout_values per side, snk_pit_moves, the tick and the
    verdict -- no observe launch, no net; one .tolist() per turn and the one that sees nothing left; and over the whole match no
    Tensor.cpu / .item / .tolist / .numpy but those and the result's"""
    import torch
    from snake_engine.arena import Arena, Playout
    n = 24
    arena = Arena(7, 7, 2, 1, n, seed=3)
    calls = arena.engine.L = Calls(arena.engine.L)
    sides = (Playout(playouts=2, horizon=3), Playout(R.FOOD, 3, 2, 256, 7))
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
    turn = ["snk_pit_rows", "snk_pit_playout_values", "snk_pit_playout_values", "snk_pit_moves", "snk_engine_step_active_tape",
            "snk_engine_rewards", "snk_pit_verdict"]
    assert res.turns >= 5 and [c for c in calls.names if c not in HOST_ONLY] == turn * res.turns + ["snk_pit_rows"]
    assert count[0] == res.turns + 1 + 4, "the turn's read-back, the one that sees nothing left, winners and lengths"
    assert res.wins_a + res.wins_b + res.draws == n and res.lengths.max() == res.turns
    assert sides[0]._sub.n_slots == n * 3 * 2 and sides[1]._sub.n_slots == n * 3 * 3
