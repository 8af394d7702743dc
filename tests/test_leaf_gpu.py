"""GPU tests of territory at the leaf: snk_pit_look_values_leaf, snk_pit_deep_values_leaf and snk_pit_playout_values_leaf against
the CPU statement (tests/leaf_ref.py), every score equal as an integer, on recorded boards of the three plane widths -- 7x7x2 (one
word), 11x11x4 at health decrement 9 (two words; the health crosses hungry = 40 within a few ticks) and 19x19x8 (six words, games
above four alive and below) -- that have been played for some turns: dead snakes, unequal lengths, eaten food, a lone survivor.
With SNK_LEAF_SCRIPT the calls are the old entry points bit for bit; the two new refusals; the chunks of q_rows; whole matches
through Arena.match and League.play against the statement's match player; and which entry points a player calls.

A board stands in the slot of its index (the playout's draws are keyed by the slot), every ring laid out across the ring's end."""
import ctypes as C
import functools

import numpy as np
import pytest

import leaf_ref as F
import script_ref as R
import search_pit_ref as SR
from conftest import load_golden
from pit_calls import Calls
from test_deep_gpu import BAD, _engine_of
from test_playout_gpu import _Cut, _after_the_cut, _alive_pairs, _check_boards, _same, _spawn

pytestmark = pytest.mark.gpu

SENT = -7.0
HUNGRY = F.HUNGRY
P, T = 2, 3
SETTINGS = ((R.ALL, 100), (R.ALL, HUNGRY), (5, 100), (5, HUNGRY))       # (flags, hungry)


@functools.lru_cache(maxsize=None)
def _engine_with(cfg):
    return _engine_of(*F.recorded(cfg))


def _new_subs(eng, slots):
    from snake_engine import Engine
    return [Engine(max(n, 1), eng.H, eng.W, eng.S, eng.health_dec, 0, seed=0) for n in slots]


def _fan(eng):
    return eng.L.snk_pit_look_fanout(eng.S)


def _run(eng, pairs, elems, call, extra=3):
    """call(d_pairs, m, d_scratch, d_q) -> float32[m][3]; the `extra` sentinel rows past m must stay as they are"""
    import torch
    from snake_engine._lib import check
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    m = len(pairs)
    d_pairs = torch.as_tensor(pairs, device="cuda")
    assert elems(m) >= 0
    scratch = torch.empty((max(elems(m), 1),), dtype=torch.int32, device="cuda")
    q = torch.full((m + extra, 3), SENT, dtype=torch.float32, device="cuda")
    check(call(d_pairs.data_ptr(), m, scratch.data_ptr(), q.data_ptr()))
    torch.cuda.synchronize()
    out = q.cpu().numpy()
    assert (out[m:] == SENT).all(), "a row past m was written"
    return out[:m]


def _look(eng, sub, pairs, flags=R.ALL, leaf=1, hungry=100, old=False, L=None):
    L = L or eng.L
    return _run(eng, pairs, lambda m: L.snk_pit_look_scratch_elems(m, eng.S), lambda p, m, s, q:
                L.snk_pit_look_values(eng.h, sub.h, p, m, flags, s, q, 0) if old else
                L.snk_pit_look_values_leaf(eng.h, sub.h, p, m, flags, leaf, hungry, s, q, 0))


def _deep(eng, subs, depth, pairs, flags=R.ALL, leaf=1, hungry=100, old=False, L=None):
    L = L or eng.L
    handles = (C.c_void_p * len(subs))(*[s.h.value for s in subs])
    return _run(eng, pairs, lambda m: L.snk_pit_deep_scratch_elems(m, eng.S, depth), lambda p, m, s, q:
                L.snk_pit_deep_values(eng.h, handles, depth, p, m, flags, s, q, 0) if old else
                L.snk_pit_deep_values_leaf(eng.h, handles, depth, p, m, flags, leaf, hungry, s, q, 0))


def _play(eng, sub, pairs, flags=R.ALL, leaf=1, hungry=100, eps=64, seed=0, old=False, L=None):
    L = L or eng.L
    return _run(eng, pairs, lambda m: L.snk_pit_playout_scratch_elems(m, eng.S, P), lambda p, m, s, q:
                L.snk_pit_playout_values(eng.h, sub.h, p, m, flags, P, T, eps, seed, s, q, 0) if old else
                L.snk_pit_playout_values_leaf(eng.h, sub.h, p, m, flags, leaf, hungry, P, T, eps, seed, s, q, 0))


def _ints(out):
    assert np.array_equal(out, np.round(out)), "a score is no integer"
    return out.astype(np.int64)


def _rows(scores, pairs):
    """the statement's rows from [board] or {board: } -> {s: three scores}; -1, -1, -1 for a dead snake or a pair out of range"""
    get = scores.get if isinstance(scores, dict) else lambda g, d: scores[g] if 0 <= g < len(scores) else d
    return np.array([get(g, {}).get(s, [-1] * 3) for g, s in np.asarray(pairs).tolist()], np.int64).reshape(-1, 3)


def _mixed(boards):
    """every alive row, with the BAD pairs and the dead snakes' pairs among them"""
    alive = _alive_pairs(boards)
    dead = np.array([(g, s) for g, st in enumerate(boards) for s in range(len(st["alive"])) if not st["alive"][s]][:5], np.int32)
    return np.concatenate([alive[:3], np.array(BAD[:4], np.int32), dead.reshape(-1, 2), alive[3:], np.array(BAD[4:], np.int32)])


# ---- 1. the lookahead over territory ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["7x7x2", "11x11x4_dec9", "19x19x8"])
def test_look_values_leaf_on_every_row(cfg):
    H, W, S, hd, boards = F.recorded(cfg)
    eng = _engine_with(cfg)
    pairs = _mixed(boards)
    sub = _new_subs(eng, [len(pairs) * _fan(eng)])[0]          # a BAD pair inside the list starts a group of its own
    before = bytes(eng.export())
    seen = {}
    for flags, hungry in SETTINGS:
        got = _ints(_look(eng, sub, pairs, flags, 1, hungry))
        _same(got, _rows(F.look_scores(cfg, flags, hungry), pairs), pairs, f"{cfg} flags {flags} hungry {hungry}")
        seen[flags, hungry] = got.tobytes()
    assert seen[R.ALL, 100] != seen[R.ALL, HUNGRY] and seen[5, 100] != seen[5, HUNGRY], "the threshold changes no score"
    assert cfg != "7x7x2" or seen[R.ALL, HUNGRY] != seen[5, HUNGRY], "the flags change no score"   # heads rarely meet on the wide boards
    assert bytes(eng.export()) == before, "the source engine was written"
    alive = [int(st["alive"].sum()) for st in boards]
    assert alive[-1] == 1 and min(alive[:-1]) >= 2 and (cfg != "19x19x8" or (max(alive) > 4 and 2 <= min(alive[:-1]) <= 4))
    plain = _ints(_look(eng, sub, pairs, R.ALL, old=True))
    assert (plain != _ints(_look(eng, sub, pairs, R.ALL, 1, 100))).any()


# ---- 2. the deep search over territory ------------------------------------------------------------------------------------------------
def _deep_pairs(cfg):
    boards = F.recorded(cfg)[4]
    return np.array([(g, s) for g in F.deep_boards(cfg) for s in range(len(boards[g]["alive"])) if boards[g]["alive"][s]], np.int32)


@pytest.mark.parametrize("cfg,depth,settings", [("7x7x2", 2, SETTINGS), ("11x11x4_dec9", 2, SETTINGS[1:2]), ("7x7x2", 3, SETTINGS[1:2])])
def test_deep_values_leaf(cfg, depth, settings):
    """11x11x4: the first recorded board of every count of snakes alive, 6 561 leaves for the one with four"""
    eng = _engine_with(cfg)
    pairs = _deep_pairs(cfg)
    subs = _new_subs(eng, [len(pairs) * _fan(eng) ** k for k in range(1, depth + 1)])
    for flags, hungry in settings:
        got = _ints(_deep(eng, subs, depth, pairs, flags, 1, hungry))
        _same(got, _rows(F.deep_scores(cfg, depth, flags, hungry), pairs), pairs, f"{cfg} depth {depth} flags {flags} hungry {hungry}")
    assert got.max() > 0 and (cfg != "7x7x2" or got.min() < -32 * (depth - 1)), "no move punished at the root's tick, or none that is not"


@pytest.mark.parametrize("cfg", ["7x7x2", "11x11x4_dec9", "19x19x8"])
def test_deep_leaf_at_depth_one_is_the_lookahead_call(cfg):
    H, W, S, hd, boards = F.recorded(cfg)
    eng = _engine_with(cfg)
    pairs = _mixed(boards)
    subs = _new_subs(eng, [len(pairs) * _fan(eng)])
    for leaf, hungry in ((1, HUNGRY), (1, 100), (0, 100)):
        assert _deep(eng, subs, 1, pairs, R.ALL, leaf, hungry).tobytes() == _look(eng, subs[0], pairs, R.ALL, leaf, hungry).tobytes()


# ---- 3. the playout over territory ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["7x7x2", "11x11x4_dec9"])
def test_playout_values_leaf_whole_cut_in_two_and_permuted(cfg):
    H, W, S, hd, boards = F.recorded(cfg)
    eng = _engine_with(cfg)
    pairs = _mixed(boards)
    m = len(pairs)
    sub = _new_subs(eng, [m * 3 * P])[0]
    for eps, hungry in ((0, HUNGRY), (64, HUNGRY), (64, 100)):
        whole = _play(eng, sub, pairs, R.ALL, 1, hungry, eps, 5)
        _same(_ints(whole), _rows(F.playout_scores(cfg, P, T, eps, 5, R.ALL, hungry), pairs), pairs, f"{cfg} eps {eps} hungry {hungry}")
        cut = m // 2 + 1
        two = np.concatenate([_play(eng, sub, pairs[:cut], R.ALL, 1, hungry, eps, 5), _play(eng, sub, pairs[cut:], R.ALL, 1, hungry, eps, 5)])
        assert two.tobytes() == whole.tobytes(), "cut into two calls"
        order = np.random.RandomState(3).permutation(m)
        assert _play(eng, sub, pairs[order], R.ALL, 1, hungry, eps, 5).tobytes() == whole[order].tobytes(), "permuted"
    assert (_ints(whole) > 3).any() and (whole != _play(eng, sub, pairs, R.ALL, seed=5, old=True)).any()


# ---- 4. SNK_LEAF_SCRIPT is the old entry point ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["7x7x2", "11x11x4_dec9", "19x19x8"])
def test_with_the_script_leaf_each_call_writes_what_the_old_call_writes(cfg):
    H, W, S, hd, boards = F.recorded(cfg)
    eng = _engine_with(cfg)
    pairs = _mixed(boards)
    F1 = _fan(eng)
    sub = _new_subs(eng, [len(pairs) * max(F1, 3 * P)])[0]
    for flags in (R.ALL, 5):
        old = _look(eng, sub, pairs, flags, old=True)
        assert _look(eng, sub, pairs, flags, 0, 100).tobytes() == old.tobytes() and (old != -1).any()
        old = _play(eng, sub, pairs, flags, seed=9, old=True)
        assert _play(eng, sub, pairs, flags, 0, 100, seed=9).tobytes() == old.tobytes() and (old != -1).any()
    few = pairs if cfg == "7x7x2" else _alive_pairs(boards)[-3:]              # the last two boards, the lone survivor's among them
    subs = _new_subs(eng, [len(few) * F1, len(few) * F1 * F1])
    old = _deep(eng, subs, 2, few, old=True)
    assert _deep(eng, subs, 2, few, R.ALL, 0, 100).tobytes() == old.tobytes() and (old != -1).any()


# ---- 5. the two new refusals ------------------------------------------------------------------------------------------------------------
def test_a_refused_leaf_or_hungry_launches_nothing():
    import torch
    from snake_engine import EngineError
    from snake_engine._lib import check
    cfg = "7x7x2"
    H, W, S, hd, boards = F.recorded(cfg)
    eng = _engine_with(cfg)
    pairs = torch.as_tensor(_alive_pairs(boards), device="cuda")
    m = int(pairs.shape[0])
    sub, sub2 = _new_subs(eng, [m * 9, m * 81])
    held = bytes(sub.export())
    handles = (C.c_void_p * 2)(sub.h.value, sub2.h.value)
    scratch = torch.empty((max(eng.L.snk_pit_deep_scratch_elems(m, S, 2), eng.L.snk_pit_playout_scratch_elems(m, S, P)),),
                          dtype=torch.int32, device="cuda")
    q = torch.full((m, 3), SENT, dtype=torch.float32, device="cuda")
    calls = Calls(eng.L)
    d = (pairs.data_ptr(), scratch.data_ptr(), q.data_ptr())
    forms = {"snk_pit_look_values_leaf": lambda leaf, h: calls.snk_pit_look_values_leaf(eng.h, sub.h, d[0], m, 7, leaf, h, d[1], d[2], 0),
             "snk_pit_deep_values_leaf": lambda leaf, h: calls.snk_pit_deep_values_leaf(eng.h, handles, 2, d[0], m, 7, leaf, h, d[1], d[2], 0),
             "snk_pit_deep_values_leaf ": lambda leaf, h: calls.snk_pit_deep_values_leaf(eng.h, handles, 1, d[0], m, 7, leaf, h, d[1], d[2], 0),
             "snk_pit_playout_values_leaf": lambda leaf, h: calls.snk_pit_playout_values_leaf(eng.h, sub.h, d[0], m, 7, leaf, h, P, T, 64, 0,
                                                                                               d[1], d[2], 0)}
    bad = [(2, 100), (-1, 100), (1 << 30, 40), (1, 101), (1, -1), (1, 1 << 20), (0, 40), (0, 99), (0, 101)]
    for name, call in forms.items():
        for leaf, hungry in bad:
            with pytest.raises(EngineError, match="leaf="):
                check(call(leaf, hungry))
    torch.cuda.synchronize()
    assert calls.names == [name.strip() for name in forms for _ in bad], "a refused call went on to another entry point"
    assert (q.cpu().numpy() == SENT).all(), "a refused call wrote"
    assert bytes(sub.export()) == held, "a refused call launched on the sub-engine"
    for name, call in forms.items():                                          # and the calls still work, at the ends of hungry too
        for leaf, hungry in ((1, 0), (1, 100), (0, 100)):
            check(call(leaf, hungry))
    torch.cuda.synchronize()
    assert (q.cpu().numpy() != SENT).all()


# ---- 6. the chunks of q_rows --------------------------------------------------------------------------------------------------------------
def test_q_rows_with_small_budgets_gives_the_rows_of_one_call(monkeypatch):
    import torch
    from snake_engine import arena as A
    cfg = "7x7x2"
    H, W, S, hd, boards = F.recorded(cfg)
    eng = _engine_with(cfg)
    np_pairs = _alive_pairs(boards)
    pairs = torch.as_tensor(np_pairs, device="cuda")
    m = int(pairs.shape[0])
    assert m > 8 and m % 4 != 0
    make = {"look": lambda: A.Lookahead(leaf=A.Territory(hungry=HUNGRY)), "deep": lambda: A.Deep(depth=2, leaf=A.Territory(hungry=HUNGRY)),
            "play": lambda: A.Playout(playouts=P, horizon=T, seed=5, leaf=A.Territory(hungry=HUNGRY))}
    want = {"look": _rows(F.look_scores(cfg, R.ALL, HUNGRY), np_pairs), "play": _rows(F.playout_scores(cfg, P, T, 64, 5, R.ALL, HUNGRY), np_pairs)}
    one = {k: f().q_rows(eng, pairs) for k, f in make.items()}
    for k, rows in want.items():
        assert np.array_equal(one[k].cpu().numpy().astype(np.int64), rows), k
    sub = _new_subs(eng, [m * 9, m * 81])
    assert one["deep"].cpu().numpy().tobytes() == _deep(eng, sub, 2, np_pairs, R.ALL, 1, HUNGRY).tobytes()
    monkeypatch.setattr(A, "LOOK_SLOT_BUDGET", 4 * 9 + 2)                       # four rows a call
    monkeypatch.setattr(A, "DEEP_BYTE_BUDGET", 4 * eng.slot_bytes * (9 + 81) + 5)
    monkeypatch.setattr(A, "PLAYOUT_SLOT_BUDGET", 4 * 3 * P + 2)
    small = {k: f() for k, f in make.items()}
    calls = eng.L = Calls(eng.L)
    try:
        many = {k: side.q_rows(eng, pairs) for k, side in small.items()}
    finally:
        eng.L = calls._L
    torch.cuda.synchronize()
    chunks = (m + 3) // 4
    for k, name in (("look", "snk_pit_look_values_leaf"), ("deep", "snk_pit_deep_values_leaf"), ("play", "snk_pit_playout_values_leaf")):
        assert torch.equal(one[k], many[k]), k
        assert calls.names.count(name) == chunks and tuple(many[k].shape) == (m, 3)
    assert not any(n in calls.names for n in ("snk_pit_look_values", "snk_pit_deep_values", "snk_pit_playout_values"))
    assert small["look"]._sub.n_slots == 4 * 9 and small["play"]._sub.n_slots == 4 * 3 * P
    assert [s.n_slots for s in small["deep"]._subs] == [4 * 9, 4 * 81]


# ---- 7. whole matches against the statement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["look-7x7x2", "deep-7x7x2", "playout-7x7x2"])
def test_a_territory_leaf_player_against_territory_through_arena_match(name):
    """from the recorded start draws of the sixteen 7x7x2 trajectories (an init_tape), the food from the statement's spawn log"""
    from snake_engine.arena import Arena, Deep, Lookahead, Playout, Territory
    from snake_engine.engine import compact_from_state
    want = F.reference(name)
    H, W, S, hd = want["geometry"]
    n = F.N_DUEL
    z = load_golden("tic_7x7x2.npz")
    tape = np.stack([z["init_positions"], z["init_dirs"], z["init_food"]], axis=1)[:n]
    leaf = Territory(hungry=HUNGRY)
    side = {"look-7x7x2": Lookahead(leaf=leaf), "deep-7x7x2": Deep(depth=2, leaf=leaf),
            "playout-7x7x2": Playout(playouts=F.MATCH_P, horizon=F.MATCH_T, leaf=leaf)}[name]
    arena = Arena(H, W, S, hd, n, seed=1)
    res = arena.match(side, Territory(hungry=HUNGRY), 1, init_tape=tape, spawn_tape=_spawn(want))
    assert res.turns == want["turns"] >= 10
    assert res.winners.tolist() == [-1 if w is None else w for w in want["winners"]]
    assert res.lengths.tolist() == want["lengths"]
    _check_boards([compact_from_state(s) for s in arena.engine.export()], want)
    assert res.wins_a + res.wins_b + res.draws == n


def test_three_territory_leaf_owners_and_a_scripted_one_through_league_play():
    """a seat each, rotated from game to game; cut at a turn cap the statement shares (6 561 territory leaves a board in Python)"""
    from snake_engine.arena import Deep, Lookahead, Playout, Scripted, Territory
    from snake_engine.league import League
    want = F.reference("league-11x11x4")
    H, W, S, hd = want["geometry"]
    n, cap = F.N_LEAGUE, F.CAP_LEAGUE
    leaf = Territory(hungry=HUNGRY)
    counts = []
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(SR.start_states("11x11x4", n))
    with pytest.raises(_Cut):
        league.play([Deep(depth=2, leaf=leaf), Lookahead(leaf=leaf), Playout(playouts=F.MATCH_P, horizon=F.MATCH_T, seed=9, leaf=leaf),
                     Scripted()], F.four_owner_table(n), counts_log=counts, spawn_tape=_spawn(want, cap))
    assert counts[:cap] == want["counts"] and len(counts) == cap + 1 and all(c > 0 for c in want["counts"][0])
    _after_the_cut(league, want)


# ---- 8. which entry points a player calls -----------------------------------------------------------------------------------------------
def test_without_a_leaf_the_old_names_with_one_the_leaf_names():
    from snake_engine.arena import Arena, Deep, Lookahead, Playout, Territory
    old = ("snk_pit_look_values", "snk_pit_deep_values", "snk_pit_playout_values")
    for leaf in (None, Territory(hungry=HUNGRY)):
        sides = [Lookahead(leaf=leaf), Deep(depth=2, leaf=leaf), Playout(playouts=2, horizon=3, leaf=leaf)]
        for side, name in zip(sides, old):
            arena = Arena(7, 7, 2, 1, 12, seed=3)
            calls = arena.engine.L = Calls(arena.engine.L)
            res = arena.match(side, Territory(), 1)
            mine = [c for c in calls.names if c.startswith(name)]
            assert res.turns >= 3 and mine == [name + ("_leaf" if leaf is not None else "")] * res.turns, (name, leaf)
            assert calls.names.count("snk_pit_territory_values") == res.turns          # the rival's launch, through its own entry point
            assert not any(c in old or c.endswith("_leaf") for c in calls.names if c not in mine)
