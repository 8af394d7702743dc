"""GPU tests of the scripted opponent: snk_pit_script_values against the CPU statement (tests/script_ref.py: plain Python, a queue
for the flood fill), scores equal as integers -- on every board of the golden trajectories, on hand-built boards aimed at the
kernel's bit-plane arithmetic (many fill rounds, row ends, word boundaries, the bits past the last cell, a wrapped ring), on edge
rows and sizes -- then whole matches through Arena.match, League.play and League.play_search against the statement's match
player, the read-back and launch counts, a real net, and the refusals."""
import functools

import numpy as np
import pytest

import league_ref as LR
import script_ref as R
import search_pit_ref as SR
from conftest import golden_state, load_golden

pytestmark = pytest.mark.gpu

SENT = -7.0
GOLDEN = ["5x5x2", "7x7x2", "9x9x3", "11x11x4", "11x11x4_dec9", "15x15x5", "16x16x6", "19x19x8"]


def _values(eng, pairs, flags=R.ALL, extra=3):
    """snk_pit_script_values over int pairs [m][2] -> int64[m][3]; the `extra` sentinel rows past m must stay as they are"""
    import torch
    from snake_engine._lib import check
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    m = len(pairs)
    d_pairs = torch.as_tensor(pairs, device="cuda") if m else None
    q = torch.full((m + extra, 3), SENT, dtype=torch.float32, device="cuda")
    check(eng.L.snk_pit_script_values(eng.h, d_pairs.data_ptr() if m else 0, m, flags, q.data_ptr(), 0))
    torch.cuda.synchronize()
    out = q.cpu().numpy()
    assert (out[m:] == SENT).all(), "a row past m was written"
    assert np.array_equal(out[:m], np.round(out[:m])), "a score is no integer"
    return out[:m].astype(np.int64)


def _engine_with(H, W, S, boards, ring_start=0):
    from snake_engine import Engine
    from snake_engine.engine import state_from_compact
    eng = Engine(len(boards), H, W, S, 1, 0.15, seed=1)
    eng.import_states([state_from_compact(H, W, S, st) for st in boards], ring_start=ring_start)
    return eng


def _alive_pairs(boards):
    return np.array([(g, s) for g, st in enumerate(boards) for s in range(len(st["alive"])) if st["alive"][s]], np.int32)


def _want(H, W, boards, pairs, flags):
    per_board = {}
    out = []
    for g, s in pairs:
        if g not in per_board:
            per_board[g] = R.board_scores(H, W, boards[g], flags)
        out.append(per_board[g][s])
    return np.array(out, np.int64).reshape(-1, 3)


# ---- 1. every board of the golden trajectories ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden(cfg):
    z = load_golden(f"tic_{cfg}.npz")
    H, W, S = int(z["H"]), int(z["W"]), int(z["S"])
    boards = [golden_state(z, i) for i in range(z["st_alive"].shape[0])]
    return H, W, S, boards, _engine_with(H, W, S, boards)


@pytest.mark.parametrize("cfg", GOLDEN)
def test_every_alive_row_of_the_golden_trajectories(cfg):
    """start boards and every post-tick board: one word (5x5, 7x7), two (9x9, 11x11), four and six with 16-bit ring entries"""
    H, W, S, boards, eng = _golden(cfg)
    pairs = _alive_pairs(boards)
    assert len(pairs) > 100
    for flags in (range(8) if H <= 9 else (R.ALL,)):
        got, want = _values(eng, pairs, flags), _want(H, W, boards, pairs, flags)
        bad = np.flatnonzero((got != want).any(1))
        assert len(bad) == 0, f"{cfg} flags {flags}: {len(bad)} of {len(pairs)} rows differ, first {pairs[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"
    if cfg == "11x11x4":
        assert (got == -1).any() and (got[:, 0] != got[:, 2]).any()


# ---- 2. hand-built boards aimed at the bit planes -------------------------------------------------------------------------------
def _serpentine(hw):
    """walls on the odd rows, each open at one end in turn: ONE corridor through the whole board, one cell wide, so the fill takes
    a round per cell of it (about NC / 2).  The walls are one snake's nodes (the record does not ask for adjacent nodes).  The
    mover (length 2) stands at the corridor's mouth: straight runs its whole length, left leaves the board, right is wall"""
    wall = [(r, x) for r in range(1, hw, 2) for x in (range(0, hw - 1) if (r // 2) % 2 == 0 else range(1, hw))]
    return R.board(hw, hw, [([(0, 1), (0, 0)], 1), (wall, 0)])


def _edge_pockets(hw):
    """a pocket of ONE cell on an edge or in a corner, the mover's head in front of it: a shift that ran over a row's end (or past
    the first or last cell) would leak into the free cell at the far end of the adjacent row"""
    mid, last = hw // 2, hw - 1
    out = []
    for y in (0, mid, last):            # pockets (y, last) on the right edge and (y, 0) on the left one, corners included
        walls_r = [(yy, last) for yy in (y - 1, y + 1) if 0 <= yy < hw]
        out.append(R.board(hw, hw, [([(y, last - 1), (y, last - 2)], 1), (walls_r, 0)]))
        walls_l = [(yy, 0) for yy in (y - 1, y + 1) if 0 <= yy < hw]
        out.append(R.board(hw, hw, [([(y, 1), (y, 2)], 3), (walls_l, 0)]))
    for x in (mid,):                    # pockets (0, x) on the top edge and (last, x) on the bottom one
        out.append(R.board(hw, hw, [([(1, x), (2, x)], 0), ([(0, x - 1), (0, x + 1)], 0)]))
        out.append(R.board(hw, hw, [([(last - 1, x), (last - 2, x)], 2), ([(last, x - 1), (last, x + 1)], 0)]))
    return out


def _word_pockets(hw):
    """for every word boundary 64 k inside the board a pocket of exactly the TWO cells 64 k - 1 and 64 k (neighbours in one row on
    every size used here), entered from above once at either cell: the second cell is reached only across the boundary"""
    out = []
    for c in range(64, hw * hw, 64):
        y, x = divmod(c, hw)
        assert x >= 1 and 2 <= y < hw - 1
        for enter in (x - 1, x):
            ring = {(y, x - 2), (y, x + 1), (y - 1, x - 1), (y - 1, x), (y + 1, x - 1), (y + 1, x)} - {(y - 1, enter)}
            walls = sorted(p for p in ring if 0 <= p[1] < hw)
            out.append(R.board(hw, hw, [([(y - 1, enter), (y - 2, enter)], 2), (walls, 0)]))
    return out


def _empty(hw):
    """a mover of length 1 in the middle and a dead second snake: every other cell is reachable, NC - 1, and not one more"""
    return R.board(hw, hw, [([(hw // 2, hw // 2)], 0), ([(0, 0), (0, 1)], 1)], dead=[1])


@pytest.mark.parametrize("hw", [7, 11, 19, 9])
def test_hand_built_boards_through_import_states(hw):
    nc = hw * hw
    pockets, words = _edge_pockets(hw), _word_pockets(hw)
    assert len(words) == 2 * ((nc - 1) // 64)                                 # 7x7: none; 9x9, 11x11: one boundary; 19x19: five
    boards = [_serpentine(hw), _empty(hw)] + pockets + words
    pairs = _alive_pairs(boards)
    cap = 1 << (nc + 1).bit_length()                                          # the ring's size: the power of two from NC + 2 up
    assert cap // 2 < nc + 2 <= cap
    for ring_start in (0, cap - 1, cap - 40):                                 # laid out from the ring's start, and wrapping past its end
        eng = _engine_with(hw, hw, 2, boards, ring_start)
        for flags in range(8) if ring_start == 0 else (R.ALL,):
            got = _values(eng, pairs, flags)
            assert np.array_equal(got, _want(hw, hw, boards, pairs, flags)), (hw, ring_start, flags)
    row = {tuple(p): got[i] for i, p in enumerate(pairs)}
    corridor = (hw + 1) // 2 * hw + (hw - 1) // 2 - 2                         # the even rows, a door per wall, less the mover
    assert row[(0, 0)].tolist() == [-1, (5 * 64) * 512 + min(corridor, 511), -1] and corridor > nc // 2 - 2
    assert row[(1, 0)].tolist() == [(3 * 64) * 512 + min(nc - 1, 511)] * 3                     # the empty board: NC - 1 cells
    for g in range(2, 2 + len(pockets)):
        assert row[(g, 0)][1] % 512 == 1, f"the pocket of board {g} leaks"
    for g in range(2 + len(pockets), len(boards)):
        assert row[(g, 0)][1] % 512 == 2, f"the two cells of board {g} are not one region"


def test_the_cpu_tests_hand_worked_boards():
    """tests/test_script_cpu.py's boards and the numbers worked out by hand there"""
    import test_script_cpu as TC
    for S in (2, 4):
        names = [k for k, v in TC.BOARDS.items() if len(v[0]["alive"]) == S]
        eng = _engine_with(TC.H, TC.W, S, [TC.BOARDS[k][0] for k in names])
        for flags in range(8):
            got = _values(eng, [(g, TC.BOARDS[k][1]) for g, k in enumerate(names)], flags)
            for g, k in enumerate(names):
                assert got[g].tolist() == TC.by_flags(TC.BOARDS[k][3], TC.BOARDS[k][2], flags), (k, flags)


# ---- 3. edge rows and sizes -----------------------------------------------------------------------------------------------------
def test_dead_and_out_of_range_pairs_and_row_counts():
    H, W, S, boards, eng = _golden("11x11x4")
    n = len(boards)
    dead = np.array([(g, s) for g, st in enumerate(boards) for s in range(S) if not st["alive"][s]], np.int32)
    assert len(dead) > 100
    assert (_values(eng, dead) == -1).all()
    bad = np.array([(-1, 0), (n, 0), (0, S), (0, -1), (1 << 30, 1), (-(1 << 31), 2), (3, 1 << 30), (0, 8)], np.int32)
    assert (_values(eng, bad) == -1).all()
    rng = np.random.RandomState(5)
    for m in (0, 1, 3, 63, 64, 65, 4099):
        pairs = np.stack([rng.randint(0, n, m), rng.randint(0, S, m)], 1).astype(np.int32)
        hit = rng.rand(m) < 0.1
        pairs[hit] = bad[rng.randint(0, len(bad), int(hit.sum()))]
        want = np.array([R.scores(H, W, boards[g], s) if 0 <= g < n and 0 <= s < S else [-1] * 3 for g, s in pairs], np.int64)
        assert np.array_equal(_values(eng, pairs), want.reshape(-1, 3)), m


def test_an_unknown_flag_bit_is_refused():
    import torch
    from snake_engine import EngineError
    from snake_engine._lib import check
    H, W, S, boards, eng = _golden("7x7x2")
    pairs = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    q = torch.full((1, 3), SENT, dtype=torch.float32, device="cuda")
    for flags in (8, 15, 1 << 31):
        with pytest.raises(EngineError, match="flag"):
            check(eng.L.snk_pit_script_values(eng.h, pairs.data_ptr(), 1, flags, q.data_ptr(), 0))
    torch.cuda.synchronize()
    assert (q.cpu().numpy() == SENT).all()
    check(eng.L.snk_pit_script_values(eng.h, 0, 0, 7, 0, 0))                  # m = 0 is a no-op, its buffers may be NULL


# ---- 4. whole matches against the statement -------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("name, board, n, flags_b", [("duel-7x7x2", "7x7x2", R.N_DUEL, R.SPACE | R.FOOD),
                                                     ("1v3-11x11x4", "11x11x4", R.N_FOUR, R.HEADS)])
def test_scripted_against_scripted_through_arena_match(name, board, n, flags_b):
    from snake_engine.arena import Arena, Scripted
    from snake_engine.engine import compact_from_state
    want = R.reference(name)
    H, W, S, hd = want["geometry"]
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(SR.start_states(board, n))
    res = arena.match(Scripted(), Scripted(flags_b), 1, spawn_tape=_spawn(want))
    _check_match(res, want, [compact_from_state(s) for s in arena.engine.export()])
    assert len(set(want["winners"])) >= 2 and res.wins_a + res.wins_b + res.draws == n


def test_two_scripted_owners_and_a_stub_net_through_league_play():
    from stubnet_device import DeviceStubNNet
    from snake_engine.arena import Scripted
    from snake_engine.engine import compact_from_state
    from snake_engine.league import League
    want = R.reference("league-11x11x4")
    H, W, S, hd = want["geometry"]
    n, counts = R.N_LEAGUE, []
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(SR.start_states("11x11x4", n))
    res = league.play([Scripted(), Scripted(R.SPACE), DeviceStubNNet()], R.three_owner_table(n), counts_log=counts,
                      spawn_tape=_spawn(want))
    _check_match(res, want, [compact_from_state(s) for s in league.engine.export()], res.winner_owner)
    assert counts == want["counts"]
    assert all(c > 0 for c in want["counts"][0]) and any(0 in c for c in want["counts"]), "every owner moves; one runs out of rows"
    assert len(set(want["winners"])) >= 3


def test_the_same_with_the_stub_searching_through_league_play_search():
    from stubnet_device import DeviceStubNNet
    from snake_engine.arena import Scripted, Searcher
    from snake_engine.engine import compact_from_state
    from snake_engine.league import League
    want = R.reference("league-search-11x11x4")
    H, W, S, hd = want["geometry"]
    n, counts = R.N_SEARCH, []
    searcher = Searcher(DeviceStubNNet(), 8, 4, 100, seed=5, sequential=True, tape_u=SR.uniform_tape(R.TAPE_SEED))
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(SR.start_states("11x11x4", n))
    res = league.play_search([Scripted(), Scripted(R.SPACE), searcher], R.three_owner_table(n), counts_log=counts,
                             spawn_tape=_spawn(want))
    _check_match(res, want, [compact_from_state(s) for s in league.engine.export()], res.winner_owner)
    assert counts == want["counts"], "a turn's read-back"
    assert searcher.tape_pos == want["tape_pos"][2] > 0, "draws consumed"


# ---- 5. read-backs and launches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scripted", [0, 1, 3])
def test_one_read_back_per_turn(monkeypatch, scripted):
    """tests/test_league_gpu.py::test_one_read_back_per_turn with zero, one and all three owners scripted: Tensor.cpu / .item /
    .tolist / .numpy counted over the match -- the K row counts once per turn (and once more to see that no row is left), then
    the winners, their owners and the lengths (.cpu + .numpy each)"""
    import torch
    from stubnet_device import DeviceStubNNet
    from snake_engine.arena import Scripted
    from snake_engine.league import League
    z, p, H, W, S, hd, n, _ = LR.meta(0)
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(LR.start_states(0))
    owner = LR.six_owner_table(n) % 3
    sides = [Scripted(R.ALL - o) if o < scripted else DeviceStubNNet() for o in range(3)]
    torch.cuda.synchronize()
    count = [0]

    def counted(orig):
        def f(self, *a, **k):
            count[0] += 1
            return orig(self, *a, **k)
        return f
    with monkeypatch.context() as mp:
        for name in ("cpu", "item", "tolist", "numpy"):
            mp.setattr(torch.Tensor, name, counted(getattr(torch.Tensor, name)))
        res = league.play(sides, owner)
    assert res.turns >= 3 and count[0] == res.turns + 1 + 6
    assert res.lengths.max() == res.turns and (res.lengths >= 1).all()


class _CountingNet:
    def __init__(self):
        self.rows = []

    def v_device(self, planes, mask):
        from stubnet_device import stub_q_device
        self.rows.append(int(planes.shape[0]))
        return stub_q_device(planes, mask)


def test_observe_and_net_run_over_the_nets_rows_only(monkeypatch):
    """Scripted against Scripted: no observe launch, no net.  A net against Scripted: every observe launch has exactly the rows the
    net is then given, and never more rows than the net's team has snakes"""
    from snake_engine import Engine
    from snake_engine.arena import Arena, Scripted
    observed = []
    orig = Engine.observe_all

    def counting(self, pairs, *a, **k):
        observed.append(int(pairs.shape[0]))
        return orig(self, pairs, *a, **k)
    monkeypatch.setattr(Engine, "observe_all", counting)
    n = 24
    res = Arena(11, 11, 4, 1, n, seed=3).match(Scripted(), Scripted(R.FOOD), 1)
    assert res.turns >= 10 and observed == []
    for a_cnt, net_first in ((1, True), (1, False), (3, True)):
        net = _CountingNet()
        del observed[:]
        sides = (net, Scripted()) if net_first else (Scripted(), net)
        res = Arena(11, 11, 4, 1, n, seed=3).match(*sides, a_cnt)
        seats = a_cnt if net_first else 4 - a_cnt
        assert res.turns >= 3 and observed == net.rows and 1 <= len(observed) <= res.turns
        assert max(observed) <= n * seats and observed[0] == n * seats
        assert res.wins_a + res.wins_b + res.draws == n


# ---- 6. a real net ----------------------------------------------------------------------------------------------------------------
def test_a_real_net_against_the_script_structure():
    from snake_engine.arena import Arena, Scripted
    from snake_engine.net import glorot_uniform_weights
    from utils.alpha_nnet import AlphaNNet
    net = AlphaNNet(input_shape=(13, 13, 3), _weights=glorot_uniform_weights((13, 13, 3), 1, seed=11))
    n = 32
    for sides, a_cnt in (((net, Scripted()), 1), ((Scripted(), net), 1)):
        res = Arena(7, 7, 2, 1, n, seed=5).match(*sides, a_cnt)
        assert res.turns >= 3 and res.wins_a + res.wins_b + res.draws == n
        assert ((res.winners >= -1) & (res.winners < 2)).all() and ((res.lengths >= 1) & (res.lengths <= res.turns)).all()
        assert res.lengths.max() == res.turns


# ---- 7. the refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from stubnet_device import DeviceStubNNet
    from snake_engine.arena import Arena, Scripted, Searcher
    from snake_engine.league import League, round_robin
    net = DeviceStubNNet()
    with pytest.raises(TypeError):
        Searcher(Scripted())
    arena = Arena(7, 7, 2, 1, 4, seed=1)
    with pytest.raises(TypeError):
        arena.match(Scripted(), object())
    league = League(7, 7, 2, 1, 4, seed=1)
    ok = np.array([[0, 1], [1, 0], [0, 1], [1, 1]])
    with pytest.raises(TypeError):
        league.play([Scripted(), Searcher(net, breadth=8, depth=4, seed=1)], ok)
    with pytest.raises(TypeError):
        league.play([Scripted(), object()], ok)
    with pytest.raises(ValueError):
        league.play([Scripted(), net], np.array([[0, 1], [1, 0], [0, 2], [1, 1]]))
    res = league.play([Scripted(), net], ok)                                  # the league still plays after them
    assert res.turns >= 1 and res.winners.shape == (4,) and res.winner_owner[3] in (-1, 1)
    res = arena.match(Searcher(net, breadth=8, depth=4, seed=1), Scripted(), 1)   # a Scripted beside a searching side
    assert res.turns >= 1 and res.wins_a + res.wins_b + res.draws == 4
    t, r = round_robin([Scripted(), Scripted(0), net], games=4, seats="duel", height=7, width=7, seed=3)
    assert np.array_equal(t.wins + t.wins.T + t.draws, t.games) and r.shape == (3,) and np.isfinite(r).all()
