"""GPU tests of the searching league (League.play_search): snk_pit_roots_owned and snk_pit_search_moves_owned one by one against
their NumPy models (tests/league_search_ref.py) and against the two-team kernels they generalise; whole matches of three and four
owners, searching and greedy in every mix, against the CPU statement in the sequential, taped parity mode; two Searchers with the
two-team table against Arena.match; no Searcher against League.play; the league's one read-back per turn; the production mode
between real nets; the refusals."""
import numpy as np
import pytest

import league_ref as LR
import league_search_ref as R
import search_pit_ref as SR
from test_arena_search_gpu import SIZES, _count, _pit_roots, _played_engine

pytestmark = pytest.mark.gpu

SENT = -7
KS = (1, 2, 3, 16)


def _masks(K):
    return {"none": 0, "all": (1 << K) - 1, "alternating": 0x5555 & ((1 << K) - 1), "odd, and bits past K": 0xAAAA0000 | (0xAAAA & ((1 << K) - 1))}


def _lives(n):
    sparse = (np.random.RandomState(n).rand(n) < 0.3).astype(np.uint8)
    sparse[-1] = 1
    return {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "sparse": sparse}


def _owners(n, S, K, rng):
    """random owners, a fifth of the bytes out of range"""
    owner = rng.randint(0, K, size=(n, S)).astype(np.uint8)
    hit = rng.rand(n, S) < 0.2
    owner[hit] = rng.choice([K, K + 1, 16, 200, 255], size=int(hit.sum())).astype(np.uint8)
    return owner


def _roots_owned(eng, live, owner, K, mask):
    """-> counts (16 cells, the sentinel past K), slots, alive rows, rank on the host, all pre-filled with sentinels"""
    import torch
    from snake_engine._lib import check
    n, S = eng.n_slots, eng.S
    d_live, d_owner = torch.as_tensor(live, device="cuda"), torch.as_tensor(np.ascontiguousarray(owner, np.uint8), device="cuda")
    counts = torch.full((16,), SENT, dtype=torch.int32, device="cuda")
    slots = torch.full((n * S,), SENT, dtype=torch.int32, device="cuda")
    alive = torch.full((n * S, S), 9, dtype=torch.uint8, device="cuda")
    rank = torch.full((n, S), SENT, dtype=torch.int32, device="cuda")
    scratch = torch.empty((eng.L.snk_pit_owned_scratch_elems(n, K),), dtype=torch.int32, device="cuda")
    check(eng.L.snk_pit_roots_owned(eng.h, d_live.data_ptr(), n, d_owner.data_ptr(), K, mask, counts.data_ptr(), slots.data_ptr(),
                                    alive.data_ptr(), rank.data_ptr(), scratch.data_ptr(), 0))
    torch.cuda.synchronize()
    assert np.array_equal(d_live.cpu().numpy(), live) and np.array_equal(d_owner.cpu().numpy(), owner), "an input was written"
    return counts.cpu().numpy().tolist(), slots.cpu().numpy(), alive.cpu().numpy(), rank.cpu().numpy()


def _check_roots_owned(eng, alive_all, live, owner, K, mask, tag):
    want_counts, want_slots, want_rows, want_rank = R.roots_owned_model(alive_all, live, owner, K, mask)
    counts, slots, rows, rank = _roots_owned(eng, live, owner, K, mask)
    assert counts[:K] == want_counts and counts[K:] == [SENT] * (16 - K), (tag, counts, want_counts)
    if want_slots is None:                                                 # a no-op: nothing but the counts
        assert (slots == SENT).all() and (rows == 9).all() and (rank == SENT).all(), tag
        return counts, slots, rows, rank
    total = sum(want_counts)
    assert np.array_equal(slots[:total], want_slots) and np.array_equal(rows[:total], want_rows), tag
    assert (slots[total:] == SENT).all() and (rows[total:] == 9).all(), f"{tag}: written past the counts"
    assert np.array_equal(rank, want_rank), tag
    return counts, slots, rows, rank


# ---- 1. snk_pit_roots_owned against its model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S", SIZES)
def test_roots_owned_against_its_model(n, S):
    eng, alive = _played_engine(n, S)
    rng = np.random.RandomState(7 * n + S)
    seen = 0
    for K in KS:
        owner = _owners(n, S, K, rng)
        for mtag, mask in _masks(K).items():
            for ltag, live in _lives(n).items():
                counts, *_ = _check_roots_owned(eng, alive, live, owner, K, mask, f"K {K}, mask {mtag}, live {ltag}")
                seen = max(seen, sum(counts[:K]))
    assert seen > 0
    if n >= 63:                                                            # one owner on every seat: its list is the open games
        live = _lives(n)["sparse"]
        counts, slots, _, _ = _check_roots_owned(eng, alive, live, np.zeros((n, S), np.uint8), 2, 0b11, "one owner")
        assert counts[:2] == [int((live.astype(bool) & alive.any(1)).sum()), 0]
    if n == 300000:                                                        # both passes of the tile-sum scan hold games
        live = _lives(n)["sparse"]
        assert live[:256 * 1024].any() and live[256 * 1024:].any()


def test_roots_owned_no_game_and_bad_owner_counts():
    import torch
    from snake_engine import EngineError
    from snake_engine._lib import check
    eng, _ = _played_engine(1, 4)
    counts = torch.full((16,), SENT, dtype=torch.int32, device="cuda")
    check(eng.L.snk_pit_roots_owned(eng.h, 0, 0, 0, 3, 7, counts.data_ptr(), 0, 0, 0, 0, 0))
    assert counts.cpu().numpy().tolist() == [0] * 3 + [SENT] * 13
    for K in (0, 17, -1):
        with pytest.raises(EngineError):
            check(eng.L.snk_pit_roots_owned(eng.h, 0, 0, 0, K, 1, counts.data_ptr(), 0, 0, 0, 0, 0))
    with pytest.raises(EngineError):
        check(eng.L.snk_pit_roots_owned(eng.h, 0, 2, 0, 2, 3, counts.data_ptr(), 0, 0, 0, 0, 0))       # more games than slots


# ---- 2. the two-team table: what snk_pit_roots writes -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S", SIZES)
def test_roots_owned_with_the_two_team_table_is_pit_roots(n, S):
    """mask 0b11 on games in which both teams have a snake, which is what the verdict leaves open: each owner's list is
    snk_pit_roots' list, and d_rank is snk_pit_roots' rank plus the owner's base on every alive seat of an open game"""
    eng, alive = _played_engine(n, S)
    for a_cnt in sorted({1, S // 2, S - 1}):
        both = alive[:, :a_cnt].any(1) & alive[:, a_cnt:].any(1)
        for ltag, live in _lives(n).items():
            live = (live.astype(bool) & both).astype(np.uint8)
            owner = LR.two_team_table(n, S, a_cnt)
            counts, slots, rows, rank = _check_roots_owned(eng, alive, live, owner, 2, 0b11, f"a_cnt {a_cnt}, live {ltag}")
            p_slots, p_alive, p_rank, G = _pit_roots(eng, live)
            p_slots, p_alive, p_rank = p_slots.cpu().numpy(), p_alive.cpu().numpy(), p_rank.cpu().numpy()
            assert counts[:2] == [G, G]
            for o in (0, 1):
                assert np.array_equal(slots[o * G:(o + 1) * G], p_slots[:G]) and np.array_equal(rows[o * G:(o + 1) * G], p_alive[:G])
            seat = alive.astype(bool) & live.astype(bool)[:, None]
            want = np.where(seat, p_rank[:, None] + G * owner.astype(np.int32), -1)
            assert np.array_equal(rank, want), (a_cnt, ltag)


# ---- 3. snk_pit_search_moves_owned against its model --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S", SIZES)
def test_search_moves_owned_against_its_model(n, S):
    import torch
    from snake_engine._lib import check
    eng, alive = _played_engine(n, S)
    rng = np.random.RandomState(11 * n + S)
    for K in KS:
        owner = _owners(n, S, K, rng)
        for mtag, mask in _masks(K).items():
            for ltag, live in _lives(n).items():
                counts, _, _, rank = R.roots_owned_model(alive, live, owner, K, mask)
                if rank is None:                                           # no list: every cell is a cell without a row
                    rank = np.full((n, S), -1, np.int32)
                total = sum(counts)
                found = rng.randint(0, 3, size=(max(total, 1), S)).astype(np.uint8)
                before = rng.randint(3, 9, size=(n, S)).astype(np.uint8)
                d_found, d_rank = torch.as_tensor(found, device="cuda"), torch.as_tensor(rank, device="cuda")
                for keep in (0, 1):
                    moves = torch.as_tensor(before, device="cuda")
                    check(eng.L.snk_pit_search_moves_owned(d_found.data_ptr() if total else 0, d_rank.data_ptr(), n, S, total, keep,
                                                           moves.data_ptr(), 0))
                    want = R.search_moves_owned_model(found, rank, total, keep, before)
                    assert np.array_equal(moves.cpu().numpy(), want), f"K {K}, mask {mtag}, live {ltag}, keep {keep}"
                    assert keep or (want < 3).all()                        # without keep_other every cell has a writer
                assert np.array_equal(d_rank.cpu().numpy(), rank) and np.array_equal(d_found.cpu().numpy(), found)


# ---- 4. whole matches against the CPU statement --------------------------------------------------------------------------------------
def _device_net(o):
    """stub number o behind v_device: 0 and 1 evaluate on the device, the others on the host from the device's observations"""
    return SR.DeviceStub(o) if o < 2 else LR.DeviceStub(o)


@pytest.mark.parametrize("name", list(R.CASES))
def test_play_search_replays_the_cpu_statement(name):
    from snake_engine.arena import Searcher
    from snake_engine.engine import compact_from_state
    from snake_engine.league import League
    board, breadth, searching, seed = R.CASES[name]
    want = R.reference(name)
    R.check_well_posed(want)
    R.check_conditions(name, want)
    table = R.TABLES[board]()
    n, K = len(table), len(searching)
    H, W, S, hd = want["geometry"]
    tapes = R.tapes(seed, K)
    sides = [Searcher(_device_net(o), breadth, 4, 100, seed=5 + o, sequential=True, tape_u=tapes[o]) if s else _device_net(o)
             for o, s in enumerate(searching)]
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(SR.start_states(board, n))
    log, counts = want["spawn_log"], []
    res = league.play_search(sides, table, counts_log=counts, spawn_tape=lambda turn: np.maximum(log[turn - 1], -1))
    assert res.turns == want["turns"]
    assert res.winners.tolist() == [-1 if w is None else w for w in want["winners"]]
    assert res.winner_owner.tolist() == [-1 if w is None else w for w in want["winner_owner"]]
    assert res.lengths.tolist() == want["lengths"]
    assert counts == want["counts"], "a turn's read-back"
    for side, pos in zip(sides, want["tape_pos"]):
        assert isinstance(side, Searcher) == (pos is not None)
        if pos is not None:
            assert side.tape_pos == pos, "draws consumed"
    got = [compact_from_state(s) for s in league.engine.export()]
    for g in range(n):
        for k in R.KEYS:
            assert np.array_equal(got[g][k], want["boards"][g][k]), f"game {g} ({want['lengths'][g]} turns): {k}"


# ---- 5. two Searchers with the two-team table: Arena.match ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["7x7x2-b8-search-v-search", "11x11x4-b8-search-v-search"])
def test_two_searchers_with_the_two_team_table_play_what_arena_match_plays(name):
    from snake_engine.arena import Arena, Searcher
    from snake_engine.league import League
    board, n, breadth, searching, seed = SR.CASES[name]
    ref = SR.reference(name)
    H, W, S, hd = ref["geometry"]
    log = ref["spawn_log"]
    spawn = lambda turn: np.maximum(log[turn - 1], -1)
    make = lambda: [Searcher(SR.DeviceStub(w), breadth, 4, 100, seed=5, sequential=True, tape_u=SR.uniform_tape(seed)) for w in (0, 1)]
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(SR.start_states(board, n))
    a_sides = make()
    a = arena.match(a_sides[0], a_sides[1], 1, spawn_tape=spawn)
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(SR.start_states(board, n))
    l_sides = make()
    b = league.play_search(l_sides, LR.two_team_table(n, S, 1), spawn_tape=spawn)
    assert a.turns == b.turns >= 3
    assert np.array_equal(a.winners, b.winners) and np.array_equal(a.lengths, b.lengths)
    assert b.winner_owner.tolist() == [-1 if w < 0 else int(w >= 1) for w in a.winners]
    for x, y in zip(a_sides, l_sides):
        assert x.tape_pos == y.tape_pos > 0 and x.stats == y.stats and x.stats["net_evals"] > 0


# ---- 6. no Searcher: League.play -------------------------------------------------------------------------------------------------------
def test_play_search_without_a_searcher_is_play():
    from snake_engine.league import League
    name = "ffa-run1"
    ci, K, _ = LR.CASES[name]
    z, p, H, W, S, hd, n, _ = LR.meta(ci)
    log = LR.reference(name)["spawn_log"]
    spawn = lambda turn: np.maximum(log[turn - 1], -1)
    out = []
    for method in ("play", "play_search"):
        league = League(H, W, S, hd, n, seed=1)
        league.import_states(LR.start_states(ci))
        counts = []
        res = getattr(league, method)([LR.DeviceStub(k) for k in range(K)], LR.case_table(name), counts_log=counts, spawn_tape=spawn)
        out.append((res, counts))
        assert league._roots is None                          # the searching turn's buffers were never made
    (a, ca), (b, cb) = out
    assert a.turns == b.turns >= 3 and ca == cb == LR.reference(name)["counts"]
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)


# ---- 7. the league's own read-backs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("searching", [(False, False, False), (True, False, True), (True, True, True)])
def test_league_reads_back_once_per_turn(monkeypatch, searching):
    """.tolist() calls made in league.py, with Searcher.search replaced by a stub that returns all-straight moves without
    synchronising: one per turn and one more that sees all zeros"""
    import torch
    from stubnet_device import DeviceStubNNet
    from snake_engine import arena as A
    from snake_engine.league import League
    z, p, H, W, S, hd, n, _ = LR.meta(0)
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(LR.start_states(0))
    owner = LR.six_owner_table(n) % 3
    calls = []

    def straight(self, engine, slots, alive):
        calls.append(int(slots.shape[0]))
        assert alive.shape == (slots.shape[0], S) and slots.dtype == torch.int32 and alive.dtype == torch.uint8
        assert slots.is_contiguous() and alive.is_contiguous()
        return torch.ones((slots.shape[0], S), dtype=torch.uint8, device=slots.device)
    monkeypatch.setattr(A.Searcher, "search", straight)
    sides = [A.Searcher(DeviceStubNNet(), 8, 4) if s else DeviceStubNNet() for s in searching]
    counts = []
    res, got = _count(monkeypatch, ("tolist",), lambda: league.play_search(sides, owner, counts_log=counts), only_file="league.py")
    assert res.turns >= 3 and got == res.turns + 1
    Kg = searching.count(False)
    width = Kg + 3 if any(searching) else 3                                # without a Searcher the read-back is play's K row counts
    assert len(counts) == res.turns and all(len(row) == width for row in counts)
    assert len(calls) == (sum(1 for row in counts for c in row[Kg:] if c) if any(searching) else 0) and (len(calls) > 0) == any(searching)
    assert res.lengths.max() == res.turns and (res.lengths >= 1).all()


# ---- 8. production mode ----------------------------------------------------------------------------------------------------------------
def test_production_mode_match_of_three_real_nets():
    """Philox draws, float atomics in the back-ups: structural invariants only.  Whether two runs with the same seeds were
    identical is printed, not asserted (production-mode back-ups are not pinned run to run)"""
    from snake_engine.arena import Searcher
    from snake_engine.league import League, schedule, table
    from snake_engine.net import glorot_uniform_weights
    from utils.alpha_nnet import AlphaNNet
    nets = [AlphaNNet(input_shape=(13, 13, 3), _weights=glorot_uniform_weights((13, 13, 3), 1, seed=s)) for s in (31, 32, 33)]
    owner = schedule(3, 4, "duel")
    assert len(owner) == 24

    def play():
        sides = [Searcher(nets[0], 8, 4, seed=41), Searcher(nets[1], 8, 4, seed=42), nets[2]]
        res = League(7, 7, 2, 1, 24, seed=5).play_search(sides, owner)
        assert all(s.stats["net_evals"] > 0 and s.stats["rollout_ticks"] >= 1 for s in sides[:2])
        return res
    runs = [play(), play()]
    for res in runs:
        assert res.turns >= 3 and (res.lengths >= 1).all() and res.lengths.max() == res.turns      # every game has a verdict
        assert ((res.winners >= -1) & (res.winners < 2)).all()
        for g in range(24):
            assert res.winner_owner[g] == (owner[g][res.winners[g]] if res.winners[g] >= 0 else -1)
        t = table(res, owner, 3)                                           # raises if a winner's owner holds no seat of its game
        assert np.array_equal(t.wins + t.wins.T + t.draws, t.games)
    same = all(np.array_equal(x, y) for x, y in zip(runs[0][:3], runs[1][:3]))
    print(f"\nproduction-mode league, two searchers and a greedy net, 24 duels, breadth 8, same seeds twice: identical = {same}; "
          f"turns {runs[0].turns} / {runs[1].turns}, winners' owners {np.bincount(runs[0].winner_owner + 1, minlength=4).tolist()} / "
          f"{np.bincount(runs[1].winner_owner + 1, minlength=4).tolist()}")


# ---- 9. the refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from stubnet_device import DeviceStubNNet
    from snake_engine.arena import Searcher
    from snake_engine.league import League
    league = League(7, 7, 2, 1, 4, seed=1)
    net = DeviceStubNNet()
    ok = np.array([[0, 1], [1, 0], [0, 1], [1, 1]])
    one = Searcher(net, breadth=8, depth=4, seed=1)
    with pytest.raises(ValueError):
        league.play_search([one, one], ok)
    with pytest.raises(TypeError):
        league.play([net, one], ok)
    with pytest.raises(TypeError):
        league.play_search([one, object()], ok)
    res = league.play_search([one, net], ok)                               # the league still plays after them
    assert res.turns >= 1 and res.winners.shape == (4,) and res.winner_owner[3] in (-1, 1)
