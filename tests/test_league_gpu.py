"""GPU tests of the league (snake_engine/league.py): the four recorded reference pits through League.play with the two-team
table, six stub owners and a four-owner free-for-all against the CPU statement (tests/league_ref.py), the two owner-table
kernels one by one against their NumPy models and against the two-team kernels they generalise, the one read-back per turn,
real nets against Arena.match, and the refusals."""
import functools

import numpy as np
import pytest

import league_ref as R

pytestmark = pytest.mark.gpu

SENT = -7


# ---- 1. the recorded reference pits, two-team table ------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_play_with_the_two_team_table_replays_the_recorded_reference_pit(ci):
    from snake_engine.league import League
    z, p, H, W, S, hd, n, a_cnt = R.meta(ci)
    owner = R.two_team_table(n, S, a_cnt)
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(R.start_states(ci))
    res = league.play([R.DeviceStub(0), R.DeviceStub(1)], owner, spawn_tape=lambda turn: z[p + "spawn"][turn - 1])
    assert res.winners.dtype == np.int32 and res.winners.tolist() == z[p + "winners"].tolist()
    assert res.lengths.dtype == np.int32 and res.lengths.tolist() == z[p + "lengths"].tolist()
    assert res.turns == int(z[p + "lengths"].max())
    w = z[p + "winners"].astype(int)
    assert res.winner_owner.tolist() == [int(owner[g][w[g]]) if w[g] >= 0 else -1 for g in range(n)]


# ---- 2. / 3. six owners and the free-for-all against the CPU statement -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_run(name):
    from snake_engine.engine import compact_from_state
    from snake_engine.league import League
    ci, K, _ = R.CASES[name]
    z, p, H, W, S, hd, n, _ = R.meta(ci)
    want = R.reference(name)
    log, counts = want["spawn_log"], []
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(R.start_states(ci))
    res = league.play([R.DeviceStub(k) for k in range(K)], R.case_table(name), counts_log=counts,
                      spawn_tape=lambda turn: np.maximum(log[turn - 1], -1))
    return res, counts, [compact_from_state(s) for s in league.engine.export()]


def _check_against_reference(name):
    want = R.reference(name)
    res, counts, boards = _device_run(name)
    assert res.turns == want["turns"]
    assert res.winners.tolist() == [-1 if w is None else w for w in want["winners"]]
    assert res.winner_owner.tolist() == [-1 if w is None else w for w in want["winner_owner"]]
    assert res.lengths.tolist() == want["lengths"]
    assert counts == want["counts"]
    for g, (a, b) in enumerate(zip(boards, want["boards"])):
        for k in R.KEYS:
            assert np.array_equal(a[k], b[k]), f"game {g} ({want['lengths'][g]} turns): {k}"
    return want


@pytest.mark.parametrize("name", ["six-owners-run0", "six-owners-run1", "six-owners-run2"])
def test_six_stub_owners_against_the_cpu_statement(name):
    want = _check_against_reference(name)
    R.check_conditions(want)                      # every branch of the verdict; a turn in which an owner has no row


def test_free_for_all_of_four_owners_against_the_cpu_statement():
    want = _check_against_reference("ffa-run1")
    assert {w for w in want["winner_owner"] if w is not None} == {0, 1, 2, 3}


# ---- 4. snk_pit_rows_owned alone ----------------------------------------------------------------------------------------------
def _engine_with_alive(n, hw, S, alive, seed=3):
    """n freshly drawn games whose snakes' alive flags are then set by hand"""
    from snake_engine import Engine
    eng = Engine(n, hw, hw, S, 1, 0.15, seed=seed)
    eng.reset()
    st = eng.export()
    for g in range(n):
        for s in range(S):
            st[g].alive[s] = int(alive[g, s])
    eng.import_states(st)
    assert np.array_equal(eng.alive().cpu().numpy(), alive)
    return eng


def _rows_owned(eng, live, owner, K):
    """-> (pairs with the sentinel past the total, the 16 count cells with the sentinel past K)"""
    import torch
    from snake_engine._lib import check
    n, S = eng.n_slots, eng.S
    d_live, d_owner = torch.as_tensor(live, device="cuda"), torch.as_tensor(np.ascontiguousarray(owner, np.uint8), device="cuda")
    pairs = torch.full((n * S, 2), SENT, dtype=torch.int32, device="cuda")
    counts = torch.full((16,), SENT, dtype=torch.int32, device="cuda")
    scratch = torch.empty((eng.L.snk_pit_owned_scratch_elems(n, K),), dtype=torch.int32, device="cuda")
    check(eng.L.snk_pit_rows_owned(eng.h, d_live.data_ptr(), n, d_owner.data_ptr(), K, pairs.data_ptr(), counts.data_ptr(),
                                   scratch.data_ptr(), 0))
    torch.cuda.synchronize()
    assert np.array_equal(d_live.cpu().numpy(), live) and np.array_equal(d_owner.cpu().numpy(), owner), "an input was written"
    return pairs.cpu().numpy(), counts.cpu().numpy().tolist()


def _check_rows_owned(eng, alive, live, owner, K):
    want, cnt = R.rows_owned_model(alive, live, owner, K)
    got, counts = _rows_owned(eng, live, owner, K)
    m = sum(cnt)
    assert counts[:K] == cnt and counts[K:] == [SENT] * (16 - K), (K, counts, cnt)
    assert np.array_equal(got[:m], want), f"K {K}"
    assert (got[m:] == SENT).all(), "a row past the total was written"
    return got, counts


def _pit_rows(eng, live, a_cnt):
    import torch
    from snake_engine._lib import check
    n, S = eng.n_slots, eng.S
    d_live = torch.as_tensor(live, device="cuda")
    pairs = torch.full((n * S, 2), SENT, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), SENT, dtype=torch.int32, device="cuda")
    scratch = torch.empty((eng.L.snk_pit_scratch_elems(n),), dtype=torch.int32, device="cuda")
    check(eng.L.snk_pit_rows(eng.h, d_live.data_ptr(), n, a_cnt, pairs.data_ptr(), counts.data_ptr(), scratch.data_ptr(), 0))
    return pairs.cpu().numpy(), counts.cpu().numpy().tolist()


ROWS_SHAPES = [(n, 7, S) for n in (1, 3, 1023, 1024, 1025, 5000) for S in (2, 4)] + [(3, 19, 8), (1025, 19, 8)]


@pytest.mark.parametrize("n, hw, S", ROWS_SHAPES)
def test_rows_owned_against_its_model(n, hw, S):
    rng = np.random.RandomState(100 * n + S)
    alive = (rng.rand(n, S) < 0.6).astype(np.uint8)
    alive[0] = 1
    live = (rng.rand(n) < 0.8).astype(np.uint8)
    live[0] = 1
    eng = _engine_with_alive(n, hw, S, alive)
    tile = np.arange(n) // 1024
    for K in (1, 2, 3, 16):
        # every game closed: no row, no count
        got, counts = _check_rows_owned(eng, alive, np.zeros(n, np.uint8), rng.randint(0, K, size=(n, S)).astype(np.uint8), K)
        assert counts[:K] == [0] * K
        # one owner holds every seat
        owner = np.full((n, S), K - 1, np.uint8)
        got, counts = _check_rows_owned(eng, alive, live, owner, K)
        assert counts[:K] == [0] * (K - 1) + [int((alive.astype(bool) & live.astype(bool)[:, None]).sum())]
        # every tile of 1 024 games knows one owner only: the others are absent from whole tiles
        owner = np.repeat(((tile + 1) % K).astype(np.uint8)[:, None], S, axis=1)
        _check_rows_owned(eng, alive, live, owner, K)
        # random tables, and the same call twice
        owner = rng.randint(0, K, size=(n, S)).astype(np.uint8)
        got, counts = _check_rows_owned(eng, alive, live, owner, K)
        again, counts2 = _rows_owned(eng, live, owner, K)
        assert counts2 == counts and np.array_equal(again, got)
        # bytes >= K: the rows of the valid seats only, nothing else written (the checks of _check_rows_owned)
        bad = owner.copy()
        hit = rng.rand(n, S) < 0.3
        bad[hit] = rng.choice([K, K + 1, 16, 200, 255], size=int(hit.sum())).astype(np.uint8)
        bad[0, 0] = 255
        got, counts = _check_rows_owned(eng, alive, live, bad, K)
        assert sum(counts[:K]) < int((alive.astype(bool) & live.astype(bool)[:, None]).sum())
    # the two-team tables: what snk_pit_rows writes
    for a_cnt in sorted({0, 1, S // 2, S}):
        owner = R.two_team_table(n, S, a_cnt)
        got, counts = _check_rows_owned(eng, alive, live, owner, 2)
        want, want_counts = _pit_rows(eng, live, a_cnt)
        assert counts[:2] == want_counts and np.array_equal(got, want), a_cnt


def test_rows_owned_300000_games_carry_between_scan_passes():
    """300 000 games = 293 tiles: the single-block scan of the tile sums takes two passes of 256 and carries every owner's total
    from the first into the second (11x11 with 4 snakes, everything alive as drawn; the open flags and the table are random)"""
    from snake_engine import Engine
    n, S, K = 300000, 4, 16
    eng = Engine(n, 11, 11, S, 1, 0.15, seed=8)
    eng.reset()
    alive = np.ones((n, S), np.uint8)
    assert np.array_equal(eng.alive().cpu().numpy(), alive)
    rng = np.random.RandomState(9)
    live = (rng.rand(n) < 0.7).astype(np.uint8)
    owner = rng.randint(0, K, size=(n, S)).astype(np.uint8)
    owner[:256 * 1024][owner[:256 * 1024] == 5] = 4            # owner 5 appears in the second pass only
    owner[256 * 1024:][owner[256 * 1024:] == 9] = 8            # owner 9 in the first pass only
    got, counts = _check_rows_owned(eng, alive, live, owner, K)
    assert min(counts) > 0
    first = got[:sum(counts)][:, 0] < 256 * 1024
    assert first.any() and (~first).any()


def test_rows_owned_refuses_an_owner_count_outside_1_to_16():
    import torch
    from snake_engine import Engine, EngineError
    from snake_engine._lib import check
    eng = Engine(4, 7, 7, 2, 1, 0.15, seed=1)
    eng.reset()
    live = torch.ones(4, dtype=torch.uint8, device="cuda")
    owner = torch.zeros((4, 2), dtype=torch.uint8, device="cuda")
    pairs = torch.full((8, 2), SENT, dtype=torch.int32, device="cuda")
    counts = torch.full((16,), SENT, dtype=torch.int32, device="cuda")
    scratch = torch.empty((64,), dtype=torch.int32, device="cuda")
    aux = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
    done, rew = torch.zeros(4, dtype=torch.uint8, device="cuda"), torch.zeros((4, 2), dtype=torch.int8, device="cuda")
    for K in (0, 17, -1):
        with pytest.raises(EngineError):
            check(eng.L.snk_pit_rows_owned(eng.h, live.data_ptr(), 4, owner.data_ptr(), K, pairs.data_ptr(), counts.data_ptr(),
                                           scratch.data_ptr(), 0))
        with pytest.raises(EngineError):
            check(eng.L.snk_pit_verdict_owned(eng.h, done.data_ptr(), rew.data_ptr(), 4, owner.data_ptr(), K, 1, live.data_ptr(),
                                              aux.data_ptr(), aux.data_ptr(), aux.data_ptr(), 0))
    torch.cuda.synchronize()
    assert (pairs.cpu().numpy() == SENT).all() and (counts.cpu().numpy() == SENT).all() and (aux.cpu().numpy() == SENT).all()


# ---- 5. snk_pit_verdict_owned alone -------------------------------------------------------------------------------------------
def _verdict_owned(eng, done, rew, owner, K, turn, live, winner, wowner, length):
    """arrays on the host in, the four written arrays on the host out"""
    import torch
    from snake_engine._lib import check
    d = [torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in (done, rew, owner, live, winner, wowner, length)]
    check(eng.L.snk_pit_verdict_owned(eng.h, d[0].data_ptr(), d[1].data_ptr(), eng.n_slots, d[2].data_ptr(), K, turn, d[3].data_ptr(),
                                      d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), 0))
    torch.cuda.synchronize()
    assert np.array_equal(d[2].cpu().numpy(), owner)
    return tuple(t.cpu().numpy() for t in d[3:])


def test_verdict_owned_every_case():
    #              alive          done  rewards           owner         live   -> winner, owner, length, live
    cases = [
        ([0, 0, 1, 0], 1, [-1, -1, 1, -1], [0, 1, 2, 1], 1, 2, 2, 9, 0),         # done, a single +1
        ([0, 1, 0, 1], 1, [-1, 1, -1, 1], [0, 1, 2, 0], 1, 3, 0, 9, 0),          # done, two +1: the larger id
        ([0, 0, 0, 0], 1, [-1, -1, -1, -1], [0, 1, 2, 1], 1, -1, -1, 9, 0),      # done, none: a draw
        ([0, 1, 0, 1], 0, [-1, 0, -1, 0], [0, 1, 1, 2], 1, -5, -4, -6, 1),       # open, two owners: stays open, nothing written
        ([1, 1, 1, 1], 0, [0, 0, 0, 0], [2, 2, 2, 1], 1, -5, -4, -6, 1),         # open, the last seat alone differs
        ([0, 1, 1, 1], 0, [-1, 0, 0, 0], [0, 2, 2, 2], 1, 1, 2, 9, 0),           # open, one owner left with three snakes
        ([1, 0, 1, 0], 0, [0, -1, 0, -1], [1, 0, 1, 0], 1, 0, 1, 9, 0),          # one owner left on seats no id split gives
        ([0, 0, 0, 1], 0, [-1, -1, -1, 0], [1, 0, 1, 0], 1, 3, 0, 9, 0),         # one snake left
        ([0, 0, 0, 0], 0, [-1, -1, -1, -1], [0, 1, 2, 1], 1, -1, -1, 9, 0),      # open and nobody alive: closed without a winner
        ([0, 0, 1, 0], 1, [-1, -1, 1, -1], [0, 1, 2, 1], 0, -5, -4, -6, 0),      # closed before: untouched although done is set
        ([0, 1, 1, 1], 0, [-1, 0, 0, 0], [0, 2, 2, 2], 0, -5, -4, -6, 0),        # closed before, one owner left: untouched
    ]
    n, S, K, turn = len(cases), 4, 3, 9
    alive = np.array([c[0] for c in cases], np.uint8)
    eng = _engine_with_alive(n, 7, S, alive)
    done, rew = np.array([c[1] for c in cases], np.uint8), np.array([c[2] for c in cases], np.int8)
    owner, live = np.array([c[3] for c in cases], np.uint8), np.array([c[4] for c in cases], np.uint8)
    start = (live, np.full(n, -5, np.int32), np.full(n, -4, np.int32), np.full(n, -6, np.int32))
    before = [bytes(s) for s in eng.export()]
    got_live, winner, wowner, length = _verdict_owned(eng, done, rew, owner, K, turn, *start)
    assert winner.tolist() == [c[5] for c in cases]
    assert wowner.tolist() == [c[6] for c in cases]
    assert length.tolist() == [c[7] for c in cases]
    assert got_live.tolist() == [c[8] for c in cases]
    assert [bytes(s) for s in eng.export()] == before, "the verdict wrote to a game record"
    model = R.verdict_owned_model(alive, done, rew, owner, turn, *start)
    for a, b in zip((got_live, winner, wowner, length), model):
        assert np.array_equal(a, b)


def test_verdict_owned_with_two_team_tables_is_the_two_team_verdict():
    import torch
    from snake_engine._lib import check
    n, S, turn = 2000, 4, 31
    rng = np.random.RandomState(12)
    alive = (rng.rand(n, S) < 0.5).astype(np.uint8)
    eng = _engine_with_alive(n, 7, S, alive)
    done = (rng.rand(n) < 0.4).astype(np.uint8)
    rew = rng.randint(-1, 2, size=(n, S)).astype(np.int8)
    live = (rng.rand(n) < 0.85).astype(np.uint8)
    start = (live, np.full(n, -5, np.int32), np.full(n, -4, np.int32), np.full(n, -6, np.int32))
    for a_cnt in (0, 1, 2, 3, 4):
        owner = R.two_team_table(n, S, a_cnt)
        got = _verdict_owned(eng, done, rew, owner, 2, turn, *start)
        d = [torch.as_tensor(a, device="cuda") for a in (done, rew, start[0], start[1], start[3])]
        check(eng.L.snk_pit_verdict(eng.h, d[0].data_ptr(), d[1].data_ptr(), n, a_cnt, turn, d[2].data_ptr(), d[3].data_ptr(),
                                    d[4].data_ptr(), 0))
        assert np.array_equal(got[0], d[2].cpu().numpy()) and np.array_equal(got[1], d[3].cpu().numpy()), a_cnt
        assert np.array_equal(got[3], d[4].cpu().numpy()), a_cnt
        model = R.verdict_owned_model(alive, done, rew, owner, turn, *start)
        for a, b in zip(got, model):
            assert np.array_equal(a, b), a_cnt
        if 0 < a_cnt < S:
            closed = (got[0] == 0) & (live == 1)
            assert closed.any() and ((got[0] == 1).any()) and (got[2][closed] >= 0).any() and (got[2][closed] < 0).any()
    # random tables of five owners against the model
    owner = rng.randint(0, 5, size=(n, S)).astype(np.uint8)
    got = _verdict_owned(eng, done, rew, owner, 5, turn, *start)
    for a, b in zip(got, R.verdict_owned_model(alive, done, rew, owner, turn, *start)):
        assert np.array_equal(a, b)


# ---- 6. one read-back per turn ------------------------------------------------------------------------------------------------
def test_one_read_back_per_turn(monkeypatch):
    """Tensor.cpu / .item / .tolist / .numpy counted over a match of three device stub nets: the K row counts once per turn (and
    once more to see that no row is left), then the winners, their owners and the lengths (.cpu + .numpy each)"""
    import torch
    from stubnet_device import DeviceStubNNet
    from snake_engine.league import League
    z, p, H, W, S, hd, n, _ = R.meta(0)
    league = League(H, W, S, hd, n, seed=1)
    league.import_states(R.start_states(0))
    owner = R.six_owner_table(n) % 3
    nets = [DeviceStubNNet() for _ in range(3)]
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
        res = league.play(nets, owner)
    assert res.turns >= 3 and count[0] == res.turns + 1 + 6
    assert res.lengths.max() == res.turns and (res.lengths >= 1).all()


# ---- 7. real nets ---------------------------------------------------------------------------------------------------------------
def _real_nets(seeds):
    from snake_engine.net import glorot_uniform_weights
    from utils.alpha_nnet import AlphaNNet
    return [AlphaNNet(input_shape=(13, 13, 3), _weights=glorot_uniform_weights((13, 13, 3), 1, seed=s)) for s in seeds]


def test_two_real_nets_play_what_arena_match_plays():
    """the same engine seed, the same batches, the same launches: the winners, lengths and turns of Arena.match exactly"""
    from snake_engine.arena import Arena
    from snake_engine.league import League
    nets = _real_nets((11, 12))
    n, S, a_cnt = 32, 2, 1

    def play():
        a = Arena(7, 7, S, 1, n, seed=5).match(nets[0], nets[1], a_cnt)
        b = League(7, 7, S, 1, n, seed=5).play(nets, R.two_team_table(n, S, a_cnt))
        return a, b
    trips = sum(net._qnet.guard_trips for net in nets)
    a, b = play()
    if sum(net._qnet.guard_trips for net in nets) != trips:      # a range guard widened a scale half way: play with settled scales
        a, b = play()
    assert a.turns >= 3 and b.turns == a.turns
    assert np.array_equal(b.winners, a.winners) and np.array_equal(b.lengths, a.lengths)
    assert b.winner_owner.tolist() == [-1 if w < 0 else int(w >= a_cnt) for w in a.winners]


def test_round_robin_of_three_real_nets_structure():
    from snake_engine.league import round_robin, schedule
    nets = _real_nets((21, 22, 23))
    t, r = round_robin(nets, games=8, seats="duel", height=7, width=7, seed=3)
    assert t.wins.shape == t.draws.shape == t.games.shape == (3, 3)
    assert np.array_equal(t.wins + t.wins.T + t.draws, t.games)
    assert (t.games[~np.eye(3, dtype=bool)] == 16).all() and (np.diag(t.games) == 0).all()
    assert ((t.score >= 0) & (t.score <= 1)).all()
    assert r.shape == (3,) and np.isfinite(r).all() and r[0] == 0.0
    # every winner's owner sits in its game
    from snake_engine.league import League
    owner = schedule(3, 8, "duel")
    res = League(7, 7, 2, 1, len(owner), seed=3).play(nets, owner)
    for g in range(len(owner)):
        assert res.winner_owner[g] == (owner[g][res.winners[g]] if res.winners[g] >= 0 else -1)
        assert -1 <= res.winners[g] < 2 and 1 <= res.lengths[g] <= res.turns


# ---- 8. the refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    from stubnet_device import DeviceStubNNet
    from snake_engine.arena import Searcher
    from snake_engine.league import League
    league = League(7, 7, 2, 1, 4, seed=1)
    net = DeviceStubNNet()
    ok = np.zeros((4, 2), np.uint8)
    with pytest.raises(ValueError):
        league.play([net] * 17, ok)
    with pytest.raises(ValueError):
        league.play([], ok)
    with pytest.raises(ValueError):
        league.play([net, net], np.array([[0, 1], [1, 0], [0, 2], [1, 1]]))       # an owner value of K
    with pytest.raises(ValueError):
        league.play([net, net], np.array([[0, 1], [1, 0], [0, -1], [1, 1]]))
    with pytest.raises(ValueError):
        league.play([net, net], np.zeros((4, 3), np.uint8))                       # a table of the wrong shape
    with pytest.raises(ValueError):
        league.play([net, net], np.zeros((3, 2), np.uint8))
    with pytest.raises(ValueError):
        league.play([net, net], np.zeros((4, 2), np.float32))
    with pytest.raises(TypeError):
        league.play([net, Searcher(net, breadth=8, depth=4, seed=1)], ok)
    with pytest.raises(TypeError):
        league.play([net, object()], ok)
    res = league.play([net, net], np.array([[0, 1], [1, 0], [0, 1], [1, 1]]))     # the league still plays after them
    assert res.turns >= 1 and res.winners.shape == (4,) and res.winner_owner[3] in (-1, 1)
