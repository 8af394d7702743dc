"""GPU tests of the device-resident arena (snake_engine/arena.py): whole pit matches against the four runs the unmodified
reference recorded (tests/golden/pit.npz) and against the host loop `MPGameRunner.run`, the three pit kernels one by one
against NumPy restatements of the reference lines they replace, the frozen records of retired games, the one host
read-back per turn, and a match between two real nets."""
import functools

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

KEYS = ("alive", "health", "length", "dir", "nodes", "food", "rewards", "counters")


class _Stub:
    """the deterministic stub Q function of the recorded runs (oracle/obs_key.py) behind the v_device contract"""

    def __init__(self, which):
        self.which = which

    def v_device(self, planes, mask):
        import torch
        from oracle.obs_key import stub_q
        q = stub_q(planes.cpu().numpy(), which=self.which)
        assert np.array_equal(q == -1.0, mask.cpu().numpy().astype(bool))
        return torch.as_tensor(q, device=planes.device)


def _meta(ci):
    z = load_golden("pit.npz")
    p = f"p{ci}_"
    H, W, S, hd, n, a_cnt = (int(v) for v in z[p + "meta"])
    return z, p, H, W, S, hd, n, (None if a_cnt < 0 else a_cnt)


def _start_states(z, p, H, W, S, n):
    from snake_engine.engine import state_from_compact
    return [state_from_compact(H, W, S, {k: z[p + "init_" + k][g] for k in KEYS}) for g in range(n)]


@functools.lru_cache(maxsize=None)
def _arena_run(ci):
    """Arena.match on the recorded start boards and spawn tape of run ci -> (result, exported records after the match)"""
    from snake_engine.arena import Arena
    from snake_engine.engine import compact_from_state
    z, p, H, W, S, hd, n, a_cnt = _meta(ci)
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(_start_states(z, p, H, W, S, n))
    res = arena.match(_Stub(0), _Stub(1), a_cnt, spawn_tape=lambda turn: z[p + "spawn"][turn - 1])
    return res, [compact_from_state(s) for s in arena.engine.export()]


@functools.lru_cache(maxsize=None)
def _oracle_run(ci):
    """the CPU restatement of the pit loop on the same boards -> (winners, lengths, every game's board at its verdict)"""
    from oracle import snake_oracle
    from oracle.obs_key import StubNet
    from oracle.pit_oracle import pit_run
    z, p, H, W, S, hd, n, a_cnt = _meta(ci)
    games = [snake_oracle.Game.from_compact(H, W, S, hd, 0.15, {k: z[p + "init_" + k][g] for k in KEYS}) for g in range(n)]
    winners, lengths = pit_run(games, StubNet(0), StubNet(1), a_cnt, spawn_tape=lambda turn: z[p + "spawn"][turn - 1])
    return winners, lengths, [g.compact() for g in games]      # pit_run does not tic a game again after its verdict


# ---- 1. the recorded reference pits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_match_replays_the_recorded_reference_pit(ci):
    z, p, H, W, S, hd, n, a_cnt = _meta(ci)
    res, _ = _arena_run(ci)
    assert res.winners.dtype == np.int32 and res.winners.tolist() == z[p + "winners"].tolist()
    assert res.lengths.tolist() == z[p + "lengths"].tolist()
    assert res.turns == int(z[p + "lengths"].max()) <= len(z[p + "spawn"])
    a = S // 2 if a_cnt is None else a_cnt
    w = z[p + "winners"].astype(int)
    assert (res.wins_a, res.wins_b, res.draws) == (int(((w >= 0) & (w < a)).sum()), int((w >= a).sum()), int((w < 0).sum()))
    assert res.wins_a + res.wins_b + res.draws == n


def test_the_recorded_pits_take_every_branch_of_the_verdict():
    """pit_mp_game_runner.py:43-47 with and without a +1 reward, :48-60 with team A gone and with team B gone: which branch
    closed a game is read off the board its verdict was taken on (a finished game has at most one snake left)"""
    seen = set()
    for ci in range(4):
        z, p, H, W, S, hd, n, a_cnt = _meta(ci)
        a = S // 2 if a_cnt is None else a_cnt
        res, boards = _arena_run(ci)
        for g in range(n):
            alive = np.flatnonzero(boards[g]["alive"])
            if len(alive) <= 1:
                seen.add("done, winner" if res.winners[g] >= 0 else "done, draw")
                assert (res.winners[g] >= 0) == (len(alive) == 1)
            else:
                seen.add("team B gone" if (alive < a).all() else "team A gone")
                assert (alive < a).all() or (alive >= a).all()
                assert res.winners[g] == alive[0]
    assert seen == {"done, winner", "done, draw", "team A gone", "team B gone"}, seen


# ---- 2. run_device against run -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_run_device_returns_what_run_returns(ci):
    from utils.pit_agent import Agent
    from utils.pit_mp_game_runner import MPGameRunner
    z, p, H, W, S, hd, n, a_cnt = _meta(ci)
    got = []
    for form in ("run", "run_device"):
        gr = MPGameRunner(H, W, S, hd, n, seed=1)
        gr.engine.import_states(_start_states(z, p, H, W, S, n))
        for g in gr.games.values():
            g._dirty()
        got.append(getattr(gr, form)(Agent(_Stub(0)), Agent(_Stub(1)), a_cnt, spawn_tape=lambda turn: z[p + "spawn"][turn - 1]))
        assert len(gr.games) == 0
    assert got[0] == got[1] and len(got[1]) == n
    assert [-1 if w is None else w for w in got[1]] == z[p + "winners"].tolist()
    assert (None in got[1]) == bool((z[p + "winners"] < 0).any()) and all(w is None or type(w) is int for w in got[1])


# ---- 3. snk_pit_rows alone -------------------------------------------------------------------------------------------------------
def _rows_model(alive, live, a_cnt):
    """pit_mp_game_runner.py:23-35: ids_A + ids_B over the live games"""
    gi, si = np.nonzero(alive.astype(bool) & live.astype(bool)[:, None])
    A = si < a_cnt
    pairs = np.concatenate([np.stack([gi[A], si[A]], 1), np.stack([gi[~A], si[~A]], 1)]).astype(np.int32)
    return pairs, int(A.sum()), int((~A).sum())


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


def _pit_rows(eng, live, a_cnt):
    import torch
    from snake_engine._lib import check
    n, S = eng.n_slots, eng.S
    d_live = torch.as_tensor(live, device="cuda")
    pairs = torch.full((n * S, 2), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    scratch = torch.empty((eng.L.snk_pit_scratch_elems(n),), dtype=torch.int32, device="cuda")
    check(eng.L.snk_pit_rows(eng.h, d_live.data_ptr(), n, a_cnt, pairs.data_ptr(), counts.data_ptr(), scratch.data_ptr(), 0))
    torch.cuda.synchronize()
    assert np.array_equal(d_live.cpu().numpy(), live), "snk_pit_rows wrote to d_live"
    return pairs.cpu().numpy(), counts.cpu().numpy().tolist()


def _check_rows(eng, alive, live, a_cnt):
    want, nA, nB = _rows_model(alive, live, a_cnt)
    got, counts = _pit_rows(eng, live, a_cnt)
    assert counts == [nA, nB]
    assert np.array_equal(got[:nA + nB], want), f"a_cnt {a_cnt}"
    again, counts2 = _pit_rows(eng, live, a_cnt)
    assert counts2 == counts and np.array_equal(again[:nA + nB], got[:nA + nB])


def test_pit_rows_hand_made_patterns():
    # all alive; only team A (for a_cnt 2); only team B; one snake; none; a dead game between live ones (live = 0); all alive
    alive = np.array([[1, 1, 1, 1], [1, 1, 0, 0], [0, 0, 1, 1], [0, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1], [1, 0, 1, 1]], np.uint8)
    live = np.array([1, 1, 1, 1, 1, 0, 1], np.uint8)
    eng = _engine_with_alive(7, 7, 4, alive)
    for a_cnt in (0, 1, 2, 4):
        _check_rows(eng, alive, live, a_cnt)
    want, nA, nB = _rows_model(alive, live, 2)
    assert (nA, nB) == (5, 7) and not (want[:, 0] == 5).any() and want[:nA].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [6, 0]]
    _check_rows(eng, alive, np.array([0, 0, 1, 0, 0, 0, 1], np.uint8), 2)     # a live game between two dead ones
    _check_rows(eng, alive, np.zeros(7, np.uint8), 2)                         # no live game: no row


def test_pit_rows_eight_snakes_on_19x19():
    rng = np.random.RandomState(5)
    alive = (rng.rand(6, 8) < 0.6).astype(np.uint8)
    alive[0] = 1
    eng = _engine_with_alive(6, 19, 8, alive)
    _check_rows(eng, alive, np.array([1, 1, 0, 1, 1, 1], np.uint8), 3)


def test_pit_rows_5000_games_several_blocks():
    """5 000 games: five blocks of 1 024 games each contribute to both teams' scans"""
    rng = np.random.RandomState(6)
    alive = (rng.rand(5000, 4) < 0.55).astype(np.uint8)
    live = (rng.rand(5000) < 0.8).astype(np.uint8)
    eng = _engine_with_alive(5000, 7, 4, alive)
    for a_cnt in (1, 2):
        _check_rows(eng, alive, live, a_cnt)


def test_pit_rows_300000_games_carry_between_scan_passes():
    """300 000 games = 293 blocks: the single-block scan of the block sums takes two passes of 256 and carries both teams'
    totals from the first into the second (7x7 with 2 snakes, everything alive as drawn; the open flags are random)"""
    from snake_engine import Engine
    n = 300000
    eng = Engine(n, 7, 7, 2, 1, 0.15, seed=8)
    eng.reset()
    alive = np.ones((n, 2), np.uint8)
    assert np.array_equal(eng.alive().cpu().numpy(), alive)
    live = (np.random.RandomState(9).rand(n) < 0.7).astype(np.uint8)
    assert live[:256 * 1024].any() and live[256 * 1024:].any()
    _check_rows(eng, alive, live, 1)


# ---- 4. snk_pit_moves alone ------------------------------------------------------------------------------------------------------
def _pit_agent_argmax(Z):
    """pit_agent.py:15-28"""
    out = []
    for z0, z1, z2 in Z:
        if z0 > z1:
            out.append(0 if z0 > z2 else 2)
        else:
            out.append(1 if z1 > z2 else 2)
    return out


def test_pit_moves_every_branch_of_the_rule():
    import itertools
    import torch
    from snake_engine._lib import lib, check
    nan = float("nan")
    rows = [list(p) for p in itertools.permutations((0.25, -0.5, 0.75))]                     # the six strict orders
    rows += [[0.3, 0.3, 0.1], [0.3, 0.3, 0.6], [0.3, 0.1, 0.3], [0.1, 0.3, 0.3], [0.6, 0.3, 0.3], [0.3, 0.6, 0.3],
             [0.2, 0.2, 0.2], [0.0, -0.0, -0.0]]                                            # pairwise ties, all equal, signed zeros
    rows += [[nan, 0.1, 0.2], [nan, 0.2, 0.1], [0.1, nan, 0.2], [0.2, nan, 0.1], [0.1, 0.2, nan], [0.2, 0.1, nan], [nan, nan, nan]]
    rows += [[-1.0, 0.4, 0.2], [0.4, -1.0, 0.2], [0.4, 0.2, -1.0], [-1.0, -1.0, 0.3], [-1.0, 0.3, -1.0], [0.3, -1.0, -1.0],
             [-1.0, -1.0, -1.0]]                                                             # masked entries
    rng = np.random.RandomState(7)
    extra = rng.uniform(-0.9, 0.9, size=(300 - len(rows), 3)).round(1)                       # many ties at one decimal
    Z = np.concatenate([np.array(rows, np.float32), extra.astype(np.float32)])
    m, n, S = len(Z), 80, 4
    assert m == 300 and m % 256 != 0 and m < n * S
    want_rows = _pit_agent_argmax(Z.tolist())
    assert set(want_rows[:6]) == {0, 1, 2} and want_rows[14:21] == [2, 1, 2, 2, 2, 2, 2]      # a NaN loses every comparison it is in
    cells = rng.permutation(n * S)[:m]                                                       # which (game, snake) each row names
    pairs = np.stack([cells // S, cells % S], 1).astype(np.int32)
    want = np.ones((n, S), np.uint8)
    want[pairs[:, 0], pairs[:, 1]] = want_rows
    L = lib()
    d_q, d_pairs = torch.as_tensor(Z, device="cuda"), torch.as_tensor(pairs, device="cuda")
    moves = torch.full((n, S), 9, dtype=torch.uint8, device="cuda")
    check(L.snk_pit_moves(d_q.data_ptr(), d_pairs.data_ptr(), m, n, S, moves.data_ptr(), 0))
    assert np.array_equal(moves.cpu().numpy(), want)
    rest = np.setdiff1d(np.arange(n * S), cells)                                             # the snakes without a row keep 1
    assert len(rest) == n * S - m and (moves.cpu().numpy().reshape(-1)[rest] == 1).all()
    # the same answers as the pit agent's device argmax of today
    pmf, am = torch.empty_like(d_q), torch.empty((m,), dtype=torch.uint8, device="cuda")
    check(L.snk_softermax_argmax(d_q.data_ptr(), m, 2.0, pmf.data_ptr(), am.data_ptr(), 0))
    assert am.cpu().numpy().tolist() == want_rows
    # no row at all: every snake keeps 1
    check(L.snk_pit_moves(0, 0, 0, n, S, moves.data_ptr(), 0))
    assert (moves.cpu().numpy() == 1).all()


# ---- 5. snk_pit_verdict alone ----------------------------------------------------------------------------------------------------
def test_pit_verdict_every_case():
    import torch
    from snake_engine._lib import check
    #              alive          done  rewards           live   -> winner, length, live
    cases = [
        ([0, 0, 1, 0], 1, [-1, -1, 1, -1], 1, 2, 9, 0),          # done, a single +1
        ([0, 1, 0, 1], 1, [-1, 1, -1, 1], 1, 3, 9, 0),           # done, two +1: the larger id
        ([0, 0, 0, 0], 1, [-1, -1, -1, -1], 1, -1, 9, 0),        # done, none: a draw
        ([0, 0, 1, 1], 0, [-1, -1, 0, 0], 1, 2, 9, 0),           # not done, team A gone: the smallest alive id
        ([1, 1, 0, 0], 0, [0, 0, -1, -1], 1, 0, 9, 0),           # not done, team B gone
        ([0, 1, 0, 1], 0, [-1, 0, -1, 0], 1, -5, -6, 1),         # not done, both present: stays open, nothing written
        ([0, 0, 1, 0], 1, [-1, -1, 1, -1], 0, -5, -6, 0),        # closed before: untouched although done is set
        ([0, 0, 1, 1], 0, [-1, -1, 0, 0], 0, -5, -6, 0),         # closed before, one team gone: untouched
    ]
    n, S, a_cnt, turn = len(cases), 4, 2, 9
    alive = np.array([c[0] for c in cases], np.uint8)
    eng = _engine_with_alive(n, 7, S, alive)
    done = torch.as_tensor(np.array([c[1] for c in cases], np.uint8), device="cuda")
    rew = torch.as_tensor(np.array([c[2] for c in cases], np.int8), device="cuda")
    live = torch.as_tensor(np.array([c[3] for c in cases], np.uint8), device="cuda")
    winner = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    length = torch.full((n,), -6, dtype=torch.int32, device="cuda")
    before = [bytes(s) for s in eng.export()]
    check(eng.L.snk_pit_verdict(eng.h, done.data_ptr(), rew.data_ptr(), n, a_cnt, turn, live.data_ptr(), winner.data_ptr(),
                                length.data_ptr(), 0))
    assert winner.cpu().numpy().tolist() == [c[4] for c in cases]
    assert length.cpu().numpy().tolist() == [c[5] for c in cases]
    assert live.cpu().numpy().tolist() == [c[6] for c in cases]
    assert [bytes(s) for s in eng.export()] == before, "the verdict wrote to a game record"
    # a_cnt 1 and 3 on the same boards: which team a snake belongs to moves with it
    for a, want in ((1, [2, 3, -1, 2, -5, 1, -5, -5]), (3, [2, 3, -1, -5, 0, -5, -5, -5])):
        live = torch.as_tensor(np.array([1, 1, 1, 1, 1, 1, 0, 0], np.uint8), device="cuda")
        winner.fill_(-5)
        check(eng.L.snk_pit_verdict(eng.h, done.data_ptr(), rew.data_ptr(), n, a, turn, live.data_ptr(), winner.data_ptr(),
                                    length.data_ptr(), 0))
        assert winner.cpu().numpy().tolist() == want, a


# ---- 6. retired games are frozen -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_retired_games_keep_the_board_of_their_verdict(ci):
    z, p, H, W, S, hd, n, a_cnt = _meta(ci)
    _, boards = _arena_run(ci)
    winners, lengths, want = _oracle_run(ci)
    assert lengths == z[p + "lengths"].tolist() and min(lengths) < max(lengths)      # games retire at different turns
    for g in range(n):
        for k in KEYS:
            assert np.array_equal(boards[g][k], want[g][k]), f"game {g} ({lengths[g]} turns): {k}"
        assert boards[g]["counters"][5] == lengths[g]


# ---- 7. one read-back per turn -----------------------------------------------------------------------------------------------------
def _count_readbacks(monkeypatch, fn):
    import torch
    count = [0]

    def counted(orig):
        def f(self, *a, **k):
            count[0] += 1
            return orig(self, *a, **k)
        return f
    with monkeypatch.context() as mp:
        for name in ("cpu", "item", "tolist", "numpy"):
            mp.setattr(torch.Tensor, name, counted(getattr(torch.Tensor, name)))
        out = fn()
    return out, count[0]


def test_one_read_back_per_turn(monkeypatch):
    """Tensor.cpu / .item / .tolist / .numpy counted over a match between two device stub nets: the two row counts once per
    turn (and once more to see that no row is left), then the winners and the lengths (.cpu + .numpy each); the host loop
    `run` on the same boards needs several per turn"""
    import torch
    from stubnet_device import DeviceStubNNet
    from snake_engine.arena import Arena
    from utils.pit_agent import Agent
    from utils.pit_mp_game_runner import MPGameRunner
    z, p, H, W, S, hd, n, a_cnt = _meta(0)
    spawn = lambda turn: z[p + "spawn"][turn - 1]
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(_start_states(z, p, H, W, S, n))
    torch.cuda.synchronize()
    res, got = _count_readbacks(monkeypatch, lambda: arena.match(DeviceStubNNet(), DeviceStubNNet(), a_cnt, spawn_tape=spawn))
    assert res.turns > 20 and got == res.turns + 5
    gr = MPGameRunner(H, W, S, hd, n, seed=1)
    gr.engine.import_states(_start_states(z, p, H, W, S, n))
    for g in gr.games.values():
        g._dirty()
    winners, host = _count_readbacks(monkeypatch, lambda: gr.run(Agent(DeviceStubNNet()), Agent(DeviceStubNNet()), a_cnt, spawn_tape=spawn))
    assert [-1 if w is None else w for w in winners] == res.winners.tolist()           # the same match, so the same number of turns
    assert host / res.turns > (got - 5) / res.turns == 1.0


# ---- 8. two real nets --------------------------------------------------------------------------------------------------------------
def test_match_between_two_real_nets():
    from snake_engine.arena import Arena
    from snake_engine.engine import compact_from_state
    from snake_engine.net import glorot_uniform_weights
    from utils.alpha_nnet import AlphaNNet
    nets = [AlphaNNet(input_shape=(21, 21, 3), _weights=glorot_uniform_weights((21, 21, 3), 1, seed=s)) for s in (11, 12)]

    def play():
        arena = Arena(11, 11, 4, 1, 64, seed=5)
        start = [compact_from_state(s) for s in arena.engine.export()]
        return arena.match(nets[0], nets[1]), start
    trips = sum(net._qnet.guard_trips for net in nets)
    res, start = play()
    if sum(net._qnet.guard_trips for net in nets) != trips:      # a range guard widened a scale half way: play with settled scales
        res, start = play()
    assert res.turns >= 3 and (res.lengths >= 1).all() and res.lengths.max() == res.turns
    assert ((res.winners >= -1) & (res.winners < 4)).all()
    assert res.wins_a + res.wins_b + res.draws == 64
    assert res.wins_a == int(((res.winners >= 0) & (res.winners < 2)).sum())
    res2, start2 = play()
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(start, start2) for k in KEYS)
    assert np.array_equal(res2.winners, res.winners) and np.array_equal(res2.lengths, res.lengths)
