"""GPU tests of the searching pit (snake_engine.arena.Searcher, Arena.match with a Searcher on either side): whole matches
against the CPU statement of tests/search_pit_ref.py in the sequential, taped parity mode; snk_pit_roots and
snk_pit_search_moves one by one against NumPy; the greedy path as it was; the arena's one read-back per turn with a searcher;
the production mode between two real nets; MPGameRunner.run_device with a searching agent."""
import functools

import numpy as np
import pytest

import search_pit_ref as R

pytestmark = pytest.mark.gpu


# ---- 1. search parity ------------------------------------------------------------------------------------------------------------
def _sides(name, tape):
    from snake_engine.arena import Searcher
    board, n, breadth, searching, seed = R.CASES[name]
    return [Searcher(R.DeviceStub(w), breadth, 4, 100, seed=5, sequential=True, tape_u=tape) if s else R.DeviceStub(w)
            for w, s in zip((0, 1), searching)]


@pytest.mark.parametrize("name", list(R.CASES))
def test_match_with_searchers_replays_the_cpu_statement(name):
    """the helper plays first (spawn draws from a seeded RandomState, spawned cells logged); Arena.match replays on the same start
    boards with that log as its spawn tape and the same uniform tape: winners, lengths, turns, every searcher's draws consumed
    and the boards at the verdicts are exact"""
    from snake_engine.arena import Arena, Searcher
    from snake_engine.engine import compact_from_state
    board, n, breadth, searching, seed = R.CASES[name]
    want = R.reference(name)
    R.check_well_posed(want)
    H, W, S, hd = want["geometry"]
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(R.start_states(board, n))
    sides = _sides(name, R.uniform_tape(seed))
    log = want["spawn_log"]
    res = arena.match(sides[0], sides[1], 1, spawn_tape=lambda turn: np.maximum(log[turn - 1], -1))
    assert res.winners.tolist() == [-1 if w is None else w for w in want["winners"]]
    assert res.lengths.tolist() == want["lengths"]
    assert res.turns == want["turns"]
    for side, pos in zip(sides, want["tape_pos"]):
        assert isinstance(side, Searcher) == (pos is not None)
        if pos is not None:
            assert side.tape_pos == pos, "draws consumed"
    got = [compact_from_state(s) for s in arena.engine.export()]
    for g in range(n):
        ref = want["games"][g].compact()
        for k in R.KEYS:
            assert np.array_equal(got[g][k], ref[k]), f"game {g} ({want['lengths'][g]} turns): {k}"


# ---- 2. snk_pit_roots against NumPy ----------------------------------------------------------------------------------------------
# (games, snakes): one block and its edges, several blocks, and 300 000 games = 293 blocks, for which the single-block scan of
# the block sums takes two passes of 256 and carries the first pass's total into the second
SIZES = [(n, S) for n in (1, 63, 64, 65, 257, 5000) for S in (2, 4, 8)] + [(300000, 2)]


@functools.lru_cache(maxsize=None)
def _played_engine(n, S):
    """n games some ticks into random play, so that dead snakes exist -> (engine, alive uint8[n][S])"""
    import torch
    from snake_engine import Engine
    eng = Engine(n, 7, 7, S, 1, 0.15, seed=40 + S)
    eng.reset()
    g = torch.Generator(device="cuda").manual_seed(n)
    for _ in range(6):
        eng.step(torch.randint(0, 3, (n, S), dtype=torch.uint8, device="cuda", generator=g))
    alive = eng.alive().cpu().numpy()
    assert n < 63 or (0 < alive.mean() < 1)
    return eng, alive


def _live_patterns(n):
    one = np.zeros(n, np.uint8); one[n // 3] = 1
    last = np.zeros(n, np.uint8); last[-1] = 1
    return {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8), "alternating": (np.arange(n) % 2).astype(np.uint8),
            "one": one, "last only": last, "random": (np.random.RandomState(n).rand(n) < 0.7).astype(np.uint8)}


def _pit_roots(eng, live):
    import torch
    from snake_engine._lib import check
    n, S = eng.n_slots, eng.S
    d_live = torch.as_tensor(live, device="cuda")
    slots = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    alive = torch.full((n, S), 9, dtype=torch.uint8, device="cuda")
    rank = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    scratch = torch.empty((eng.L.snk_pit_scratch_elems(n),), dtype=torch.int32, device="cuda")
    check(eng.L.snk_pit_roots(eng.h, d_live.data_ptr(), n, slots.data_ptr(), alive.data_ptr(), rank.data_ptr(), count.data_ptr(),
                              scratch.data_ptr(), 0))
    torch.cuda.synchronize()
    assert np.array_equal(d_live.cpu().numpy(), live), "snk_pit_roots wrote to d_live"
    return slots, alive, rank, int(count.item())


@pytest.mark.parametrize("n,S", SIZES)
def test_pit_roots_against_numpy(n, S):
    eng, alive = _played_engine(n, S)
    for tag, live in _live_patterns(n).items():
        slots, d_alive, rank, G = _pit_roots(eng, live)
        want = np.flatnonzero(live).astype(np.int32)
        assert G == len(want), tag
        slots, d_alive, rank = slots.cpu().numpy(), d_alive.cpu().numpy(), rank.cpu().numpy()
        assert np.array_equal(slots[:G], want), tag
        assert np.array_equal(d_alive[:G], alive[want]), tag
        assert (slots[G:] == -7).all() and (d_alive[G:] == 9).all(), f"{tag}: written behind G"
        want_rank = np.full(n, -1, np.int32)
        want_rank[want] = np.arange(G)
        assert np.array_equal(rank, want_rank), tag
    if n == 300000:
        live = _live_patterns(n)["random"]
        assert live[:256 * 1024].any() and live[256 * 1024:].any()


def test_pit_roots_no_game_is_a_no_op():
    import torch
    from snake_engine._lib import check
    eng, _ = _played_engine(1, 4)
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    check(eng.L.snk_pit_roots(eng.h, 0, 0, 0, 0, 0, count.data_ptr(), 0, 0))
    assert int(count.item()) == 0
    assert eng.L.snk_pit_roots(eng.h, 0, 2, 0, 0, 0, count.data_ptr(), 0, 0) < 0           # more games than slots


# ---- 3. snk_pit_search_moves against NumPy ---------------------------------------------------------------------------------------
def _merge_model(ma, mb, rank, alive, n, S, a_cnt, keep_other, before):
    out = before.copy()
    for s in range(S):
        src = ma if s < a_cnt else mb
        j = rank
        is_open = j >= 0
        jj = np.where(is_open, j, 0)
        al = is_open & (alive[jj, s] != 0)
        col = np.ones(n, np.uint8)
        if src is not None:
            col = np.where(al, src[jj, s], 1).astype(np.uint8)
        elif keep_other:
            col = np.where(al, before[:, s], 1).astype(np.uint8)
        out[:, s] = col
    return out


@pytest.mark.parametrize("n,S", SIZES)
def test_pit_search_moves_against_numpy(n, S):
    import torch
    from snake_engine._lib import check
    eng, alive_all = _played_engine(n, S)
    L = eng.L
    rng = np.random.RandomState(n + S)
    live = _live_patterns(n)["random" if n > 1 else "all"]
    slots, d_alive, d_rank, G = _pit_roots(eng, live)
    rank, alive = d_rank.cpu().numpy(), d_alive.cpu().numpy()
    assert (rank < 0).any() or n == 1                                              # closed games
    ma, mb = (rng.randint(0, 3, size=(max(G, 1), S)).astype(np.uint8) for _ in range(2))
    d_ma, d_mb = torch.as_tensor(ma, device="cuda"), torch.as_tensor(mb, device="cuda")
    # what snk_pit_moves leaves for a greedy team: 1 everywhere, the rows' greedy moves on top
    gi, si = np.nonzero(alive_all.astype(bool) & live.astype(bool)[:, None])
    pairs = torch.as_tensor(np.stack([gi, si], 1).astype(np.int32), device="cuda")
    q = torch.as_tensor(rng.uniform(-0.9, 0.9, size=(len(gi), 3)).astype(np.float32), device="cuda")
    greedy = torch.empty((n, S), dtype=torch.uint8, device="cuda")
    check(L.snk_pit_moves(q.data_ptr(), pairs.data_ptr(), len(gi), n, S, greedy.data_ptr(), 0))
    greedy_h = greedy.cpu().numpy()
    assert n < 63 or len(np.unique(greedy_h)) == 3
    for a_cnt in (0, 1, S):
        for tag, pa, pb, keep, before in (("both", d_ma, d_mb, 0, None), ("A only, keep", d_ma, None, 1, greedy_h),
                                          ("B only, keep", None, d_mb, 1, greedy_h), ("B only", None, d_mb, 0, None),
                                          ("A only", d_ma, None, 0, None)):
            before = np.full((n, S), 9, np.uint8) if before is None else before
            moves = torch.as_tensor(before, device="cuda")
            check(L.snk_pit_search_moves(0 if pa is None else pa.data_ptr(), 0 if pb is None else pb.data_ptr(), d_rank.data_ptr(),
                                         d_alive.data_ptr(), n, S, a_cnt, keep, moves.data_ptr(), 0))
            want = _merge_model(None if pa is None else ma, None if pb is None else mb, rank, alive, n, S, a_cnt, keep, before)
            assert np.array_equal(moves.cpu().numpy(), want), f"{tag}, a_cnt {a_cnt}"
            assert (want != 9).all()                                               # every cell has a writer or keeps a greedy move
    dead = (rank >= 0)[:, None] & (alive[np.maximum(rank, 0)] == 0)
    assert n < 63 or dead.any()                                                    # dead snakes of open games were among the cells


# ---- 4. the greedy path is untouched ---------------------------------------------------------------------------------------------
def _count(monkeypatch, names, fn, only_file=None):
    import sys
    import torch
    count = [0]

    def counted(orig):
        def f(self, *a, **k):
            if only_file is None or sys._getframe(1).f_code.co_filename.endswith(only_file):
                count[0] += 1
            return orig(self, *a, **k)
        return f
    with monkeypatch.context() as mp:
        for name in names:
            mp.setattr(torch.Tensor, name, counted(getattr(torch.Tensor, name)))
        out = fn()
    return out, count[0]


def _recorded_pit():
    from conftest import load_golden
    from snake_engine.engine import state_from_compact
    z = load_golden("pit.npz")
    H, W, S, hd, n, a_cnt = (int(v) for v in z["p0_meta"])
    states = [state_from_compact(H, W, S, {k: z["p0_init_" + k][g] for k in R.KEYS}) for g in range(n)]
    return z, (H, W, S, hd, n, a_cnt), states


def test_match_between_two_nets_is_as_before(monkeypatch):
    """one read-back per turn (Tensor.cpu / .item / .tolist / .numpy counted: the two row counts once per turn and once more to
    see that no row is left, then the winners and the lengths), and the recorded winners of recorded pit 0"""
    import torch
    from snake_engine.arena import Arena
    z, (H, W, S, hd, n, a_cnt), states = _recorded_pit()
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(states)
    torch.cuda.synchronize()
    res, got = _count(monkeypatch, ("cpu", "item", "tolist", "numpy"),
                      lambda: arena.match(R.DeviceStub(0), R.DeviceStub(1), a_cnt, spawn_tape=lambda turn: z["p0_spawn"][turn - 1]))
    assert res.winners.tolist() == z["p0_winners"].tolist() and res.lengths.tolist() == z["p0_lengths"].tolist()
    assert res.turns > 20 and got == res.turns + 5
    assert arena._roots is None                            # the searching turn's buffers were never made


# ---- 5. the arena's read-back with a searcher ------------------------------------------------------------------------------------
@pytest.mark.parametrize("searching", [(True, True), (True, False), (False, True)])
def test_arena_reads_back_once_per_turn_with_a_searcher(monkeypatch, searching):
    """.tolist() calls made in arena.py, with Searcher.search replaced by a stub that returns all-straight moves without
    synchronising: one per turn and one more that sees G = 0"""
    import torch
    from snake_engine import arena as A
    z, (H, W, S, hd, n, a_cnt), states = _recorded_pit()
    arena = A.Arena(H, W, S, hd, n, seed=1)
    arena.import_states(states)
    calls = []

    def straight(self, engine, slots, alive):
        calls.append(int(slots.shape[0]))
        assert alive.shape == (slots.shape[0], S) and slots.dtype == torch.int32 and alive.dtype == torch.uint8
        return torch.ones((slots.shape[0], S), dtype=torch.uint8, device=slots.device)
    monkeypatch.setattr(A.Searcher, "search", straight)
    sides = [A.Searcher(R.DeviceStub(w), 8, 4) if s else R.DeviceStub(w) for w, s in zip((0, 1), searching)]
    res, got = _count(monkeypatch, ("tolist",), lambda: arena.match(sides[0], sides[1], a_cnt), only_file="arena.py")
    assert res.turns >= 3 and got == res.turns + 1
    assert len(calls) == res.turns * sum(searching)
    assert calls[0] == n and min(calls) < n and sorted(calls, reverse=True) == calls        # G shrinks as games close
    assert res.lengths.max() == res.turns and res.wins_a + res.wins_b + res.draws == n


# ---- 6. production mode ----------------------------------------------------------------------------------------------------------
def test_production_mode_match_between_two_real_nets():
    """Philox draws, float atomics in the back-ups: structural invariants only.  Whether two runs with the same seeds were
    identical is printed, not asserted (production-mode back-ups are not pinned run to run)"""
    from snake_engine.arena import Arena, Searcher
    from snake_engine.net import glorot_uniform_weights
    from utils.alpha_nnet import AlphaNNet
    nets = [AlphaNNet(input_shape=(21, 21, 3), _weights=glorot_uniform_weights((21, 21, 3), 1, seed=s)) for s in (11, 12)]

    def play():
        arena = Arena(11, 11, 4, 1, 32, seed=5)
        sides = [Searcher(net, 8, 8, seed=21 + k) for k, net in enumerate(nets)]
        res = arena.match(sides[0], sides[1])
        assert all(s.stats["net_evals"] > 0 and s.stats["rollout_ticks"] >= res.turns for s in sides)
        return res
    runs = [play(), play()]
    for res in runs:
        assert res.turns >= 3 and (res.lengths >= 1).all() and res.lengths.max() == res.turns
        assert ((res.winners >= -1) & (res.winners < 4)).all()
        assert res.wins_a + res.wins_b + res.draws == 32
        assert res.wins_a == int(((res.winners >= 0) & (res.winners < 2)).sum())
    same = np.array_equal(runs[0].winners, runs[1].winners) and np.array_equal(runs[0].lengths, runs[1].lengths)
    print(f"\nproduction-mode search v search, 32 games, breadth 8, same seeds twice: identical = {same}; "
          f"turns {runs[0].turns} / {runs[1].turns}, wins {runs[0].wins_a}-{runs[0].wins_b} / {runs[1].wins_a}-{runs[1].wins_b}")


# ---- 7. run_device with a searching agent ----------------------------------------------------------------------------------------
def test_run_device_with_a_searching_agent_equals_the_match_with_its_searcher():
    from snake_engine.arena import Arena, Searcher
    from utils.agent import Agent
    from utils.pit_agent import Agent as PitAgent
    from utils.pit_mp_game_runner import MPGameRunner
    name = "7x7x2-b8-search-v-greedy"
    board, n, breadth, searching, seed = R.CASES[name]
    want = R.reference(name)
    H, W, S, hd = want["geometry"]
    tape, log = R.uniform_tape(seed), want["spawn_log"]
    spawn = lambda turn: np.maximum(log[turn - 1], -1)
    arena = Arena(H, W, S, hd, n, seed=1)
    arena.import_states(R.start_states(board, n))
    res = arena.match(Searcher(R.DeviceStub(0), breadth, 4, 100, seed=5, sequential=True, tape_u=tape), R.DeviceStub(1), 1, spawn_tape=spawn)
    gr = MPGameRunner(H, W, S, hd, n, seed=1)
    gr.engine.import_states(R.start_states(board, n))
    for g in gr.games.values():
        g._dirty()
    alice = Agent(R.DeviceStub(0), 100, False, 4, breadth, seed=5, sequential=True, tape_u=tape)
    got = gr.run_device(alice, PitAgent(R.DeviceStub(1)), 1, spawn_tape=spawn)
    assert got == [None if w < 0 else w for w in res.winners.tolist()] == want["winners"]
    assert gr.arena_result.lengths.tolist() == res.lengths.tolist() and gr.arena_result.turns == res.turns
    assert len(gr.games) == 0
