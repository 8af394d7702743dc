"""Test infrastructure: the CPU statement of a league match in which any owner may move by search, written from
tests/search_pit_ref.py::search_pit_run (a searching team) and tests/league_ref.py::league_run (an owner per seat), and NumPy
models of the two kernels behind League.play_search (snk_pit_roots_owned, snk_pit_search_moves_owned).

A searching owner is one oracle.mcts_oracle.SelfPlayOracle(net, base, training=False, depth, breadth, draws=CheckedDraws(tape_o))
kept over the match.  Each turn its root_turn runs over the open games in which the owner HOLDS A SEAT (an alive snake on a seat
of the owner), in game order; it simulates all snakes of those games with the owner's net and the owner's own seats take the
moves (Agent.make_moves, agent.py:25-99).  An owner without such a game is skipped: the verdict closes a game for good, so it can
never have one again and its caches are never read again.  Greedy owners, the food draws and the verdict are league_run's.

q_gap and u_edge are search_pit_ref's: the smallest gap between the two largest Q at a root decision a searching owner took, and
the smallest distance of a rollout uniform from an edge of its cdf.  CASES lists what the GPU test plays; the seeds were chosen
on the CPU so that every case is well posed and meets check_conditions."""
import functools

import numpy as np

import league_ref as LR
import search_pit_ref as SR
from oracle.mcts_oracle import SelfPlayOracle, argmaxs

KEYS = SR.KEYS


def league_search_run(games, nets, searching, owner, spawn_seed, tapes=None, depth=4, breadth=8, base=100):
    """games: oracle Games (index = game id); nets: K objects with .v; searching[o]: owner o moves by search; owner[g][s] in
    0..K-1; food from RandomState(spawn_seed) as in league_run; tapes[o]: owner o's uniform tape.  Returns a dict: winners (None
    for a draw), winner_owner, lengths, turns, counts [turn - 1] = the greedy owners' row counts in owner order followed by the K
    counts of games per owner (0 for a greedy owner: what League.play_search reads back), spawn_log, branch, boards, games,
    tape_pos [o] (None for a greedy owner), q_gap, u_edge, and lists [turn - 1][o] = the game ids owner o searched"""
    S, K = games[0].g.S, len(nets)
    owner = np.asarray(owner)
    assert owner.shape == (len(games), S) and owner.min() >= 0 and owner.max() < K
    rng = np.random.RandomState(spawn_seed)
    oracles = [SelfPlayOracle(net, base, False, depth, breadth, draws=SR.CheckedDraws(None if tapes is None else tapes[o])) if s else None
               for o, (net, s) in enumerate(zip(nets, searching))]
    winners, lengths, branch = [None] * len(games), [0] * len(games), [None] * len(games)
    live = list(range(len(games)))
    counts, lists, spawn_log, q_gap, turn = [], [], [], np.inf, 0
    while live:
        turn += 1
        dense = {g: np.ones(S, np.uint8) for g in live}
        rows_of, games_of = [], [0] * K
        lists.append([[] for _ in range(K)])
        for o in range(K):
            if oracles[o] is None:                                          # pit_agent.py:10-13 on the owner's own rows
                ids = [(g, s) for g in live for s in games[g].alive_ids() if owner[g][s] == o]
                rows_of.append(len(ids))
                states = [games[g].make_state(s) for g, s in ids]
                for (g, s), m in zip(ids, argmaxs(nets[o].v(states)) if states else []):
                    dense[g][s] = m
                continue
            mine = [g for g in live if any(owner[g][s] == o for s in games[g].alive_ids())]
            games_of[o] = len(mine)
            lists[-1][o] = mine
            if not mine:
                continue
            rows, V, moves = oracles[o].root_turn([games[g] for g in mine])
            for (gi, s), v, m in zip(rows, V, moves):
                if owner[mine[gi]][s] == o:
                    dense[mine[gi]][s] = m
                    top = np.sort(np.asarray(v, np.float64))
                    q_gap = min(q_gap, float(top[2] - top[1]))
        counts.append(rows_of + games_of)
        spawn_log.append(np.full(len(games), -2, np.int16))
        nxt = []
        for g in live:
            done = games[g].tic(dense[g], draws=(rng.random_sample(), rng.random_sample()))
            spawn_log[-1][g] = games[g].last_spawn
            lengths[g] += 1
            if done:                                                        # pit_mp_game_runner.py:43-47
                for i, r in enumerate(games[g].rewards):
                    if r == 1.0:
                        winners[g] = i
                branch[g] = "done, winner" if winners[g] is not None else "done, draw"
            else:                                                           # :48-60 with a team read as an owner
                ids = games[g].alive_ids()
                if len({int(owner[g][s]) for s in ids}) <= 1:
                    winners[g] = ids[0] if ids else None
                    branch[g] = "one owner left"
                else:
                    nxt.append(g)
        live = nxt
    return dict(winners=winners, winner_owner=[None if w is None else int(owner[g][w]) for g, w in enumerate(winners)],
                lengths=lengths, turns=turn, counts=counts, lists=lists, spawn_log=spawn_log, branch=branch, games=games,
                boards=[g.compact() for g in games], tape_pos=[None if o is None else o.draw.pos for o in oracles], q_gap=q_gap,
                u_edge=min([o.draw.u_edge for o in oracles if o is not None], default=np.inf))


# ---- the matches of the GPU test ---------------------------------------------------------------------------------------------
def duel_table():
    """schedule(3, 1, "duel"): the six ordered pairs of three owners, one 7x7x2 board each"""
    return np.array([[i, j] for i in range(3) for j in range(3) if i != j], np.uint8)


def four_table():
    """five 11x11x4 boards: two 1 v 3 line-ups, two four-owner line-ups, and two owners with two seats each"""
    return np.array([[0, 1, 1, 1], [0, 1, 2, 3], [2, 3, 3, 3], [3, 2, 1, 0], [1, 0, 0, 1]], np.uint8)


TABLES = {"7x7x2": duel_table, "11x11x4": four_table}

# name: (start boards, breadth, which owners search, seed).  Depth 4; owner o's net is stub number o (league_ref.RefStub), its
# uniform tape RandomState(seed + o), the food spawns RandomState(seed + 1000)
CASES = {
    "7x7x2-b8-sss": ("7x7x2", 8, (True, True, True), 11),
    "7x7x2-b16-sgs": ("7x7x2", 16, (True, False, True), 0),
    "7x7x2-b8-gsg": ("7x7x2", 8, (False, True, False), 0),
    "11x11x4-b8-ssss": ("11x11x4", 8, (True, True, True, True), 15),
    "11x11x4-b16-sgsg": ("11x11x4", 16, (True, False, True, False), 3),
    "11x11x4-b8-gssg": ("11x11x4", 8, (False, True, True, False), 1),
}


def tapes(seed, K):
    return [np.random.RandomState(seed + o).random_sample(SR.TAPE_LEN) for o in range(K)]


def run_case(board, breadth, searching, seed):
    table = TABLES[board]()
    games, geo = SR.start_games(board, len(table))
    K = len(searching)
    out = league_search_run(games, [LR.RefStub(o) for o in range(K)], searching, table, seed + 1000, tapes(seed, K), 4, breadth)
    out["geometry"] = geo
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the statement's run of CASES[name], computed once and shared (callers must not change it)"""
    return run_case(*CASES[name])


def check_well_posed(out):
    assert out["q_gap"] > SR.Q_GAP, f"a root decision hangs on {out['q_gap']:.3e}"
    assert out["u_edge"] > SR.U_EDGE, f"a rollout uniform lies {out['u_edge']:.3e} from a cdf edge"
    assert max(p or 0 for p in out["tape_pos"]) <= SR.TAPE_LEN


def conditions(out, searching, owner):
    """which of the four things a case must contain so that it cannot hide the sub-list logic it does contain"""
    owner = np.asarray(owner)
    n = len(owner)
    n_open = [int((row >= -1).sum()) for row in out["spawn_log"]]           # games open at the start of each turn
    subset = any(0 < len(lst[o]) < n_open[t] for t, lst in enumerate(out["lists"]) for o, s in enumerate(searching) if s)
    no_game = any(not lst[o] for lst in out["lists"] for o, s in enumerate(searching) if s)
    two_seats = any(s and (owner[g] == o).sum() > 1 for g in range(n) for o, s in enumerate(searching))
    one_left = any(out["branch"][g] == "one owner left" and any(searching[o] for o in set(owner[g].tolist())) for g in range(n))
    return dict(subset=subset, no_game=no_game, two_seats=two_seats, one_left=one_left)


def check_conditions(name, out):
    """every case: a turn in which a searching owner's list is a proper, non-empty subset of the open games, and a turn in which a
    searching owner has no game while the match goes on.  Every four-seat case also: a game in which a searching owner holds more
    than one seat, and a game closed by "one owner left" with a searcher seated.  (A duel of schedule(3, 1, "duel") cannot have
    either: its two seats belong to two owners, and a game of two snakes is done as soon as one is left.)"""
    board, _, searching, _ = CASES[name]
    got = conditions(out, searching, TABLES[board]())
    want = ("subset", "no_game") + (("two_seats", "one_left") if board == "11x11x4" else ())
    assert all(got[k] for k in want), (name, got)


# ---- NumPy models of the two kernels -------------------------------------------------------------------------------------------
def roots_owned_model(alive, live, owner, K, mask):
    """snk_pit_roots_owned -> (counts [K], slots int32[total], alive rows uint8[total][S], rank int32[n][S]); None for the three
    arrays when the call is a no-op (no game, or no owner below K in the mask)"""
    n, S = alive.shape
    mask &= (1 << K) - 1
    if n == 0 or mask == 0:
        return [0] * K, None, None, None
    seat = alive.astype(bool) & live.astype(bool)[:, None] & (owner < K)
    rank = np.full((n, S), -1, np.int32)
    counts, slots = [], []
    base = 0
    for o in range(K):
        mine = seat & (owner == o) if (mask >> o) & 1 else np.zeros_like(seat)
        g = np.flatnonzero(mine.any(1))
        pos = np.full(n, -1, np.int64)
        pos[g] = base + np.arange(len(g))
        rank[mine] = np.broadcast_to(pos[:, None], (n, S))[mine]
        counts.append(len(g))
        slots.append(g)
        base += len(g)
    slots = np.concatenate(slots).astype(np.int32)
    return counts, slots, alive[slots].astype(np.uint8), rank


def search_moves_owned_model(found, rank, total, keep_other, before):
    """snk_pit_search_moves_owned on a copy of the move array"""
    n, S = rank.shape
    hit = (rank >= 0) & (rank < total)
    out = before.copy() if keep_other else np.ones((n, S), np.uint8)
    cols = np.broadcast_to(np.arange(S)[None, :], (n, S))
    out[hit] = found[rank[hit], cols[hit]]
    return out
