"""Test infrastructure: the CPU statement of the lookahead opponent (snake_engine.arena.Lookahead, snk_pit_look_values) in plain
Python over the compact boards of tests/script_ref.py, and a match player built on it.

The policy (include/snake_engine.h), for snake s of a board with A snakes alive (ids ascending, k = 0 .. A-1):

    fallback  A < 2 or A > 4: the plain scores of script_ref.scores
    children  child j < 3^A: Game.subgame of the board as oracle.snake_oracle makes it (no food spawning), one tic in which the
              k-th alive snake makes relative move (j // 3^k) % 3 and every dead snake's entry is 1
    leaf      of s in child c: dead -- s is not alive in c; WIN = 2^24 -- s alone is alive; else max(script_ref.scores(c, s))
    score     of own move a, over the children whose digit of s is a: min(leaf) when s lives in all of them, else
              -2 - (the number of them in which s is dead)

The move is script_ref.move of the three scores.  Nothing here is shared with the kernels: the children come from the C game of
oracle/, the leaves from the queue flood fill of script_ref."""
import functools

import numpy as np

import league_ref as LR
import script_ref as R
import search_pit_ref as SR
from conftest import golden_state, load_golden
from oracle import snake_oracle
from oracle.mcts_oracle import argmaxs

WIN = 1 << 24
LOW, HIGH = -29, WIN                                # every value lies inside


def fanout(S):
    return 3 ** min(S, 4)


def child_boards(H, W, S, health_dec, st):
    """the 3^A stepped children of a compact board with A = 2..4 snakes alive, as compact boards, and the alive ids"""
    alive = [s for s in range(S) if st["alive"][s]]
    assert 2 <= len(alive) <= 4
    root = snake_oracle.Game.from_compact(H, W, S, health_dec, 0.15, st)
    out = []
    for j in range(3 ** len(alive)):
        c = root.subgame()
        moves = np.ones(S, np.uint8)
        for k, s in enumerate(alive):
            moves[s] = (j // 3 ** k) % 3
        c.tic(moves)
        assert c.last_spawn == -1                   # a sub-game spawns no food
        out.append(c.compact())
    return out, alive


def leaves(H, W, S, health_dec, st, flags=R.ALL):
    """[child j] -> {s: leaf value} over the snakes alive in child j (a snake that died there has no entry), and the alive ids"""
    children, alive = child_boards(H, W, S, health_dec, st)
    out = []
    for c in children:
        left = [s for s in alive if c["alive"][s]]
        plain = R.board_scores(H, W, c, flags) if len(left) >= 2 else {}
        out.append({s: WIN if len(left) == 1 else max(plain[s]) for s in left})
    return out, alive


def board_look_scores(H, W, S, health_dec, st, flags=R.ALL):
    """{s: the three lookahead scores} of every alive snake of a compact board"""
    A = int(np.count_nonzero(st["alive"][:S]))
    if A < 2 or A > 4:
        return R.board_scores(H, W, st, flags)
    leaf, alive = leaves(H, W, S, health_dec, st, flags)
    out = {}
    for k, s in enumerate(alive):
        q = []
        for a in range(3):
            mine = [lf for j, lf in enumerate(leaf) if (j // 3 ** k) % 3 == a]
            assert len(mine) == 3 ** (len(alive) - 1)
            dead = sum(s not in lf for lf in mine)
            q.append(-2 - dead if dead else min(lf[s] for lf in mine))
        out[s] = q
    return out


def look_scores(H, W, S, health_dec, st, s, flags=R.ALL):
    """the three lookahead scores of snake s; [-1, -1, -1] for a dead or absent snake"""
    if not 0 <= s < S or not st["alive"][s]:
        return [-1, -1, -1]
    return board_look_scores(H, W, S, health_dec, st, flags)[s]


class RefLookahead(R.RefScripted):
    """the statement's side of a match: what snake_engine.arena.Lookahead(flags) is on the device"""


# ---- the match player -------------------------------------------------------------------------------------------------------------
def look_run(games, sides, owner, spawn_seed):
    """script_ref.script_run without searching owners and with RefLookahead among the sides: sides[o] is a RefLookahead, a
    RefScripted or a net with .v.  Returns what script_run returns, and reads [turn - 1] = the turn's K row counts"""
    S, K = games[0].g.S, len(sides)
    H, W, hd = games[0].g.H, games[0].g.W, games[0].g.health_dec
    owner = np.asarray(owner)
    assert owner.shape == (len(games), S) and owner.min() >= 0 and owner.max() < K
    rng = np.random.RandomState(spawn_seed)
    winners, lengths = [None] * len(games), [0] * len(games)
    live = list(range(len(games)))
    counts, spawn_log, turn = [], [], 0
    while live:
        turn += 1
        dense = {g: np.ones(S, np.uint8) for g in live}
        rows_of = []
        for o in range(K):
            ids = [(g, s) for g in live for s in games[g].alive_ids() if owner[g][s] == o]
            rows_of.append(len(ids))
            if isinstance(sides[o], R.RefScripted):
                look = isinstance(sides[o], RefLookahead)
                for g in sorted({g for g, _ in ids}):
                    st = games[g].compact()
                    q = board_look_scores(H, W, S, hd, st, sides[o].flags) if look else R.board_scores(H, W, st, sides[o].flags)
                    for s in (s for gg, s in ids if gg == g):
                        dense[g][s] = R.move(q[s])
            elif ids:
                for (g, s), m in zip(ids, argmaxs(sides[o].v([games[g].make_state(s) for g, s in ids]))):
                    dense[g][s] = m
        counts.append(rows_of)
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
            else:                                                           # :48-60 with a team read as an owner
                ids = games[g].alive_ids()
                if len({int(owner[g][s]) for s in ids}) <= 1:
                    winners[g] = ids[0] if ids else None
                else:
                    nxt.append(g)
        live = nxt
    return dict(winners=winners, winner_owner=[None if w is None else int(owner[g][w]) for g, w in enumerate(winners)],
                lengths=lengths, turns=turn, counts=counts, spawn_log=spawn_log, boards=[g.compact() for g in games])


# ---- what the tests share: sampled golden boards and the matches of the GPU test ---------------------------------------------------
STRIDE = {"7x7x2": 3, "9x9x3": 4, "11x11x4": 40, "15x15x5": 4, "19x19x8": 16}


@functools.lru_cache(maxsize=None)
def sampled(cfg):
    """(H, W, S, health_dec, boards): every STRIDE[cfg]-th board of the golden trajectories tic_<cfg>.npz"""
    z = load_golden(f"tic_{cfg}.npz")
    H, W, S, hd = (int(z[k]) for k in ("H", "W", "S", "health_dec"))
    return H, W, S, hd, [golden_state(z, i) for i in range(0, z["st_alive"].shape[0], STRIDE[cfg])]


@functools.lru_cache(maxsize=None)
def sampled_scores(cfg, flags=R.ALL):
    """[board] -> {s: the three scores}: the statement over sampled(cfg), computed once and shared (callers must not change it)"""
    H, W, S, hd, boards = sampled(cfg)
    return [board_look_scores(H, W, S, hd, st, flags) for st in boards]


SPAWN_SEED = 43
N_DUEL, N_FOUR, N_LEAGUE = 16, 12, 12


@functools.lru_cache(maxsize=None)
def reference(name):
    """the statement's run of one of the matches, computed once and shared (callers must not change it)"""
    if name == "duel-7x7x2":                      # Lookahead() against Scripted(), one snake each, sixteen recorded start boards
        games, geo = SR.start_games("7x7x2", N_DUEL)
        out = look_run(games, [RefLookahead(), R.RefScripted()], LR.two_team_table(N_DUEL, 2, 1), SPAWN_SEED)
    elif name == "1v3-11x11x4":                   # one Lookahead() against three snakes of Scripted()
        games, geo = SR.start_games("11x11x4", N_FOUR)
        out = look_run(games, [RefLookahead(), R.RefScripted()], LR.two_team_table(N_FOUR, 4, 1), SPAWN_SEED)
    else:                                         # a lookahead owner, a scripted owner and stub net 0
        assert name == "league-11x11x4"
        games, geo = SR.start_games("11x11x4", N_LEAGUE)
        out = look_run(games, [RefLookahead(), R.RefScripted(R.SPACE), LR.RefStub(0)], R.three_owner_table(N_LEAGUE), SPAWN_SEED)
    out["geometry"] = geo
    return out
