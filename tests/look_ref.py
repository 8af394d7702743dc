"""Test infrastructure: the CPU statement of the lookahead opponent (snake_engine.arena.Lookahead, snk_pit_look_values) in plain
Python over the compact boards of tests/script_ref.py, whose match player (script_ref.run) plays it.

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


def leaves(H, W, S, health_dec, st, flags=R.ALL, score=R.board_scores, only=None):
    """[child j] -> {s: leaf value} over the snakes (only: of those ids) alive in child j (a snake that died there has no entry),
    and the alive ids"""
    children, alive = child_boards(H, W, S, health_dec, st)
    out = []
    for c in children:
        left = [s for s in alive if c["alive"][s]]
        mine = [s for s in left if only is None or s in only]
        plain = score(H, W, c, flags, mine) if len(left) >= 2 and mine else {}
        out.append({s: WIN if len(left) == 1 else max(plain[s]) for s in mine})
    return out, alive


def fold(leaf, alive, only=None, punished=-2):
    """{s: the three scores} (only: of those ids) from [child j] -> {s: leaf value}; a move that can be punished scores
    `punished` less the number of children in which s is dead"""
    out = {}
    for k, s in enumerate(alive):
        if only is not None and s not in only:
            continue
        q = []
        for a in range(3):
            mine = [lf for j, lf in enumerate(leaf) if (j // 3 ** k) % 3 == a]
            assert len(mine) == 3 ** (len(alive) - 1)
            dead = sum(s not in lf for lf in mine)
            q.append(punished - dead if dead else min(lf[s] for lf in mine))
        out[s] = q
    return out


def board_look_scores(H, W, S, health_dec, st, flags=R.ALL, score=R.board_scores, only=None):
    """{s: the three lookahead scores} of the alive snakes of a compact board (only: of those ids), the rows of the children and
    of a fallback board scored by the row-scoring function `score` (script_ref.board_scores, or leaf_ref.scorer of a leaf)"""
    A = int(np.count_nonzero(st["alive"][:S]))
    if A < 2 or A > 4:
        return score(H, W, st, flags, only)
    leaf, alive = leaves(H, W, S, health_dec, st, flags, score, only)
    return fold(leaf, alive, only)


def look_scores(H, W, S, health_dec, st, s, flags=R.ALL):
    """the three lookahead scores of snake s; [-1, -1, -1] for a dead or absent snake"""
    if not 0 <= s < S or not st["alive"][s]:
        return [-1, -1, -1]
    return board_look_scores(H, W, S, health_dec, st, flags)[s]


class RefLookahead(R.RefScripted):
    """the statement's side of a match: what snake_engine.arena.Lookahead(flags, leaf) is on the device"""

    def __init__(self, flags=R.ALL, leaf=None):
        super().__init__(flags)
        self.leaf = leaf


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
        out = R.run(games, [RefLookahead(), R.RefScripted()], LR.two_team_table(N_DUEL, 2, 1), SPAWN_SEED)
    elif name == "1v3-11x11x4":                   # one Lookahead() against three snakes of Scripted()
        games, geo = SR.start_games("11x11x4", N_FOUR)
        out = R.run(games, [RefLookahead(), R.RefScripted()], LR.two_team_table(N_FOUR, 4, 1), SPAWN_SEED)
    else:                                         # a lookahead owner, a scripted owner and stub net 0
        assert name == "league-11x11x4"
        games, geo = SR.start_games("11x11x4", N_LEAGUE)
        out = R.run(games, [RefLookahead(), R.RefScripted(R.SPACE), LR.RefStub(0)], R.three_owner_table(N_LEAGUE), SPAWN_SEED)
    out["geometry"] = geo
    return out
