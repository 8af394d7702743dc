"""Test infrastructure: the CPU statement of the deep opponent (snake_engine.arena.Deep, snk_pit_deep_values) in plain Python, built
on tests/look_ref.py (the children, the depth-1 scores, the fold) and tests/script_ref.py (the plain scores, the match player).

The policy (include/snake_engine.h), for snake s of a board with A snakes alive, V_k = the three scores of a search k ticks deep:

    fallback  A < 2 or A > 4: the plain scores of script_ref.scores, at every depth
    V_1       look_ref.board_look_scores
    V_k       k >= 2, over the 3^A children of look_ref.child_boards:
      leaf_k(c)  dead -- s is not alive in c; WIN = 2^24 -- s alone is alive; else max(V_{k-1}(c, s, .))
      score      of own move a, over the children whose digit of s is a: min(leaf_k) when s lives in all of them, else
                 -2 - (the number of them in which s is dead) - 32 * (k - 1)

The move is script_ref.move of the three scores.  Nothing here is shared with the kernels."""
import functools

import numpy as np

import league_ref as LR
import look_ref as K
import script_ref as R
import search_pit_ref as SR

WIN = K.WIN
STEP_PENALTY = 32                                   # a death one tick earlier costs this much: above the 27 ways to die of a tick


def low(depth):
    """the smallest value a search `depth` ticks deep can give"""
    return -STEP_PENALTY * (depth - 1) - 29


def fanout(S, depth):
    F = K.fanout(S) ** depth
    return F if 2 <= S <= 8 and depth >= 1 and F <= 6561 else -1


def board_deep_scores(H, W, S, health_dec, st, depth, flags=R.ALL, score=R.board_scores, only=None):
    """{s: the three scores of a search `depth` ticks deep} of the alive snakes of a compact board (only: of those ids), the rows
    scored by the row-scoring function `score` as in look_ref.board_look_scores"""
    assert depth >= 1
    A = int(np.count_nonzero(st["alive"][:S]))
    if depth == 1 or A < 2 or A > 4:                # the fallback is the lookahead's
        return K.board_look_scores(H, W, S, health_dec, st, flags, score, only)
    children, alive = K.child_boards(H, W, S, health_dec, st)
    leaf = []
    for c in children:
        left = [s for s in alive if c["alive"][s]]
        mine = [s for s in left if only is None or s in only]
        if len(left) >= 2 and mine:                 # 2 .. A alive: never the fallback
            below = board_deep_scores(H, W, S, health_dec, c, depth - 1, flags, score, mine)
            leaf.append({s: max(below[s]) for s in mine})
        else:
            leaf.append({s: WIN for s in mine})
    return K.fold(leaf, alive, only, -2 - STEP_PENALTY * (depth - 1))


def deep_scores(H, W, S, health_dec, st, s, depth, flags=R.ALL):
    """the three scores of snake s; [-1, -1, -1] for a dead or absent snake"""
    if not 0 <= s < S or not st["alive"][s]:
        return [-1, -1, -1]
    return board_deep_scores(H, W, S, health_dec, st, depth, flags)[s]


class RefDeep(R.RefScripted):
    """the statement's side of a match: what snake_engine.arena.Deep(flags, depth, leaf) is on the device"""

    def __init__(self, depth=2, flags=R.ALL, leaf=None):
        super().__init__(flags)
        self.depth, self.leaf = depth, leaf


# ---- what the tests share -------------------------------------------------------------------------------------------------------------
EVERY = {"7x7x2": 2, "9x9x3": 4, "11x11x4": 13}      # of look_ref.sampled's boards: depth 2 is 81, 729 and 6 561 leaves a board here
PICK = {"5x5x2": lambda alive: range(0, len(alive), 6),                         # of the golden trajectory itself
        "16x16x6": lambda alive: [int(np.flatnonzero(alive == 4)[0]), int(np.flatnonzero(alive == 5)[0])]}
LIMIT = {"11x11x4": 4}


@functools.lru_cache(maxsize=None)
def sampled(cfg):
    """(H, W, S, health_dec, boards): a few boards of a golden configuration, as few as keep the statement quick"""
    if cfg in EVERY:
        H, W, S, hd, boards = K.sampled(cfg)
        return H, W, S, hd, boards[::EVERY[cfg]][:LIMIT.get(cfg)]
    from conftest import golden_state, load_golden
    z = load_golden(f"tic_{cfg}.npz")
    H, W, S, hd = (int(z[k]) for k in ("H", "W", "S", "health_dec"))
    return H, W, S, hd, [golden_state(z, i) for i in PICK[cfg](z["st_alive"].sum(1))]


@functools.lru_cache(maxsize=None)
def sampled_scores(cfg, depth, flags=R.ALL):
    """[board] -> {s: the three scores}: the statement over sampled(cfg), computed once and shared (callers must not change it)"""
    H, W, S, hd, boards = sampled(cfg)
    return [board_deep_scores(H, W, S, hd, st, depth, flags) for st in boards]


SPAWN_SEED = 47
N_DUEL, N_FOUR, N_LEAGUE = 16, 4, 2
CAP_FOUR, CAP_LEAGUE = 2, 2                         # turn caps the device matches share: 6 561 leaves a board and turn in Python


@functools.lru_cache(maxsize=None)
def reference(name):
    """the statement's run of one of the matches, computed once and shared (callers must not change it)"""
    if name == "duel-7x7x2":                      # Deep(depth=2) against Lookahead(), one snake each, sixteen recorded start boards
        games, geo = SR.start_games("7x7x2", N_DUEL)
        out = R.run(games, [RefDeep(2), K.RefLookahead()], LR.two_team_table(N_DUEL, 2, 1), SPAWN_SEED, R.NO_CAP)
    elif name == "1v3-11x11x4":                   # one Deep(depth=2) against three snakes of Scripted(), cut at CAP_FOUR turns
        games, geo = SR.start_games("11x11x4", N_FOUR)
        out = R.run(games, [RefDeep(2), R.RefScripted()], LR.two_team_table(N_FOUR, 4, 1), SPAWN_SEED, CAP_FOUR)
    else:                                         # a deep owner, a scripted owner and stub net 0, cut at CAP_LEAGUE turns
        assert name == "league-11x11x4"
        games, geo = SR.start_games("11x11x4", N_LEAGUE)
        out = R.run(games, [RefDeep(2), R.RefScripted(R.SPACE), LR.RefStub(0)], R.three_owner_table(N_LEAGUE), SPAWN_SEED, CAP_LEAGUE)
    out["geometry"] = geo
    return out
