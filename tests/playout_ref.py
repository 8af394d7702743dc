"""Test infrastructure: the CPU statement of the playout opponent (snake_engine.arena.Playout, snk_pit_playout_values) in plain
Python, built on tests/script_ref.py (the plain scores, snk_pit_moves' tie order), the stepper of tests/look_ref.py (Game.subgame
and Game.tic of the C game of oracle/, no food spawning) and the Philox of tests/mcts_ref.py; script_ref.run plays it in matches.

The policy (include/snake_engine.h), for snake s of the board in slot g with A snakes alive, P playouts, horizon T, exploration eps
and a 64-bit seed:

    fallback  A < 2: the plain scores of script_ref.scores
    plain(a)  the three plain scores of s on the board itself; a blocked move (-1) scores -1 and is not played out
    playout   (a, p), p < P: a sub-game of the board, stepped for ticks i < T.  At tick 0 s makes move a; every other alive snake,
              and s too from tick 1 on, makes its playout move; dead snakes' entries are 1
    move      of snake t at tick i: q = t's plain scores on the sub-game as it stands; r = philox4x32_10((g, s | a << 4 | t << 8,
              p | i << 8, TAG), (seed low, seed high)); with n = the moves with q != -1: the (r[1] % n)-th of them in ascending
              order when (r[0] & 255) < eps and n > 0, else script_ref.move(q)
    value     i when s is not alive after the step of tick i; 2T as soon as s is alive and no other snake is; else T
    score     4 * sum of the P values + (the moves b != a with plain(b) < plain(a))

The move is script_ref.move of the three scores.  Nothing here is shared with the kernels."""
import functools

import numpy as np

import league_ref as LR
import look_ref as K
import script_ref as R
import search_pit_ref as SR
from mcts_ref import philox4x32_10
from oracle import snake_oracle

TAG = 0x504C4159                                    # counter word 3 of every playout draw
MAX_P, MAX_T, MAX_EPS = 64, 64, 256


def high(P, T):
    """the largest score: every playout ends with s alone, both other moves score less"""
    return 8 * T * P + 2


def playout_move(q, r, eps):
    """the playout move from the three plain scores q and the four Philox words r"""
    free = [a for a in range(3) if q[a] != -1]
    if (int(r[0]) & 255) < eps and free:
        return free[int(r[1]) % len(free)]
    return R.move(q)


def playout_value(root, g, s, a, p, T, eps, seed, flags, score=R.board_scores):
    """the value of playout (a, p) of snake s of the oracle game `root` in slot g, every snake's playout move taken from the
    row-scoring function `score`; root is not changed"""
    c = root.subgame()
    S, H, W = c.g.S, c.g.H, c.g.W
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for i in range(T):
        alive = c.alive_ids()
        assert s in alive and len(alive) >= 2
        q = score(H, W, c.compact(), flags)
        r = philox4x32_10((g, [s | a << 4 | t << 8 for t in alive], p | i << 8, TAG), key)
        moves = np.ones(S, np.uint8)
        for k, t in enumerate(alive):
            moves[t] = a if i == 0 and t == s else playout_move(q[t], r[k], eps)
        c.tic(moves)
        assert c.last_spawn == -1                   # a sub-game spawns no food
        left = c.alive_ids()
        if s not in left:
            return i
        if left == [s]:
            return 2 * T
    return T


def board_playout_scores(H, W, S, health_dec, st, g, P, T, eps=64, seed=0, flags=R.ALL, score=R.board_scores, only=None):
    """{s: the three playout scores} of the alive snakes of the compact board st standing in slot g (only: of those ids), the
    plain scores those of the row-scoring function `score` (script_ref.board_scores, or leaf_ref.scorer of a leaf)"""
    assert 1 <= P <= MAX_P and 1 <= T <= MAX_T and 0 <= eps <= MAX_EPS and 0 <= seed < 1 << 64
    plain = score(H, W, st, flags)
    if len(plain) < 2:
        return plain if only is None else {s: z for s, z in plain.items() if s in only}
    root = snake_oracle.Game.from_compact(H, W, S, health_dec, 0.15, st)
    out = {}
    for s in plain if only is None else [s for s in only if s in plain]:
        z = plain[s]
        out[s] = [-1 if z[a] == -1 else
                  4 * sum(playout_value(root, g, s, a, p, T, eps, seed, flags, score) for p in range(P)) + sum(z[b] < z[a] for b in range(3) if b != a)
                  for a in range(3)]
    return out


def playout_scores(H, W, S, health_dec, st, g, s, P, T, eps=64, seed=0, flags=R.ALL):
    """the three scores of snake s; [-1, -1, -1] for a dead or absent snake"""
    if not 0 <= s < S or not st["alive"][s]:
        return [-1, -1, -1]
    return board_playout_scores(H, W, S, health_dec, st, g, P, T, eps, seed, flags, only=[s])[s]


class RefPlayout(R.RefScripted):
    """the statement's side of a match: what snake_engine.arena.Playout(flags, P, T, eps, seed, leaf) is on the device"""

    def __init__(self, P=8, T=8, eps=64, seed=0, flags=R.ALL, leaf=None):
        super().__init__(flags)
        self.P, self.T, self.eps, self.seed, self.leaf = P, T, eps, seed, leaf


# ---- what the tests share -------------------------------------------------------------------------------------------------------------
def _first(alive, count):
    return int(np.flatnonzero(alive == count)[0])


# which boards of the golden trajectory tic_<cfg>.npz: a handful per geometry, chosen by the number of snakes alive so that every
# count the geometry reaches is met, the ones above four (where Lookahead and Deep fall back) included
PICK = {"5x5x2": lambda alive: list(range(0, len(alive), 9)),
        "7x7x2": lambda alive: list(range(0, len(alive), 40)),
        "9x9x3": lambda alive: [_first(alive, 3), _first(alive, 2), _first(alive, 2) + 5],
        "11x11x4": lambda alive: [_first(alive, 4), _first(alive, 3), _first(alive, 2)],
        "16x16x6": lambda alive: [_first(alive, 5), _first(alive, 6)],
        "19x19x8": lambda alive: [int(np.flatnonzero(alive >= 6)[-1]), _first(alive, 8)]}


@functools.lru_cache(maxsize=None)
def sampled(cfg):
    """(H, W, S, health_dec, boards): a few boards of a golden configuration, as few as keep the statement quick"""
    from conftest import golden_state, load_golden
    z = load_golden(f"tic_{cfg}.npz")
    H, W, S, hd = (int(z[k]) for k in ("H", "W", "S", "health_dec"))
    return H, W, S, hd, [golden_state(z, i) for i in PICK[cfg](z["st_alive"].sum(1))]


@functools.lru_cache(maxsize=None)
def sampled_scores(cfg, P=2, T=3, eps=64, seed=0, flags=R.ALL):
    """[board g] -> {s: the three scores}: the statement over sampled(cfg), board g in slot g, computed once and shared (callers
    must not change it)"""
    H, W, S, hd, boards = sampled(cfg)
    return [board_playout_scores(H, W, S, hd, st, g, P, T, eps, seed, flags) for g, st in enumerate(boards)]


# ---- hand-built boards.  Cells are (y, x); heading 0 = y-1, 1 = x+1, 2 = y+1, 3 = x-1; move 0 turns left, 1 goes straight, 2 right
# A dead-end corridor that closes within six ticks.  Snake 0 (length 3) heads x-1 along the top edge at (0, 4): straight is (0, 3),
# the mouth of the corridor (0, 3) .. (0, 0) under which snake 1 (length 11, heading down the left edge, away) lies on (1, 0) ..
# (1, 3) for six more ticks; left is (1, 4), the open right half of the board; right leaves the board.  The corridor's four cells are
# room enough for a snake of three, and the food at its end draws the plain script in, one tick deep as well.  Inside, every tick
# has one unblocked move, the food is eaten at tick 3, and at tick 4 nothing is left.
CORRIDOR = R.board(7, 7, [([(0, 4), (0, 5), (0, 6)], 3),
                          ([(3, 0), (2, 0), (1, 0), (1, 1), (1, 2), (1, 3), (2, 3), (3, 3), (4, 3), (5, 3), (6, 3)], 2)], food=[(0, 0)])

_STUB = ([(6, 6), (6, 5)], 3)                       # a third snake that is dead where a board needs two


def _hand():
    lone = R.board(7, 7, [([(3, 3), (3, 2), (3, 1)], 1), ([(0, 0), (0, 1)], 3), _STUB], food=[(5, 5)], dead=[1, 2])
    # snake 0 has two ticks of health left and no food within reach of them
    starve = R.board(7, 7, [([(3, 3), (3, 2), (3, 1)], 1), ([(0, 1), (0, 0), (1, 0)], 1), _STUB], food=[(6, 0)], dead=[2])
    starve["health"][0] = 2
    # snake 1 (length 4) has one unblocked move, straight on to (3, 3), which is also straight on for snake 0 (length 3)
    headon = R.board(7, 7, [([(3, 2), (3, 1), (3, 0)], 1), ([(3, 4), (3, 5), (4, 5), (4, 4)], 3), ([(2, 4), (2, 5), (2, 6)], 3)])
    return 7, 7, 3, 1, [lone, starve, headon]


HAND = _hand()
LONE, STARVE, HEADON = range(3)


SPAWN_SEED = 53
N_DUEL, N_FOUR, N_LEAGUE = 16, 3, 2
CAP_FOUR, CAP_LEAGUE = 3, 3                         # turn caps the device matches share
MATCH_P, MATCH_T = 2, 3


@functools.lru_cache(maxsize=None)
def reference(name):
    """the statement's run of one of the matches, computed once and shared (callers must not change it)"""
    if name == "duel-7x7x2":                      # Playout(P=2, T=3) against Scripted(), one snake each, sixteen recorded start boards
        games, geo = SR.start_games("7x7x2", N_DUEL)
        out = R.run(games, [RefPlayout(MATCH_P, MATCH_T), R.RefScripted()], LR.two_team_table(N_DUEL, 2, 1), SPAWN_SEED, R.NO_CAP)
    elif name == "strength-7x7x2":                # the reading of DESIGN section 7: RefPlayout(P=4, T=6) against RefScripted()
        games, geo = SR.start_games("7x7x2", N_DUEL)
        out = R.run(games, [RefPlayout(4, 6), R.RefScripted()], LR.two_team_table(N_DUEL, 2, 1), SPAWN_SEED, R.NO_CAP)
    elif name == "1v3-11x11x4":                   # one Playout against three snakes of Scripted(), cut at CAP_FOUR turns
        games, geo = SR.start_games("11x11x4", N_FOUR)
        out = R.run(games, [RefPlayout(MATCH_P, MATCH_T), R.RefScripted()], LR.two_team_table(N_FOUR, 4, 1), SPAWN_SEED, CAP_FOUR)
    else:                                         # a playout owner, a lookahead owner and a scripted owner, cut at CAP_LEAGUE turns
        assert name == "league-11x11x4"
        games, geo = SR.start_games("11x11x4", N_LEAGUE)
        out = R.run(games, [RefPlayout(MATCH_P, MATCH_T, seed=9), K.RefLookahead(), R.RefScripted(R.SPACE)],
                    R.three_owner_table(N_LEAGUE), SPAWN_SEED, CAP_LEAGUE)
    out["geometry"] = geo
    return out
