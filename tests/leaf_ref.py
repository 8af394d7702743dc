"""Test infrastructure: the CPU statement of territory at the leaf (snake_engine.arena.Lookahead / Deep / Playout with
leaf=Territory(flags, hungry); snk_pit_look_values_leaf, snk_pit_deep_values_leaf, snk_pit_playout_values_leaf) in plain Python:
the three searches of tests/look_ref.py, tests/deep_ref.py and tests/playout_ref.py with the row-scoring function as a parameter,
and a match player.

A row-scoring function is `score(H, W, st, flags, only=None) -> {s: the three scores}` over the alive snakes of a compact board
(only: of those ids): `scorer(None)` is script_ref.board_scores, `scorer(RefTerritory(flags, hungry))` is
territory_ref.board_scores with that threshold.  The policy (include/snake_engine.h) is the one of the three files with every
"the plain scores of script_ref" read as "score":

    lookahead  fallback (A < 2 or A > 4): score of the board;  leaf of s in child c: dead, WIN = 2^24 when alone, else
               max(score(c)[s]);  the fold as in look_ref
    deep       fallback: score of the board at every depth;  V_1 the lookahead;  V_k over the same children with max(V_{k-1}) as
               the leaf and -2 - dead - 32 (k - 1) for a move that can be punished
    playout    fallback (A < 2): score of the board;  plain(a) = score of the board; every playout move from score of the
               sub-game as it stands, with the Philox draw of playout_ref;  value and score as in playout_ref

The children and the stepping come from look_ref / playout_ref (the C game of oracle/); where those files call script_ref directly
their few lines are restated here.  With scorer(None) every function gives what its namesake gives (tests/test_leaf_cpu.py)."""
import functools

import numpy as np

import deep_ref as D
import league_ref as LR
import look_ref as K
import playout_ref as P
import script_ref as R
import search_pit_ref as SR
import territory_ref as T
from conftest import golden_state, load_golden
from mcts_ref import philox4x32_10
from oracle import snake_oracle
from oracle.mcts_oracle import argmaxs

WIN = K.WIN
LEAF_SCRIPT, LEAF_TERRITORY = 0, 1                  # SNK_LEAF_* of include/snake_engine.h


def _script(H, W, st, flags=R.ALL, only=None):
    q = R.board_scores(H, W, st, flags)
    return q if only is None else {s: z for s, z in q.items() if s in only}


def scorer(leaf):
    """the row-scoring function of a leaf: None or a plain RefScripted -- the script; a RefTerritory -- territory with its hungry"""
    if leaf is None or type(leaf) is R.RefScripted:
        return _script
    assert type(leaf) is T.RefTerritory, leaf

    def territory(H, W, st, flags=R.ALL, only=None):
        their = T.fronts(H, W, st) if flags & R.SPACE else None
        return {s: T.scores(H, W, st, s, flags, leaf.hungry, their)
                for s in range(len(st["alive"])) if st["alive"][s] and (only is None or s in only)}
    return territory


def leaf_args(leaf):
    """(leaf, hungry) as the C entry points take them"""
    return (LEAF_SCRIPT, 100) if leaf is None or type(leaf) is R.RefScripted else (LEAF_TERRITORY, leaf.hungry)


def _fold(leaf, alive, only, punished):
    """look_ref's fold: {s: three scores} from [child j] -> {s: leaf value}"""
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


def board_look_scores(H, W, S, health_dec, st, flags=R.ALL, score=_script, only=None):
    """{s: the three lookahead scores} of the alive snakes of a compact board, the children's rows scored by `score`"""
    return board_deep_scores(H, W, S, health_dec, st, 1, flags, score, only)


def board_deep_scores(H, W, S, health_dec, st, depth, flags=R.ALL, score=_script, only=None):
    """{s: the three scores of a search `depth` ticks deep} of the alive snakes of a compact board"""
    assert depth >= 1
    A = int(np.count_nonzero(st["alive"][:S]))
    if A < 2 or A > 4:
        return score(H, W, st, flags, only)
    children, alive = K.child_boards(H, W, S, health_dec, st)
    mine = alive if only is None else [s for s in alive if s in only]
    leaf = []
    for c in children:
        left = [s for s in mine if c["alive"][s]]
        if not left:
            leaf.append({})
        elif sum(bool(c["alive"][s]) for s in alive) >= 2:    # 2 .. A alive: never the fallback below the root
            below = score(H, W, c, flags, left) if depth == 1 else board_deep_scores(H, W, S, health_dec, c, depth - 1, flags, score, left)
            leaf.append({s: max(below[s]) for s in left})
        else:
            leaf.append({s: WIN for s in left})
    return _fold(leaf, alive, only, -2 - D.STEP_PENALTY * (depth - 1))


def playout_value(root, g, s, a, p, T_, eps, seed, flags, score=_script):
    """playout_ref.playout_value with every snake's playout move taken from `score`"""
    c = root.subgame()
    S, H, W = c.g.S, c.g.H, c.g.W
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for i in range(T_):
        alive = c.alive_ids()
        assert s in alive and len(alive) >= 2
        q = score(H, W, c.compact(), flags)
        r = philox4x32_10((g, [s | a << 4 | t << 8 for t in alive], p | i << 8, P.TAG), key)
        moves = np.ones(S, np.uint8)
        for k, t in enumerate(alive):
            moves[t] = a if i == 0 and t == s else P.playout_move(q[t], r[k], eps)
        c.tic(moves)
        assert c.last_spawn == -1                   # a sub-game spawns no food
        left = c.alive_ids()
        if s not in left:
            return i
        if left == [s]:
            return 2 * T_
    return T_


def board_playout_scores(H, W, S, health_dec, st, g, P_, T_, eps=64, seed=0, flags=R.ALL, score=_script, only=None):
    """{s: the three playout scores} of the alive snakes of the compact board st standing in slot g (only: of those ids)"""
    assert 1 <= P_ <= P.MAX_P and 1 <= T_ <= P.MAX_T and 0 <= eps <= P.MAX_EPS and 0 <= seed < 1 << 64
    plain = score(H, W, st, flags)
    if len(plain) < 2:
        return plain if only is None else {s: z for s, z in plain.items() if s in only}
    root = snake_oracle.Game.from_compact(H, W, S, health_dec, 0.15, st)
    out = {}
    for s in plain if only is None else [s for s in only if s in plain]:
        z = plain[s]
        out[s] = [-1 if z[a] == -1 else
                  4 * sum(playout_value(root, g, s, a, p, T_, eps, seed, flags, score) for p in range(P_))
                  + sum(z[b] < z[a] for b in range(3) if b != a) for a in range(3)]
    return out


# ---- the sides of a match ------------------------------------------------------------------------------------------------------------
def _checked(leaf, flags):
    assert leaf is None or (type(leaf) in (R.RefScripted, T.RefTerritory) and leaf.flags == flags), leaf
    return leaf


class RefLookahead(K.RefLookahead):
    """what snake_engine.arena.Lookahead(flags, leaf) is on the device"""

    def __init__(self, flags=R.ALL, leaf=None):
        super().__init__(flags)
        self.leaf = _checked(leaf, flags)


class RefDeep(D.RefDeep):
    """what snake_engine.arena.Deep(flags, depth, leaf) is on the device"""

    def __init__(self, depth=2, flags=R.ALL, leaf=None):
        super().__init__(depth, flags)
        self.leaf = _checked(leaf, flags)


class RefPlayout(P.RefPlayout):
    """what snake_engine.arena.Playout(flags, P, T, eps, seed, leaf) is on the device"""

    def __init__(self, P=8, T=8, eps=64, seed=0, flags=R.ALL, leaf=None):
        super().__init__(P, T, eps, seed, flags)
        self.leaf = _checked(leaf, flags)


def side_scores(side, H, W, S, health_dec, st, g, only=None):
    """{s: three scores} of the board in slot g for a scripted side of any kind"""
    if isinstance(side, RefPlayout):
        return board_playout_scores(H, W, S, health_dec, st, g, side.P, side.T, side.eps, side.seed, side.flags, scorer(side.leaf), only)
    if isinstance(side, RefDeep):
        return board_deep_scores(H, W, S, health_dec, st, side.depth, side.flags, scorer(side.leaf), only)
    if isinstance(side, RefLookahead):
        return board_look_scores(H, W, S, health_dec, st, side.flags, scorer(side.leaf), only)
    if isinstance(side, T.RefTerritory):
        return scorer(side)(H, W, st, side.flags, only)
    return P.side_scores(side, H, W, S, health_dec, st, g, only)


# ---- the match player -------------------------------------------------------------------------------------------------------------
def leaf_run(games, sides, owner, spawn_seed, max_turns=None):
    """playout_ref.playout_run with the sides above and RefTerritory among them (a game's slot is its index).  Returns what
    playout_run returns, and moves [turn - 1] = {game: the dense moves of the turn}"""
    S, K_ = games[0].g.S, len(sides)
    H, W, hd = games[0].g.H, games[0].g.W, games[0].g.health_dec
    owner = np.asarray(owner)
    assert owner.shape == (len(games), S) and owner.min() >= 0 and owner.max() < K_
    rng = np.random.RandomState(spawn_seed)
    winners, lengths = [None] * len(games), [0] * len(games)
    live = list(range(len(games)))
    counts, spawn_log, moves_log, turn = [], [], [], 0
    while live and (max_turns is None or turn < max_turns):
        turn += 1
        dense = {g: np.ones(S, np.uint8) for g in live}
        rows_of = []
        for o in range(K_):
            ids = [(g, s) for g in live for s in games[g].alive_ids() if owner[g][s] == o]
            rows_of.append(len(ids))
            if isinstance(sides[o], R.RefScripted):
                for g in sorted({g for g, _ in ids}):
                    mine = [s for gg, s in ids if gg == g]
                    q = side_scores(sides[o], H, W, S, hd, games[g].compact(), g, mine)
                    for s in mine:
                        dense[g][s] = R.move(q[s])
            elif ids:
                for (g, s), m in zip(ids, argmaxs(sides[o].v([games[g].make_state(s) for g, s in ids]))):
                    dense[g][s] = m
        counts.append(rows_of)
        moves_log.append(dense)
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
                lengths=lengths, turns=turn, counts=counts, spawn_log=spawn_log, moves=moves_log, boards=[g.compact() for g in games],
                open=live)


# ---- what the tests share -------------------------------------------------------------------------------------------------------------
HUNGRY = 40
# which recorded boards (the states of tests/golden/states_<cfg>.npz, in order of recording): as few as keep the statement quick.
# 7x7x2 and 11x11x4_dec9 are played to the end, so they hold unequal lengths, eaten food, dead snakes and a lone survivor, and at
# decrement 9 the health crosses HUNGRY within seven ticks; 19x19x8 gives games above four alive (the searches' fallback) and below
EVERY = {"7x7x2": 5, "11x11x4_dec9": 9, "19x19x8": 57}


@functools.lru_cache(maxsize=None)
def recorded(cfg):
    """(H, W, S, health_dec, boards): every EVERY[cfg]-th recorded board of states_<cfg>.npz (its boards are those of
    tic_<cfg>.npz that state_index names: the boards somebody still moves on), and behind them the first board of the trajectories
    with a lone survivor, which no observation was recorded of"""
    z = load_golden(f"tic_{cfg}.npz")
    index = np.unique(load_golden(f"states_{cfg}.npz")["state_index"])
    H, W, S, hd = (int(k_) for k_ in (z["H"], z["W"], z["S"], z["health_dec"]))
    lone = int(np.flatnonzero(z["st_alive"].sum(1) == 1)[0])
    return H, W, S, hd, [golden_state(z, int(i)) for i in list(index[::EVERY[cfg]]) + [lone]]


def deep_boards(cfg):
    """the indices into recorded(cfg) of the boards the deep search is stated on: at 7x7x2 every other one; at 11x11x4, where depth
    2 is 6 561 leaves a board with four alive, the first board of every count of snakes alive"""
    H, W, S, hd, boards = recorded(cfg)
    if cfg == "7x7x2":
        return list(range(0, len(boards), 2)) + [len(boards) - 1]
    alive = [int(st["alive"].sum()) for st in boards]
    return sorted(alive.index(a) for a in set(alive))


@functools.lru_cache(maxsize=None)
def look_scores(cfg, flags=R.ALL, hungry=None):
    """[board] -> {s: three scores} of the lookahead over recorded(cfg); hungry None: the script leaf.  Computed once and shared
    (callers must not change it)"""
    H, W, S, hd, boards = recorded(cfg)
    score = scorer(None if hungry is None else T.RefTerritory(flags, hungry))
    return [board_look_scores(H, W, S, hd, st, flags, score) for st in boards]


@functools.lru_cache(maxsize=None)
def deep_scores(cfg, depth, flags=R.ALL, hungry=None):
    """{board index: {s: three scores}} of the deep search over deep_boards(cfg), shared as above"""
    H, W, S, hd, boards = recorded(cfg)
    score = scorer(None if hungry is None else T.RefTerritory(flags, hungry))
    return {i: board_deep_scores(H, W, S, hd, boards[i], depth, flags, score) for i in deep_boards(cfg)}


@functools.lru_cache(maxsize=None)
def playout_scores(cfg, P_=2, T_=3, eps=64, seed=0, flags=R.ALL, hungry=None):
    """[board g] -> {s: three scores} of the playout over recorded(cfg), board g in slot g, shared as above"""
    H, W, S, hd, boards = recorded(cfg)
    score = scorer(None if hungry is None else T.RefTerritory(flags, hungry))
    return [board_playout_scores(H, W, S, hd, st, g, P_, T_, eps, seed, flags, score) for g, st in enumerate(boards)]


# A hand-built board on which the two leaves disagree.  Cells are (y, x); heading 0 = y-1, 1 = x+1, 2 = y+1, 3 = x-1; move 0 turns
# left, 1 goes straight, 2 right.  See tests/test_leaf_cpu.py for what it shows.
def cut_off_board():
    return CUT_OFF


CUT_OFF = None                                      # set below

SPAWN_SEED = 59
N_DUEL, N_LEAGUE = 16, 2
CAP_LEAGUE = 2                                      # the turn cap the league match shares: 6 561 territory leaves a board in Python
MATCH_P, MATCH_T = 2, 3


def four_owner_table(n):
    """four seats, four owners, a seat each, rotated from game to game"""
    return np.array([[(s + g) % 4 for s in range(4)] for g in range(n)], np.uint8)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the statement's run of one of the matches, computed once and shared (callers must not change it)"""
    leaf = T.RefTerritory(hungry=HUNGRY)
    rival = T.RefTerritory(hungry=HUNGRY)
    if name == "league-11x11x4":                  # a seat each: Deep(2), Lookahead and Playout over territory, and the plain script
        games, geo = SR.start_games("11x11x4", N_LEAGUE)
        out = leaf_run(games, [RefDeep(2, leaf=leaf), RefLookahead(leaf=leaf), RefPlayout(MATCH_P, MATCH_T, seed=9, leaf=leaf),
                               R.RefScripted()], four_owner_table(N_LEAGUE), SPAWN_SEED, CAP_LEAGUE)
    else:                                         # a territory-leaf player against Territory(hungry=40), sixteen recorded start boards
        side = {"deep-7x7x2": RefDeep(2, leaf=leaf), "look-7x7x2": RefLookahead(leaf=leaf),
                "playout-7x7x2": RefPlayout(MATCH_P, MATCH_T, leaf=leaf)}[name]
        games, geo = SR.start_games("7x7x2", N_DUEL)
        out = leaf_run(games, [side, rival], LR.two_team_table(N_DUEL, 2, 1), SPAWN_SEED)
    out["geometry"] = geo
    return out
