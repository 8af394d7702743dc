"""Test infrastructure: the CPU statement of territory at the leaf (snake_engine.arena.Lookahead / Deep / Playout with
leaf=Territory(flags, hungry); snk_pit_look_values_leaf, snk_pit_deep_values_leaf, snk_pit_playout_values_leaf) in plain Python:
the three searches of tests/look_ref.py, tests/deep_ref.py and tests/playout_ref.py, which take the row-scoring function as their
`score` parameter, with the leaf's function for it; and side_scores, the scores of any scripted side, which the match player
(script_ref.run) moves by.

A row-scoring function is `score(H, W, st, flags, only=None) -> {s: the three scores}` over the alive snakes of a compact board
(only: of those ids): `scorer(None)` is script_ref.board_scores, `scorer(RefTerritory(flags, hungry))` is
territory_ref.board_scores with that threshold.  The policy (include/snake_engine.h) is the one of the three files with every
"the plain scores of script_ref" read as "score":

    lookahead  fallback (A < 2 or A > 4): score of the board;  leaf of s in child c: dead, WIN = 2^24 when alone, else
               max(score(c)[s]);  the fold as in look_ref
    deep       fallback: score of the board at every depth;  V_1 the lookahead;  V_k over the same children with max(V_{k-1}) as
               the leaf and -2 - dead - 32 (k - 1) for a move that can be punished
    playout    fallback (A < 2): score of the board;  plain(a) = score of the board; every playout move from score of the
               sub-game as it stands, with the Philox draw of playout_ref;  value and score as in playout_ref"""
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
from deep_ref import board_deep_scores              # the three searches under this module's name, as its tests call them
from look_ref import board_look_scores
from playout_ref import board_playout_scores

LEAF_SCRIPT, LEAF_TERRITORY = 0, 1                  # SNK_LEAF_* of include/snake_engine.h


def scorer(leaf):
    """the row-scoring function of a leaf: None or a plain RefScripted -- the script; a RefTerritory -- territory with its hungry"""
    if leaf is None or type(leaf) is R.RefScripted:
        return R.board_scores
    assert type(leaf) is T.RefTerritory, leaf
    return lambda H, W, st, flags=R.ALL, only=None: T.board_scores(H, W, st, flags, leaf.hungry, only)


def leaf_args(leaf):
    """(leaf, hungry) as the C entry points take them"""
    return (LEAF_SCRIPT, 100) if leaf is None or type(leaf) is R.RefScripted else (LEAF_TERRITORY, leaf.hungry)


def side_scores(side, H, W, S, health_dec, st, g, only=None):
    """{s: three scores} (only: of those ids) of the board in slot g for a scripted side of any kind"""
    if not isinstance(side, (P.RefPlayout, D.RefDeep, K.RefLookahead)):
        return scorer(side)(H, W, st, side.flags, only)             # the script or territory itself
    assert side.leaf is None or side.leaf.flags == side.flags, side.leaf
    score = scorer(side.leaf)
    if isinstance(side, P.RefPlayout):
        return board_playout_scores(H, W, S, health_dec, st, g, side.P, side.T, side.eps, side.seed, side.flags, score, only)
    if isinstance(side, D.RefDeep):
        return board_deep_scores(H, W, S, health_dec, st, side.depth, side.flags, score, only)
    return board_look_scores(H, W, S, health_dec, st, side.flags, score, only)


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


SPAWN_SEED = 59
N_DUEL, N_LEAGUE = 16, 2
CAP_LEAGUE = 2                                      # the turn cap the league match shares: 6 561 territory leaves a board in Python
MATCH_P, MATCH_T = 2, 3


def four_owner_table(n):
    """four seats, four owners, a seat each, rotated from game to game"""
    return np.array([[(s + g) % 4 for s in range(4)] for g in range(n)], np.uint8)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the statement's run of one of the matches, with the moves of every turn; computed once and shared (callers must not change
    it)"""
    leaf = T.RefTerritory(hungry=HUNGRY)
    rival = T.RefTerritory(hungry=HUNGRY)
    if name == "league-11x11x4":                  # a seat each: Deep(2), Lookahead and Playout over territory, and the plain script
        games, geo = SR.start_games("11x11x4", N_LEAGUE)
        out = R.run(games, [D.RefDeep(2, leaf=leaf), K.RefLookahead(leaf=leaf), P.RefPlayout(MATCH_P, MATCH_T, seed=9, leaf=leaf),
                            R.RefScripted()], four_owner_table(N_LEAGUE), SPAWN_SEED, CAP_LEAGUE, log_moves=True)
    else:                                         # a territory-leaf player against Territory(hungry=40), sixteen recorded start boards
        side = {"deep-7x7x2": D.RefDeep(2, leaf=leaf), "look-7x7x2": K.RefLookahead(leaf=leaf),
                "playout-7x7x2": P.RefPlayout(MATCH_P, MATCH_T, leaf=leaf)}[name]
        games, geo = SR.start_games("7x7x2", N_DUEL)
        out = R.run(games, [side, rival], LR.two_team_table(N_DUEL, 2, 1), SPAWN_SEED, R.NO_CAP, log_moves=True)
    out["geometry"] = geo
    return out
