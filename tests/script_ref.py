"""Test infrastructure: the CPU statement of the scripted opponent (snake_engine.arena.Scripted, snk_pit_script_values) in plain
Python over compact boards -- the dicts snake_engine.engine.compact_from_state makes of exported snk_game_state records, which is
also the format of the golden trajectories -- and a match player built on it that steps with oracle.snake_oracle, as
tests/league_ref.py and tests/league_search_ref.py do.

The policy (include/snake_engine.h), for snake s of a board and relative move a in {0 left, 1 straight, 2 right}:

    target    the head moved by d = (a + dir + 3) & 3, 0 = y-1, 1 = x+1, 2 = y+1, 3 = x-1
    occupied  nodes 0 .. length-1 of every alive snake (tails and s's own body included); dead snakes occupy nothing
    blocked   target off the board or occupied: score -1
    space     cells reachable from the target by 4-neighbour steps over free cells, the target included -- by a QUEUE here, one
              cell at a time (the kernel shifts whole bit planes: nothing of that is shared)
    room      min(space, length_s, 255);  safe: 0 when another alive snake at least as long has its head next to the target
    food      H + W - (smallest Manhattan distance from the target to a food cell), 0 without food;  fill: min(space, 511)
    score     ((room * 2 + safe) * 64 + food) * 512 + fill

flags (SPACE 1, HEADS 2, FOOD 4) switch the parts off: room = fill = 0, safe = 1, food = 0.  The move is argmaxs of the three
scores with the strict comparisons of snk_pit_moves (oracle.mcts_oracle.argmaxs; `move` below restates it)."""
import functools
from collections import deque

import numpy as np

import league_ref as LR
import search_pit_ref as SR
from oracle.mcts_oracle import SelfPlayOracle, argmaxs

SPACE, HEADS, FOOD = 1, 2, 4
ALL = SPACE | HEADS | FOOD
KEYS = LR.KEYS
STEP = ((-1, 0), (0, 1), (1, 0), (0, -1))          # heading d -> (dy, dx)


def board(H, W, snakes, food=(), dead=()):
    """a compact board built by hand.  snakes: a list of (cells head..tail as (y, x), heading); food: (y, x) cells; dead: ids
    whose alive flag is cleared (their nodes stay in the record, as a stale ring would)"""
    S = len(snakes)
    n = max(len(c) for c, _ in snakes)
    st = dict(alive=np.ones(S, np.uint8), health=np.full(S, 90, np.int16), length=np.zeros(S, np.int16), dir=np.zeros(S, np.uint8),
              nodes=np.full((S, n), -1, np.int16), food=np.zeros(H * W, np.uint8), rewards=np.zeros(S, np.int8),
              counters=np.zeros(6, np.int32))
    for s, (cells, d) in enumerate(snakes):
        st["length"][s], st["dir"][s] = len(cells), d
        st["nodes"][s, :len(cells)] = [y * W + x for y, x in cells]
    for y, x in food:
        st["food"][y * W + x] = 1
    for s in dead:
        st["alive"][s] = 0
    return st


def flood(H, W, occupied, y, x):
    """cells reachable from the free cell (y, x), itself included: a queue, one cell at a time"""
    seen = {(y, x)}
    todo = deque(seen)
    while todo:
        cy, cx = todo.popleft()
        for dy, dx in STEP:
            c = (cy + dy, cx + dx)
            if 0 <= c[0] < H and 0 <= c[1] < W and c not in seen and c[0] * W + c[1] not in occupied:
                seen.add(c)
                todo.append(c)
    return len(seen)


def region_sizes(H, W, occupied):
    """{free cell (y, x): the size of its region}: every region flooded once by the same queue (for scoring many rows of a board)"""
    sizes = {}
    for y in range(H):
        for x in range(W):
            if (y, x) in sizes or y * W + x in occupied:
                continue
            seen = {(y, x)}
            todo = deque(seen)
            while todo:
                cy, cx = todo.popleft()
                for dy, dx in STEP:
                    c = (cy + dy, cx + dx)
                    if 0 <= c[0] < H and 0 <= c[1] < W and c not in seen and c[0] * W + c[1] not in occupied:
                        seen.add(c)
                        todo.append(c)
            sizes.update(dict.fromkeys(seen, len(seen)))
    return sizes


def board_scores(H, W, st, flags=ALL, only=None):
    """{s: scores(H, W, st, s, flags)} of every alive snake of a board (only: of those ids), its regions flooded once.  This is
    the form of a row-scoring function: what the searches of look_ref, deep_ref and playout_ref take as `score`"""
    alive = [t for t in range(len(st["alive"])) if st["alive"][t]]
    occupied = {int(c) for t in alive for c in st["nodes"][t][:int(st["length"][t])]}
    sizes = region_sizes(H, W, occupied) if flags & SPACE else None
    return {s: scores(H, W, st, s, flags, sizes) for s in alive if only is None or s in only}


def scores(H, W, st, s, flags=ALL, sizes=None):
    """the three integer scores of snake s of the compact board st; [-1, -1, -1] for a dead snake.  sizes: region_sizes of the
    board, when the caller scores several rows of it"""
    S = len(st["alive"])
    if not 0 <= s < S or not st["alive"][s]:
        return [-1, -1, -1]
    alive = [t for t in range(S) if st["alive"][t]]
    occupied = {int(c) for t in alive for c in st["nodes"][t][:int(st["length"][t])]}
    length = int(st["length"][s])
    hy, hx = divmod(int(st["nodes"][s][0]), W)
    foods = [divmod(int(c), W) for c in np.flatnonzero(st["food"][:H * W])]
    out = []
    for a in range(3):
        dy, dx = STEP[(a + int(st["dir"][s]) + 3) & 3]
        y, x = hy + dy, hx + dx
        if not (0 <= y < H and 0 <= x < W) or y * W + x in occupied:
            out.append(-1)
            continue
        space = (flood(H, W, occupied, y, x) if sizes is None else sizes[(y, x)]) if flags & SPACE else 0
        safe = 1
        if flags & HEADS:
            for t in alive:
                ty, tx = divmod(int(st["nodes"][t][0]), W)
                if t != s and int(st["length"][t]) >= length and abs(ty - y) + abs(tx - x) == 1:
                    safe = 0
        food = 0
        if flags & FOOD and foods:
            food = H + W - min(abs(fy - y) + abs(fx - x) for fy, fx in foods)
        out.append(((min(space, length, 255) * 2 + safe) * 64 + food) * 512 + min(space, 511))
    return out


def move(z):
    """snk_pit_moves' greedy move of three scores: strict comparisons, so of equal best scores the later move wins"""
    if z[0] > z[1]:
        return 0 if z[0] > z[2] else 2
    return 1 if z[1] > z[2] else 2


class RefScripted:
    """the statement's side of a match: what snake_engine.arena.Scripted(flags) is on the device"""

    def __init__(self, flags=ALL):
        self.flags = flags


# ---- the match player -------------------------------------------------------------------------------------------------------------
NO_CAP = float("inf")                               # a turn cap that never cuts: the result still says which games are open


def run(games, sides, owner, spawn_seed, max_turns=None, log_moves=False, searching=None, tapes=None, depth=4, breadth=8, base=100):
    """the match player of every scripted statement: league_ref.league_run / league_search_ref.league_search_run with scripted
    owners.  sides[o] is a RefScripted of any kind (its moves are `move` of leaf_ref.side_scores; a game's slot is its index) or a
    net with .v; searching[o]: owner o (a net) moves by search with the uniform tape tapes[o].  A scripted owner counts as a greedy
    one.  Food from RandomState(spawn_seed), two uniforms per open game and turn in game order.  Returns a dict: winners (None for
    a draw), winner_owner, lengths, turns, counts [turn - 1] (without a searcher the K row counts; with one the greedy owners' row
    counts in owner order, then the K counts of games per owner), spawn_log, boards; and
        max_turns   (a turn cap; NO_CAP for none) open: the games still open after it, which stay as they stand, without a winner
        log_moves   moves [turn - 1] = {game: the dense moves of the turn}
        searching   tape_pos [o] = how far owner o's tape was read, None for an owner that does not search"""
    from leaf_ref import side_scores                # the module that sees every player class; it imports this one
    S, K = games[0].g.S, len(sides)
    H, W, hd = games[0].g.H, games[0].g.W, games[0].g.health_dec
    owner = np.asarray(owner)
    assert owner.shape == (len(games), S) and owner.min() >= 0 and owner.max() < K
    rng = np.random.RandomState(spawn_seed)
    oracles = [SelfPlayOracle(side, base, False, depth, breadth, draws=SR.CheckedDraws(tapes[o])) if s else None
               for o, (side, s) in enumerate(zip(sides, searching or [False] * K))]
    winners, lengths = [None] * len(games), [0] * len(games)
    live = list(range(len(games)))
    counts, spawn_log, moves_log, turn = [], [], [], 0
    while live and (max_turns is None or turn < max_turns):
        turn += 1
        dense = {g: np.ones(S, np.uint8) for g in live}
        rows_of, games_of = [], [0] * K
        for o in range(K):
            if oracles[o] is not None:
                mine = [g for g in live if any(owner[g][s] == o for s in games[g].alive_ids())]
                games_of[o] = len(mine)
                if mine:
                    rows, V, moves = oracles[o].root_turn([games[g] for g in mine])
                    for (gi, s), m in zip(rows, moves):
                        if owner[mine[gi]][s] == o:
                            dense[mine[gi]][s] = m
                continue
            ids = [(g, s) for g in live for s in games[g].alive_ids() if owner[g][s] == o]
            rows_of.append(len(ids))
            if isinstance(sides[o], RefScripted):
                for g in sorted({g for g, _ in ids}):
                    mine = [s for gg, s in ids if gg == g]
                    q = side_scores(sides[o], H, W, S, hd, games[g].compact(), g, mine)
                    for s in mine:
                        dense[g][s] = move(q[s])
            elif ids:
                for (g, s), m in zip(ids, argmaxs(sides[o].v([games[g].make_state(s) for g, s in ids]))):
                    dense[g][s] = m
        counts.append(rows_of + games_of if searching and any(searching) else rows_of)
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
    out = dict(winners=winners, winner_owner=[None if w is None else int(owner[g][w]) for g, w in enumerate(winners)],
               lengths=lengths, turns=turn, counts=counts, spawn_log=spawn_log, boards=[g.compact() for g in games])
    if max_turns is not None:
        out["open"] = live
    if log_moves:
        out["moves"] = moves_log
    if searching is not None:
        out["tape_pos"] = [None if o is None else o.draw.pos for o in oracles]
    return out


def script_run(games, sides, owner, spawn_seed, searching=None, **search):
    """run with searching owners, or with none of them: it returns tape_pos either way"""
    return run(games, sides, owner, spawn_seed, searching=searching or [False] * len(sides), **search)


# ---- the matches of the GPU test ---------------------------------------------------------------------------------------------------
def three_owner_table(n):
    """four seats, three owners (0 and 1 scripted, 2 the stub net): every owner meets every other, and owner 2 holds two seats in
    a third of the games"""
    rows = ([0, 1, 2, 1], [2, 0, 1, 2], [1, 2, 0, 0])
    return np.array([rows[g % 3] for g in range(n)], np.uint8)


SPAWN_SEED = 31
N_DUEL, N_FOUR, N_LEAGUE, N_SEARCH = 16, 12, 12, 5
TAPE_SEED = 17


@functools.lru_cache(maxsize=None)
def reference(name):
    """the statement's run of one of the GPU test's matches, computed once and shared (callers must not change it)"""
    if name == "duel-7x7x2":                      # Scripted() against Scripted(SPACE | FOOD), sixteen recorded start boards
        games, geo = SR.start_games("7x7x2", N_DUEL)
        out = script_run(games, [RefScripted(), RefScripted(SPACE | FOOD)], LR.two_team_table(N_DUEL, 2, 1), SPAWN_SEED)
    elif name == "1v3-11x11x4":                   # one Scripted() against three snakes of Scripted(HEADS)
        games, geo = SR.start_games("11x11x4", N_FOUR)
        out = script_run(games, [RefScripted(), RefScripted(HEADS)], LR.two_team_table(N_FOUR, 4, 1), SPAWN_SEED)
    elif name == "league-11x11x4":                # two scripted owners with different flags and stub net 0
        games, geo = SR.start_games("11x11x4", N_LEAGUE)
        out = script_run(games, [RefScripted(), RefScripted(SPACE), LR.RefStub(0)], three_owner_table(N_LEAGUE), SPAWN_SEED)
    else:                                         # the same with the stub moving by a taped sequential search
        assert name == "league-search-11x11x4"
        games, geo = SR.start_games("11x11x4", N_SEARCH)
        out = script_run(games, [RefScripted(), RefScripted(SPACE), LR.RefStub(0)], three_owner_table(N_SEARCH), SPAWN_SEED,
                         searching=(False, False, True), tapes=[None, None, SR.uniform_tape(TAPE_SEED)], depth=4, breadth=8)
    out["geometry"] = geo
    return out
