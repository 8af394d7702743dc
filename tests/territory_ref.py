"""Test infrastructure: the CPU statement of the territory opponent (snake_engine.arena.Territory, snk_pit_territory_values) in
plain Python over the compact boards of tests/script_ref.py, whose match player (script_ref.run) plays it.

The policy (include/snake_engine.h), for snake s of a board and relative move a:

    target, occupied, blocked   as in script_ref.scores: a blocked move scores -1
    free        the on-board cells that are not occupied
    start set   of another alive snake t: the targets of t's three moves that are free (it may be empty)
    d_s(c)      the fewest 4-neighbour steps from the target to c over free cells; d_t(c): the same from the nearest cell of t's
                start set -- by a QUEUE here, one cell at a time (the kernel shifts whole bit planes: nothing of that is shared).
                Fronts do not block each other
    territory   the free cells c with d_s(c) finite, d_s(c) < d_t(c) for every alive t != s at least as long as s (strong) and
                d_s(c) <= d_t(c) for every shorter one (weak)
    room        min(territory, length_s, 255);  fill: min(territory, 511);  safe: as in the script
    food        the script's food term when health_s <= hungry, else 0
    score       ((room * 2 + safe) * 64 + food) * 512 + fill

flags (SPACE 1, HEADS 2, FOOD 4) switch the parts off as in the script; without SPACE no distance is taken.  The move is
script_ref.move of the three scores."""
import functools
from collections import deque

import numpy as np

import league_ref as LR
import script_ref as R
import search_pit_ref as SR
from conftest import golden_state, load_golden

FAR = 1 << 30                                       # the distance of a cell a front never reaches


def distances(H, W, occupied, sources):
    """{cell (y, x): the fewest steps from the nearest of the free cells `sources`} over free cells: a queue, one cell at a time.
    A cell that is not reached has no entry"""
    dist = {c: 0 for c in sources}
    todo = deque(dist)
    while todo:
        cy, cx = todo.popleft()
        for dy, dx in R.STEP:
            c = (cy + dy, cx + dx)
            if 0 <= c[0] < H and 0 <= c[1] < W and c not in dist and c[0] * W + c[1] not in occupied:
                dist[c] = dist[(cy, cx)] + 1
                todo.append(c)
    return dist


def _occupied(st):
    return {int(c) for t in range(len(st["alive"])) if st["alive"][t] for c in st["nodes"][t][:int(st["length"][t])]}


def targets(H, W, st, t):
    """the three cells (y, x) snake t's moves lead to, off-board ones included"""
    hy, hx = divmod(int(st["nodes"][t][0]), W)
    return [(hy + dy, hx + dx) for dy, dx in (R.STEP[(a + int(st["dir"][t]) + 3) & 3] for a in range(3))]


def start_set(H, W, st, t, occupied):
    """the cells snake t can stand on after this tick: its targets that are on the board and free"""
    return [(y, x) for y, x in targets(H, W, st, t) if 0 <= y < H and 0 <= x < W and y * W + x not in occupied]


def fronts(H, W, st):
    """{t: d_t} of every alive snake of a board, from its start set (for scoring many rows of a board)"""
    occupied = _occupied(st)
    return {t: distances(H, W, occupied, start_set(H, W, st, t, occupied)) for t in range(len(st["alive"])) if st["alive"][t]}


def territory(H, W, st, s, y, x, their=None):
    """the territory of snake s behind its free target (y, x)"""
    occupied = _occupied(st)
    their = fronts(H, W, st) if their is None else their
    length = int(st["length"][s])
    strong = [d for t, d in their.items() if t != s and int(st["length"][t]) >= length]
    weak = [d for t, d in their.items() if t != s and int(st["length"][t]) < length]
    count = 0
    for c, mine in distances(H, W, occupied, [(y, x)]).items():
        if all(mine < d.get(c, FAR) for d in strong) and all(mine <= d.get(c, FAR) for d in weak):
            count += 1
    return count


def territories(H, W, st, s, their=None):
    """the territory behind each of snake s's three moves, None for a blocked one"""
    occupied = _occupied(st)
    their = fronts(H, W, st) if their is None else their
    return [territory(H, W, st, s, y, x, their) if 0 <= y < H and 0 <= x < W and y * W + x not in occupied else None
            for y, x in targets(H, W, st, s)]


def scores(H, W, st, s, flags=R.ALL, hungry=100, their=None, terrs=None):
    """the three integer scores of snake s of the compact board st; [-1, -1, -1] for a dead or absent snake.  their: fronts of
    the board, when the caller scores several rows of it; terrs: territories of the row, when the caller scores it several times"""
    S = len(st["alive"])
    if not 0 <= s < S or not st["alive"][s]:
        return [-1, -1, -1]
    alive = [t for t in range(S) if st["alive"][t]]
    occupied = _occupied(st)
    length = int(st["length"][s])
    foods = [divmod(int(c), W) for c in np.flatnonzero(st["food"][:H * W])]
    if flags & R.SPACE and their is None and terrs is None:
        their = fronts(H, W, st)
    out = []
    for a, (y, x) in enumerate(targets(H, W, st, s)):
        if not (0 <= y < H and 0 <= x < W) or y * W + x in occupied:
            out.append(-1)
            continue
        terr = (territory(H, W, st, s, y, x, their) if terrs is None else terrs[a]) if flags & R.SPACE else 0
        safe = 1
        if flags & R.HEADS:
            for t in alive:
                ty, tx = divmod(int(st["nodes"][t][0]), W)
                if t != s and int(st["length"][t]) >= length and abs(ty - y) + abs(tx - x) == 1:
                    safe = 0
        food = 0
        if flags & R.FOOD and foods and int(st["health"][s]) <= hungry:
            food = H + W - min(abs(fy - y) + abs(fx - x) for fy, fx in foods)
        out.append(((min(terr, length, 255) * 2 + safe) * 64 + food) * 512 + min(terr, 511))
    return out


def board_scores(H, W, st, flags=R.ALL, hungry=100, only=None):
    """{s: scores(H, W, st, s, flags, hungry)} of every alive snake of a board (only: of those ids), the other snakes' distances
    taken once"""
    their = fronts(H, W, st) if flags & R.SPACE else None
    return {s: scores(H, W, st, s, flags, hungry, their)
            for s in range(len(st["alive"])) if st["alive"][s] and (only is None or s in only)}


def parts(score):
    """(room, safe, food, fill) of a score that is not -1"""
    return score >> 16, (score >> 15) & 1, (score >> 9) & 63, score & 511


class RefTerritory(R.RefScripted):
    """the statement's side of a match: what snake_engine.arena.Territory(flags, hungry) is on the device"""

    def __init__(self, flags=R.ALL, hungry=100):
        super().__init__(flags)
        self.hungry = hungry


# ---- what the tests share: the golden boards, the statement over them and the matches of the GPU test ------------------------------
@functools.lru_cache(maxsize=None)
def golden(cfg):
    """(H, W, S, boards): every board of the golden trajectories tic_<cfg>.npz"""
    z = load_golden(f"tic_{cfg}.npz")
    H, W, S = int(z["H"]), int(z["W"]), int(z["S"])
    return H, W, S, [golden_state(z, i) for i in range(z["st_alive"].shape[0])]


@functools.lru_cache(maxsize=None)
def golden_territories(cfg):
    """[board] -> {s: territories}: the distances over golden(cfg) taken once for every flags and hungry value"""
    H, W, S, boards = golden(cfg)
    out = []
    for st in boards:
        their = fronts(H, W, st)
        out.append({s: territories(H, W, st, s, their) for s in their})
    return out


@functools.lru_cache(maxsize=None)
def golden_scores(cfg, flags=R.ALL, hungry=100):
    """[board] -> {s: the three scores}: the statement over golden(cfg), computed once and shared (callers must not change it)"""
    H, W, S, boards = golden(cfg)
    return [{s: scores(H, W, st, s, flags, hungry, terrs=terrs) for s, terrs in of.items()}
            for st, of in zip(boards, golden_territories(cfg))]


def golden_hungry(cfg):
    """a hungry threshold with alive rows of golden(cfg) on both sides of it: the median of their recorded healths, less one when
    that is the largest health"""
    H, W, S, boards = golden(cfg)
    healths = sorted(int(st["health"][s]) for st in boards for s in range(S) if st["alive"][s])
    mid = healths[len(healths) // 2]
    return mid - 1 if mid == healths[-1] else mid


SPAWN_SEED = 47
N_DUEL, N_FOUR, N_LEAGUE = 16, 12, 12
HUNGRY_FOUR = 40


@functools.lru_cache(maxsize=None)
def reference(name):
    """the statement's run of one of the matches, computed once and shared (callers must not change it)"""
    if name == "duel-7x7x2":                      # Territory() against Scripted(), one snake each, sixteen recorded start boards
        games, geo = SR.start_games("7x7x2", N_DUEL)
        out = R.run(games, [RefTerritory(), R.RefScripted()], LR.two_team_table(N_DUEL, 2, 1), SPAWN_SEED)
    elif name == "1v3-11x11x4":                   # one Territory(hungry=40) against three snakes of Scripted(HEADS)
        games, geo = SR.start_games("11x11x4", N_FOUR)
        out = R.run(games, [RefTerritory(hungry=HUNGRY_FOUR), R.RefScripted(R.HEADS)], LR.two_team_table(N_FOUR, 4, 1),
                            SPAWN_SEED)
    else:                                         # a territory owner, a scripted owner and stub net 0
        assert name == "league-11x11x4"
        games, geo = SR.start_games("11x11x4", N_LEAGUE)
        out = R.run(games, [RefTerritory(), R.RefScripted(), LR.RefStub(0)], R.three_owner_table(N_LEAGUE), SPAWN_SEED)
    out["geometry"] = geo
    return out
