"""Test infrastructure: the CPU statement of the pit's tally (snake_engine.tally, snk_pit_tally) in plain Python, written from the
reference's own lines -- the move, health, eat and death phases of Game.tic (game.py:87-165; Snake.move 329-358, Snake.grow
360-365) for one tick, with the sets the reference keeps (heads, bodies, food) rebuilt from the board before the tick.

Boards are the compact dicts of snake_engine.engine.compact_from_state / oracle.snake_oracle.Game.compact: nodes[s][:length[s]]
are snake s's cells y * W + x, head first.

The one rule that is the project's and not the reference's: the engine does not move a game with fewer than two snakes alive
(Game.tic returned the rewards list on the tick before, game.py:199-202); tick_fates returns None for such a board."""
import numpy as np

ALIVE, WALL, BODY, HEAD, STARVED = range(5)
FATES = ("alive", "wall", "body", "head", "starved")


def tick_fates(H, W, health_dec, pre, dense):
    """pre: the compact board before the tick, dense: the move of every snake id -> (fate, eats, length), int32[S] each: the fate
    code of every snake alive before the tick (0: it lives; 0 for a snake that was dead already), whether it ate, and its length
    after the eat phase (0 for a snake that was dead already).  None for a board the engine does not move."""
    S = len(pre["alive"])
    ids = [s for s in range(S) if pre["alive"][s]]                          # Game.snakes, in id order
    if len(ids) < 2:
        return None
    cells = {s: [divmod(int(c), W) for c in pre["nodes"][s][:int(pre["length"][s])]] for s in ids}
    length = {s: int(pre["length"][s]) for s in ids}
    health = {s: int(pre["health"][s]) for s in ids}
    food = {divmod(int(c), W) for c in np.flatnonzero(np.asarray(pre["food"])[:H * W])}
    bodies = {c for s in ids for c in cells[s][1:]}                         # Game.bodies: every node but the heads
    heads = {}
    for s in ids:                                                           # :90-114
        d = (int(dense[s]) + int(pre["dir"][s]) - 1) % 4                    # :92
        hy, hx = cells[s][0]
        new = (hy - 1, hx) if d == 0 else (hy, hx + 1) if d == 1 else (hy + 1, hx) if d == 2 else (hy, hx - 1)   # :330-342
        old_tail = cells[s][-1]
        cells[s] = [new] + cells[s][:-1]                                    # :343-350
        heads.setdefault(new, []).append(s)                                 # :97-101
        bodies.add(cells[s][1] if len(cells[s]) > 1 else old_tail)          # :109, the old head
        if old_tail != cells[s][-1]:                                        # :354-356: a doubled tail keeps its cell
            bodies.discard(old_tail)                                        # :110-111
    for s in ids:                                                           # :117-118
        health[s] -= health_dec
    eats = {s: 0 for s in ids}
    for s in ids:                                                           # :121-127, list order
        if cells[s][0] in food:
            food.remove(cells[s][0])
            health[s] = 100
            length[s] += 1
            cells[s].append(cells[s][-1])
            eats[s] = 1
    fate = {s: ALIVE for s in ids}
    for s in ids:                                                           # :145-165
        y, x = cells[s][0]
        if y < 0 or y >= H or x < 0 or x >= W:
            fate[s] = WALL
        elif (y, x) in bodies:
            fate[s] = BODY
        elif len(heads[(y, x)]) > 1:
            for t in heads[(y, x)]:
                if length[s] <= length[t] and t != s:
                    fate[s] = HEAD
                    break
        elif health[s] <= 0:
            fate[s] = STARVED
    out = np.zeros((3, S), np.int32)
    for s in ids:
        out[:, s] = fate[s], eats[s], length[s]
    return out[0], out[1], out[2]


class Counting:
    """a game of the statement's players (oracle.pit_oracle.pit_run, tests/script_ref.py::script_run, the search and league
    references) whose tic also tallies: they play a list of these as they play bare games.  fate / died / food / length are the
    int32[S] rows a Tally holds for this game; ticks counts the tics, so died is the match's turn number"""

    def __init__(self, game):
        self._game = game
        S = game.g.S
        self.fate, self.died, self.food, self.length = (np.zeros(S, np.int32) for _ in range(4))
        self.ticks = 0

    def __getattr__(self, name):
        return getattr(self._game, name)

    def tic(self, dense, *args, **kwargs):
        g = self._game.g
        got = tick_fates(g.H, g.W, g.health_dec, self._game.compact(), dense)
        self.ticks += 1
        if got is not None:
            fate, eats, length = got
            was = np.asarray(self._game.compact()["alive"]).astype(bool)
            self.food += eats
            self.length[was] = length[was]
            self.fate[fate > 0] = fate[fate > 0]
            self.died[fate > 0] = self.ticks
        return self._game.tic(dense, *args, **kwargs)
