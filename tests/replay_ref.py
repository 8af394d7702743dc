"""Test infrastructure: the CPU statement of the replay recorder (snake_engine.replay, snk_pit_record_moves / _boards) in plain
Python, written from the reference's own lines -- the move and eat phases of Game.tic (game.py:87-127; Snake.move 329-358,
Snake.grow 360-365), the two calls of Game.draw (game.py:140-141, 194-195) and Game.draw itself (game.py:281-300).

Boards are the compact dicts of snake_engine.engine.compact_from_state / oracle.snake_oracle.Game.compact: nodes[s][:length[s]]
are snake s's cells y * W + x, head first.  The statement keeps linked-list-free copies of what the reference keeps: a snake is
[id, length, [(y, x) head, body ...]].  The food of the mid-tick board is what self.food holds at game.py:141 -- the food before
the tick less what was eaten plus what was spawned -- which is the food of the post-state, since the removal of dead snakes
(game.py:143-192) never touches it; tick_frames checks that against its own eat phase.

The one rule that is the project's and not the reference's: the engine does not move a game with fewer than two snakes alive
(Game.tic returned the rewards list on the tick before, game.py:199-202), and the recorder draws such a game, when its live flag
is still set, as it stands in both frames."""
import numpy as np

EMPTY, FOOD = 0, 9


def snakes_of(W, st):
    """the alive snakes of a compact board in id order (the order of Game.snakes)"""
    out = []
    for s in range(len(st["alive"])):
        if st["alive"][s]:
            n = int(st["length"][s])
            out.append([s, n, [divmod(int(c), W) for c in st["nodes"][s][:n]]])
    return out


def food_of(W, st):
    return {divmod(int(c), W) for c in np.flatnonzero(np.asarray(st["food"]))}


def draw(H, W, food, snakes):
    """Game.draw (game.py:281-300) -> int8[H][W]"""
    board = [[EMPTY] * W for _ in range(H)]
    for y, x in food:                                                       # :284-285
        board[y][x] = FOOD
    for sid, _, cells in sorted(snakes, key=lambda sn: sn[1]):              # :287, a stable sort of a list in id order
        hy, hx = cells[0]
        if 0 <= hy < H and 0 <= hx < W:                                     # :289-291
            board[hy][hx] = -(sid + 1)
    for sid, _, cells in snakes:                                            # :292-294
        for y, x in cells[1:]:
            board[y][x] = sid + 1
    return np.array(board, np.int8)


def tick_frames(H, W, pre, dense, post):
    """pre, post: the compact boards before and after one tick, dense: the move of every snake id -> (mid, post) frames"""
    snakes = snakes_of(W, pre)
    if len(snakes) < 2:                                                     # not moved (see the module's docstring)
        frame = draw(H, W, food_of(W, post), snakes_of(W, post))
        return frame, frame.copy()
    food = food_of(W, pre)
    for sn in snakes:                                                       # :90-95
        d = (int(dense[sn[0]]) + int(pre["dir"][sn[0]]) - 1) % 4            # :92
        hy, hx = sn[2][0]
        head = (hy - 1, hx) if d == 0 else (hy, hx + 1) if d == 1 else (hy + 1, hx) if d == 2 else (hy, hx - 1)   # :330-342
        sn[2] = [head] + sn[2][:-1]                                         # :343-350: new head, the tail node leaves
    for sn in snakes:                                                       # :121-127, list order
        if sn[2][0] in food:
            food.remove(sn[2][0])
            sn[1] += 1                                                      # :361
            sn[2].append(sn[2][-1])                                         # :362-365: the tail, doubled
    after = food_of(W, post)
    assert food <= after and len(after - food) <= 1, "the post-state's food is not the food at the first draw"
    return draw(H, W, after, snakes), draw(H, W, after, snakes_of(W, post))


def text(frames):
    """game.py:296-300 over a list of boards"""
    out = ""
    for frame in frames:
        for row in np.asarray(frame).tolist():
            out += str(row) + "\n"
        out += "\n"
    return out.encode("ascii")


class Recording:
    """an oracle game whose tic also draws: the statement's players (oracle.pit_oracle.pit_run, tests/script_ref.py::script_run,
    the search references) play a list of these as they play bare games, and .frames then holds two boards per tick"""

    def __init__(self, game):
        self._game = game
        self.frames = []

    def __getattr__(self, name):
        return getattr(self._game, name)

    def tic(self, dense, *args, **kwargs):
        g = self._game.g
        pre = self._game.compact()
        done = self._game.tic(dense, *args, **kwargs)
        self.frames.extend(tick_frames(g.H, g.W, pre, dense, self._game.compact()))
        return done
