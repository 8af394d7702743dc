"""Replay: chosen games of a device pit match as the boards the reference draws -- Game.tic(show=True) appends two boards per
tick to replay.rep (Game.draw, game.py:281-300, called at game.py:140-141 and 194-195) and player.py shows them.

``Arena.record(games)`` / ``League.record(games)`` return a ``Replay`` that the next match on that arena or league fills.  The
match keeps what it was built for -- one read-back per turn, no per-game Python -- so no state is exported while it runs: two
kernels per turn draw the boards of the recorded games into a log in device memory,

    snk_pit_record_moves          before the step: the snakes of the mid-tick board, from the records and the dense moves
    snk_engine_step_active_tape
    snk_pit_record_boards         after the step, before the verdict: the food into that board, and the post-tick board

and the log comes to the host in one copy after the last turn.  The log is int8[turns][recorded games][2][stride]; the host knows
the turn number, so it grows the log by doubling between turns (a device-to-device copy, nothing is read back).  A game is drawn
on the turns the step moved it: game g ends up with 2 * lengths[g] frames, lengths being the match result's own verdict turns.

Cell codes (game.py:281-294): 0 empty, 9 food, -(id + 1) a head, id + 1 a body node.

The class and its helpers are defined in snake_engine/arena.py (that module imports only the library binding and the engine, and
the league imports the arena); this module is the name they are imported by."""
from .arena import Replay, board_text, checked_games, frames_text  # noqa: F401
