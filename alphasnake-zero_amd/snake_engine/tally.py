"""Tally: every seat's fate in a device pit match.  A match returns winners and game lengths; a tally says how each seat's game
went -- who hit a wall, who ran into a body, who lost a head-on, who starved, on which turn, how much each seat ate and how long
it grew.  The engine's counters are per game: when two snakes die on one tick from different causes they cannot say which seat
died how, and reading the boards back each turn is the one thing the pit avoids.

``Arena.tally()`` / ``League.tally()`` return a ``Tally`` that the next match on that arena or league fills.  One kernel per turn,

    snk_pit_tally                 before the step: Game.tic's move, eat and death phases (game.py:90-165) restated for this tick from
                                  the records and the dense moves, a wavefront per game, into int32[4][games][snakes] on the device
    snk_engine_step_active_tape

and that array comes to the host in one copy after the last turn.  The turn's read-back stays the one it is; a recorder
(snake_engine/replay.py) may be active in the same match.

    fate      a code of FATES = ("alive", "wall", "body", "head", "starved"); 0: alive when the game's verdict came in
    died      the turn the seat died on, 0 for a seat alive at the verdict
    food      food eaten
    length    the final length; of a dead seat the length it died with

``by_owner()`` gives a row per side -- team A and team B of an arena match, every owner of a league match: seats, the count per
fate, food eaten, mean final length, mean turns lived.  ``games(owner, fate)`` gives the games in which a seat of that owner met
that fate -- what one hands to ``record()`` when the match is replayed from the same seed.  ``text(names)`` is the table as text.

The class and its helpers are defined in snake_engine/arena.py (that module imports only the library binding and the engine, and
the league imports the arena); this module is the name they are imported by."""
from .arena import FATES, Tally, TallyRows, fate_code  # noqa: F401
