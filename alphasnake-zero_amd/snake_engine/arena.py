"""Arena: whole pit matches on the device -- the reference's pit loop (pit_mp_game_runner.py:14-63) with greedy agents
(pit_agent.py:10-28) as a fixed sequence of launches per turn and ONE host read-back per turn.  ``League`` (snake_engine/league.py)
plays the same turn with an owner per seat instead of two teams; the turn itself stands once, in ``_Pit._play``:

    the seating's lists           (slot, snake id) of every alive snake of every open game, bucketed by greedy side (:23-35);
                                  with a searching side also the open games a searcher plays: the slots, their alive rows, and
                                  where a seat finds its game in that list
    the turn's read-back          the counts that size the batches, one tensor, one .tolist(); nothing left ends the match
    the greedy sides              ``mixed_values``: snk_engine_observe over the nets' rows (:28), each net on its own slice (:34),
                                  a Scripted side's slice scored by snk_pit_script_values; then ONE snk_pit_moves: greedy moves
                                  into the dense move array, which it first fills with 1                              (:36-38)
    searcher.search, end_of_turn  each searching side in order, on its games; then the seating's merge launch puts the moves a
                                  searcher found for its own seats into the dense move array
    snk_engine_step_active_tape   open games move, games whose verdict is in stay as they are                         (:42)
    snk_engine_rewards
    the seating's verdict         winners, game lengths, the open flags                                               (:43-62)

There is no per-game Python loop and nothing else comes back to the host until the match is over.  The host loop of
``utils.pit_mp_game_runner.MPGameRunner.run`` (four synchronising copies, ``np.nonzero`` and a Python loop over the games each
turn) stays as the parity-pinned form; ``MPGameRunner.run_device`` is ``Arena.match`` behind the same interface.

The seating is three hooks of the subclass: ``_lists`` (the list launches and the read-back), ``_merge`` and ``_verdict``; a
fourth, ``_result``, reads the match's result back.  The arena's seating is the reference's: snakes 0 .. a_cnt-1 are team A's.

    _lists    snk_pit_rows: the row list, team A first, and the two row counts {nA, nB} -- the read-back of a match without a
              Searcher.  With one: snk_pit_roots (the open slots ascending, their alive rows, each slot's rank in that list, the
              count G), then snk_pit_rows only when one side is greedy -- it still lists both teams, the greedy team's slice is
              used --, and the read-back is {nA, nB, G}.  Every searching side gets all G open games; G = 0 ends the match
    _merge    snk_pit_search_moves: only its own team's columns of a searcher's root moves are used
    _verdict  snk_pit_verdict

A side is anything with ``v_device``, or a ``Searcher`` around one: it moves the way ``Agent(nnet, training=False).make_moves``
moves (agent.py:25-99), by a ``DeviceMCTS.search`` that simulates all snakes of its games with its own net.  The search reads back
on its own, and those are not the pit's: the largest root depth once per turn, the number of new keys once per rollout tick (it
sizes the net batch), the table status after every epoch but the last and at the end of the turn together with the turn's
sub-game tick counter; a taped (parity) search also reads its row counts.  A guarded net is calibrated once, on the first turn's
root observations.

Or a side is a ``Scripted``: the flood-fill heuristic snake every Battlesnake project keeps as its fixed point (the project's own
policy -- the reference has none; include/snake_engine.h states it, tests/script_ref.py restates it in plain Python).  It costs no
weights and is the same opponent in every run.  It counts as a greedy side; the observe launch and the nets run over the other
sides' rows only (one observe per run of consecutive nets), and ``Scripted`` against ``Scripted`` launches neither.
``Lookahead`` is a ``Scripted`` one tick deep, the second fixed point above the first: snk_pit_look_values plays every joint move
of the up to four snakes alive on copies of the game in a sub-engine the side owns, scores the copies with the plain script and
folds them into three scores per row on the device -- launches only, so the turn's read-back stays the one it is.
``Deep`` is the same search several ticks deep, the third fixed point: snk_pit_deep_values keeps one sub-engine per tick, the
children of a game shared by all its rows at every level, and folds the levels from the last one up -- launches only as well.
``Playout`` is flat Monte-Carlo over the same script, the fourth fixed point and the one without a limit on the snakes alive:
snk_pit_playout_values plays every unblocked move out a few times for several ticks on copies of the game and scores how long the
snake survives -- launches only again.
``Territory`` is the fixed point whose judgement differs in kind: snk_pit_territory_values scores a move by the cells the snake
reaches before anybody else does (Voronoi territory) instead of the cells it reaches if nobody else moves -- one launch, no copies.
``Lookahead``, ``Deep`` and ``Playout`` take ``leaf=Territory(flags, hungry)``: the searches as they are with the territory
evaluation wherever they asked the plain script -- the fallback rows, the leaves, the playout's plain scores and its playout moves
(snk_pit_look_values_leaf, snk_pit_deep_values_leaf, snk_pit_playout_values_leaf).  The same buffers, the same chunks, launches only;
without a leaf they are the players they were and call the entry points they called.

``record(games)`` returns a ``replay.Replay`` that the next match fills with the boards Game.tic(show=True) draws for those games
(game.py:140-141, 194-195): snk_pit_record_moves before the step and snk_pit_record_boards after it draw them into a log on the
device, which is copied to the host once, after the last turn (``Replay`` below; snake_engine/replay.py names it).  The turn's
read-back stays the one it is, and a match without a recorder issues no launch and no read-back for one.

``tally()`` returns a ``tally.Tally`` that the next match fills with every seat's fate: which death it died (wall, body, head-on,
starved) and on which turn, how much it ate and how long it grew.  snk_pit_tally, one launch per turn before the step, beside the
recorder's, writes them into one array on the device, which is copied to the host once, after the last turn (``Tally`` below;
snake_engine/tally.py names it).  A fifth hook, ``_owners``, gives the owner of every seat, for ``Tally.by_owner``.  A match without
a tally issues no launch and no read-back for one.
"""
from collections import namedtuple

import numpy as np
import torch

from ._lib import check, lib, EngineError
from .engine import Engine, _ptr, _stream

ArenaResult = namedtuple("ArenaResult", "winners lengths turns wins_a wins_b draws")
ArenaResult.__doc__ = """winners: int32[game_cnt] winning snake id, -1 for a draw (the reference's None); lengths: int32[game_cnt]
the turn a game's verdict came in; turns: turns played; wins_a / wins_b: games won by a snake of team A (id < alice_snake_cnt) /
team B; draws: games without a winner"""


def _device_mcts():
    """DeviceMCTS, looked up when the first Searcher plays: a match between two nets never loads the search"""
    return __import__(__package__ + ".mcts", fromlist=["DeviceMCTS"]).DeviceMCTS


class Searcher:
    """A side of a pit match that moves by search: Agent(net, softmax_base, False, depth, breadth).make_moves (agent.py:25-99) over
    the arena's open games.  It owns one DeviceMCTS with training=False (the root decision is Agent.argmaxs), with its own
    transposition table and its own rollout engine, created at the first turn, when the geometry is known."""

    def __init__(self, net, breadth=128, depth=8, softmax_base=100, seed=None, sequential=False, tape_u=None, tt_capacity=None):
        if not hasattr(net, "v_device"):
            raise TypeError(f"{type(net).__name__} has no v_device(planes, mask): the arena evaluates on the device only")
        self.net = net
        self.breadth, self.depth, self.softmax_base = int(breadth), int(depth), softmax_base
        self.seed = int(np.random.randint(1 << 62)) if seed is None else int(seed)
        self.sequential, self.tape_u, self.tt_capacity = sequential, tape_u, tt_capacity
        self.mcts = None

    def _evaluate(self, planes, mask):
        if self.mcts.guard is not None:               # gated ticks: no synchronisation per leaf batch (utils/agent.py)
            return self.net.v_device_unguarded(planes, mask)
        return self.net.v_device(planes, mask)

    def search(self, engine, slots, alive):
        """slots int32[G], alive uint8[G][S] on the device -> the root moves uint8[G][S] of every snake of those games"""
        m = self.mcts
        if m is None or (m.H, m.W, m.S, m.dev_index) != (engine.H, engine.W, engine.S, engine.device.index):
            m = self.mcts = _device_mcts()(self._evaluate, engine.H, engine.W, engine.S, self.softmax_base, False, self.depth,
                                           self.breadth, seed=self.seed, device=engine.device.index, sequential=self.sequential,
                                           tape_u=self.tape_u, tt_capacity=self.tt_capacity)
        net = self.net
        m.guard = getattr(net, "guard", None)         # the Q-net's range-guard word gates the rollout ticks
        if hasattr(net, "calibrate") and not getattr(getattr(net, "_qnet", None), "calibrated", True):
            # new weights: fit the split-f16 kernel's activation scales to real observations (the root states) once
            pairs = torch.nonzero(alive)[:4096].to(torch.int32)
            pairs[:, 0] = slots[pairs[:, 0].long()]
            planes, _, _ = engine.observe_all(pairs.contiguous(), want_mask=False, want_key=False)
            net.calibrate(planes)
        return m.search(engine, slots, alive)[1]

    def end_of_turn(self):
        if self.mcts is not None:
            self.mcts.end_of_turn()

    def clear(self):
        """Agent.clear (agent.py:140-147)"""
        if self.mcts is not None:
            self.mcts.clear()

    @property
    def tape_pos(self):
        """uniforms of tape_u consumed so far"""
        return 0 if self.mcts is None else self.mcts.tape_pos

    @property
    def stats(self):
        """DeviceMCTS.stats: net_evals, rollout_ticks, sim_steps, lookups"""
        return dict(net_evals=0, rollout_ticks=0, sim_steps=0, lookups=0) if self.mcts is None else self.mcts.stats


SCRIPT_SPACE, SCRIPT_HEADS, SCRIPT_FOOD = 1, 2, 4          # SNK_SCRIPT_* of include/snake_engine.h


class Scripted:
    """A side of a pit match (or an owner of a league match) that moves by the scripted policy of include/snake_engine.h: avoid
    walls and bodies, do not enter a pocket smaller than yourself, step away from the head of a snake at least as long, go for
    food.  flags switch the parts (SCRIPT_SPACE | SCRIPT_HEADS | SCRIPT_FOOD; 0 = any unblocked move), so one class gives several
    fixed yardsticks.  It has no net and no v_device: a Searcher around it is a TypeError."""

    def __init__(self, flags=SCRIPT_SPACE | SCRIPT_HEADS | SCRIPT_FOOD):
        flags = int(flags)
        if flags & ~(SCRIPT_SPACE | SCRIPT_HEADS | SCRIPT_FOOD):
            raise ValueError(f"Scripted flags {flags:#x}: bits outside SCRIPT_SPACE | SCRIPT_HEADS | SCRIPT_FOOD")
        self.flags = flags

    def q_rows(self, engine, pairs):
        """pairs int32[rows][2] (slot, snake id) on the device -> the three move scores float32[rows][3] on the device"""
        m = int(pairs.shape[0])
        q = engine.new((m, 3), torch.float32)
        check(engine.L.snk_pit_script_values(engine.h, _ptr(pairs), m, self.flags, _ptr(q), _stream()))
        return q


class Territory(Scripted):
    """The scripted policy with Voronoi territory in place of space (include/snake_engine.h states it): a move scores the free
    cells the snake reaches before any other snake does, every other snake starting from the cells it can stand on after this
    tick; a tie goes to the longer snake and an equal-length tie to neither.  The food term counts only for a snake whose health
    is at most `hungry` (0..100): at 100, the default, it always counts and the player is the script with territory for space;
    below 100 a snake that is not hungry maximises territory.  The same flags and refusals as Scripted, and it sits wherever a
    Scripted can; a Searcher around it is a TypeError.  One launch of snk_pit_territory_values: no sub-engine, no scratch."""

    def __init__(self, flags=SCRIPT_SPACE | SCRIPT_HEADS | SCRIPT_FOOD, hungry=100):
        super().__init__(flags)
        hungry = int(hungry)
        if not 0 <= hungry <= 100:
            raise ValueError(f"Territory hungry {hungry}: 0 .. 100")
        self.hungry = hungry

    def q_rows(self, engine, pairs):
        """pairs int32[rows][2] (slot, snake id) on the device -> the three move scores float32[rows][3] on the device"""
        m = int(pairs.shape[0])
        q = engine.new((m, 3), torch.float32)
        check(engine.L.snk_pit_territory_values(engine.h, _ptr(pairs), m, self.flags, self.hungry, _ptr(q), _stream()))
        return q


LEAF_SCRIPT, LEAF_TERRITORY = 0, 1                         # SNK_LEAF_* of include/snake_engine.h


def checked_leaf(leaf, flags):
    """the leaf evaluation of a Lookahead, a Deep or a Playout with these flags: None (the plain script; a plain Scripted means
    the same) or a Territory.  A leaf is a one-launch evaluation, so every other object -- a searching opponent too -- is a
    TypeError, and one flag set governs the root, the fallback and the leaves: other flags are a ValueError"""
    if leaf is not None and type(leaf) not in (Scripted, Territory):
        raise TypeError(f"leaf is a {type(leaf).__name__}: None, a plain Scripted or a Territory expected")
    if leaf is not None and leaf.flags != flags:
        raise ValueError(f"the leaf's flags {leaf.flags:#x} differ from the player's {flags:#x}")
    return leaf if type(leaf) is Territory else None


class _Search(Scripted):
    """What Lookahead, Deep and Playout share: the leaf, the sub-engines without food spawning and the scratch a player owns, and
    the chunks of q_rows.  _subs holds one sub-engine per level (one level for Lookahead and Playout: _sub), _handles their
    snk_engine * as an array on the host, _scratch int32 on the device.  They are made at first use; all levels are remade, and
    the replaced ones closed, when the geometry, health_dec or the device changes or level 1 is too small; the scratch only grows."""

    def __init__(self, flags, leaf):
        super().__init__(flags)
        self.leaf = checked_leaf(leaf, self.flags)
        self._subs = self._handles = self._scratch = None

    @property
    def _sub(self):
        return self._subs[0] if self._subs else None

    def _buffers(self, engine, slots, elems):
        """sub-engines of at least slots[k] slots at level k + 1, the array of their handles and a scratch of at least elems elements"""
        top = self._sub
        key = (engine.H, engine.W, engine.S, engine.health_dec, engine.device)
        if top is not None and (top.H, top.W, top.S, top.health_dec, top.device) != key:
            top = self._scratch = None
        if top is None or top.n_slots < slots[0]:
            for sub in self._subs or ():
                sub.close()
            self._subs = [Engine(n, engine.H, engine.W, engine.S, engine.health_dec, 0, seed=0, device=engine.device.index) for n in slots]
            self._handles = torch.tensor([sub.h.value for sub in self._subs], dtype=torch.int64)       # snk_engine *[levels], on the host
        if self._scratch is None or self._scratch.numel() < elems:
            self._scratch = engine.new((elems,), torch.int32)
        return self._subs, self._handles, self._scratch

    def _chunks(self, engine, pairs, name, per, need, head, tail=()):
        """q_rows in calls of at most `per` rows.  need(rows) -> the slots per level and the scratch elements of a call of that many
        rows; head(subs, handles) -> the arguments between the engine and the pair list; tail: those between the leaf and the
        scratch.  Without a leaf the call is the entry point `name` with its plain argument list, with one it is name_leaf with
        LEAF_TERRITORY and the leaf's hungry after the flags"""
        m = int(pairs.shape[0])
        q = engine.new((m, 3), torch.float32)
        leaf = () if self.leaf is None else (LEAF_TERRITORY, self.leaf.hungry)
        call = getattr(engine.L, name + "_leaf" if leaf else name)
        for lo in range(0, m, per):
            cnt = min(per, m - lo)
            subs, handles, scratch = self._buffers(engine, *need(cnt))
            check(call(engine.h, *head(subs, handles), _ptr(pairs[lo:lo + cnt]), cnt, self.flags, *leaf, *tail, _ptr(scratch),
                       _ptr(q[lo:lo + cnt]), _stream()))
        return q

    @staticmethod
    def _one(subs, handles):
        return (subs[0].h,)


LOOK_SLOT_BUDGET = 4096 * 4 * 81    # rows times fanout of one snk_pit_look_values call: a 4 096-game 11x11x4 match, every seat


class Lookahead(_Search):
    """The scripted policy one tick deep (include/snake_engine.h states it): every joint move of the up to four snakes alive is
    played on a copy of the game, the copies are scored by the plain script, and a move scores what the worst reply leaves --
    or, when a reply can kill, minus the number of ways to die.  The same flags and refusals as Scripted, and it sits wherever a
    Scripted can (mixed_values asks isinstance(side, Scripted)); a Searcher around it is a TypeError.  It owns a sub-engine
    without food spawning for the copies and the scratch of snk_pit_look_values (_Search keeps them); the sub-engine holds
    min(rows, games) * fanout slots and a call takes at most LOOK_SLOT_BUDGET // fanout rows, so it never exceeds
    LOOK_SLOT_BUDGET slots.  leaf=Territory(flags, hungry) -- the player's own flags -- scores the copies and the fallback rows by
    territory instead (snk_pit_look_values_leaf); .leaf keeps it."""

    def __init__(self, flags=SCRIPT_SPACE | SCRIPT_HEADS | SCRIPT_FOOD, leaf=None):
        super().__init__(flags, leaf)

    def q_rows(self, engine, pairs):
        """pairs int32[rows][2] (slot, snake id) on the device -> the three move scores float32[rows][3] on the device"""
        F = engine.L.snk_pit_look_fanout(engine.S)

        def need(rows):
            elems = engine.L.snk_pit_look_scratch_elems(rows, engine.S)
            if elems < 0:
                raise EngineError(f"no lookahead scratch for {rows} rows of {engine.S} snakes")
            return [min(rows, engine.n_slots) * F], elems
        # a boundary inside a game is harmless: the game is cloned again
        return self._chunks(engine, pairs, "snk_pit_look_values", max(LOOK_SLOT_BUDGET // F, 1), need, self._one)


DEEP_BYTE_BUDGET = 1 << 30           # bytes of records in the sub-engines of one snk_pit_deep_values call, all levels together


class Deep(_Search):
    """The scripted policy `depth` ticks deep (include/snake_engine.h states it): a fixed-depth paranoid search over the
    lookahead's children.  A move scores what the worst replies of the next `depth` ticks leave; a move that can be punished now
    ranks below every move that can only be punished later.  Deep(depth=1) is Lookahead bit for bit.  The same flags and refusals
    as Scripted, and it sits wherever a Scripted can; a Searcher around it is a TypeError.  It owns `depth` sub-engines without
    food spawning (level k holds min(rows, games) * fanout^k slots) and the scratch of snk_pit_deep_values (_Search keeps them).
    A call takes as many rows as keep the sub-engines' records within DEEP_BYTE_BUDGET bytes, at least one; a depth the board's
    snake count cannot have (snk_pit_deep_fanout) is refused at first use.  leaf=Territory(flags, hungry) as for Lookahead
    (snk_pit_deep_values_leaf)."""

    def __init__(self, flags=SCRIPT_SPACE | SCRIPT_HEADS | SCRIPT_FOOD, depth=2, leaf=None):
        super().__init__(flags, leaf)
        depth = int(depth)
        if depth < 1:
            raise ValueError(f"Deep depth {depth}: at least 1")
        self.depth = depth

    def q_rows(self, engine, pairs):
        """pairs int32[rows][2] (slot, snake id) on the device -> the three move scores float32[rows][3] on the device"""
        F, FD = engine.L.snk_pit_look_fanout(engine.S), engine.L.snk_pit_deep_fanout(engine.S, self.depth)
        if FD < 0:
            raise EngineError(f"Deep depth {self.depth} is too deep for {engine.S} snakes (fanout {F} a tick, at most 6561 in all)")
        levels = [F ** k for k in range(1, self.depth + 1)]

        def need(rows):
            elems = engine.L.snk_pit_deep_scratch_elems(rows, engine.S, self.depth)
            if elems < 0:
                raise EngineError(f"no deep scratch for {rows} rows of {engine.S} snakes at depth {self.depth}")
            return [min(rows, engine.n_slots) * n for n in levels], elems
        # a boundary inside a game is harmless: the game is cloned again
        return self._chunks(engine, pairs, "snk_pit_deep_values", max(DEEP_BYTE_BUDGET // (engine.slot_bytes * sum(levels)), 1), need,
                            lambda subs, handles: (_ptr(handles), self.depth))


PLAYOUT_SLOT_BUDGET = 1 << 18        # clones (rows times 3 * playouts) of one snk_pit_playout_values call: 296 MiB of 11x11x4 records


class Playout(_Search):
    """Flat Monte-Carlo over the scripted policy (include/snake_engine.h states it): every unblocked move is played out
    `playouts` times for `horizon` ticks on copies of the game, every snake following the plain script, or with probability
    `explore` / 256 a uniformly drawn unblocked move, and the move scores how long the snake survives; the plain script breaks the
    ties.  The cost is rows * 3 * playouts clones whatever the number of snakes alive, so unlike Lookahead and Deep it does not
    fall back to the plain script above four snakes, and its horizon is a parameter.  The draws are counter-based (Philox keyed by
    seed, slot and snake), so the same position and seed give the same move in every run and in every row order.  The defaults
    (8 playouts, 8 ticks, explore 64) are a starting point, not tuned values.  The same flags and refusals as Scripted, and it
    sits wherever a Scripted can; a Searcher around it is a TypeError.  It owns a sub-engine without food spawning for the
    clones and the scratch of snk_pit_playout_values (_Search keeps them); a call takes at most
    PLAYOUT_SLOT_BUDGET // (3 * playouts) rows, at least one.  leaf=Territory(flags, hungry) as for Lookahead: the plain scores
    and every playout move are territory's (snk_pit_playout_values_leaf)."""

    def __init__(self, flags=SCRIPT_SPACE | SCRIPT_HEADS | SCRIPT_FOOD, playouts=8, horizon=8, explore=64, seed=0, leaf=None):
        super().__init__(flags, leaf)
        playouts, horizon, explore, seed = int(playouts), int(horizon), int(explore), int(seed)
        if not 1 <= playouts <= 64:
            raise ValueError(f"Playout playouts {playouts}: 1 .. 64")
        if not 1 <= horizon <= 64:
            raise ValueError(f"Playout horizon {horizon}: 1 .. 64")
        if not 0 <= explore <= 256:
            raise ValueError(f"Playout explore {explore}: 0 .. 256")
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"Playout seed {seed}: 64 bits")
        self.playouts, self.horizon, self.explore, self.seed = playouts, horizon, explore, seed

    def q_rows(self, engine, pairs):
        """pairs int32[rows][2] (slot, snake id) on the device -> the three move scores float32[rows][3] on the device"""
        def need(rows):
            elems = engine.L.snk_pit_playout_scratch_elems(rows, engine.S, self.playouts)
            if elems < 0:
                raise EngineError(f"no playout scratch for {rows} rows of {engine.S} snakes and {self.playouts} playouts")
            return [rows * 3 * self.playouts], elems
        # a cut anywhere changes nothing: the draws are keyed by slot and snake
        return self._chunks(engine, pairs, "snk_pit_playout_values", max(PLAYOUT_SLOT_BUDGET // (3 * self.playouts), 1), need, self._one,
                            (self.playouts, self.horizon, self.explore, self.seed))


def mixed_values(eng, sides, rows, pairs):
    """the values float32[sum(rows)][3] of a row list in which side o (a net or a Scripted) moves the next rows[o] rows, at least
    one row in all: a Scripted side's slice is scored by the kernel; every run of consecutive nets shares one observe launch
    over its rows only, and each net with rows runs on its own slice"""
    parts, lo, o, K = [], 0, 0, len(sides)
    while o < K:
        if isinstance(sides[o], Scripted):
            if rows[o]:
                parts.append(sides[o].q_rows(eng, pairs[lo:lo + rows[o]]))
            lo += rows[o]
            o += 1
            continue
        end = o
        while end < K and not isinstance(sides[end], Scripted):
            end += 1
        cnt = sum(rows[o:end])
        if cnt:
            planes, mask, _ = eng.observe_all(pairs[lo:lo + cnt], want_key=False)
            at = 0
            for net, c in zip(sides[o:end], rows[o:end]):
                if c:
                    parts.append(net.v_device(planes[at:at + c], mask[at:at + c]))
                    at += c
        lo += cnt
        o = end
    q = parts[0] if len(parts) == 1 else torch.cat(parts)
    if q.dtype != torch.float32 or tuple(q.shape) != (lo, 3) or not q.is_cuda:
        raise EngineError(f"v_device returned {q.dtype} {tuple(q.shape)} on {q.device} for {lo} rows: float32 [rows][3] on the device expected")
    return q.contiguous()


# ---- replays of chosen games (snake_engine/replay.py is the module a user imports; the code stands here because this module
# ---- imports the library binding and the engine and nothing else of the package) ---------------------------------------------
def checked_games(games, game_cnt):
    """the recorded game indices as int32[r]: distinct, each inside 0..game_cnt-1, in the caller's order"""
    out = []
    for g in games:
        if isinstance(g, (bool, np.bool_)) or int(g) != g:
            raise ValueError(f"game index {g!r} is no integer")
        out.append(int(g))
    for g in out:
        if not 0 <= g < game_cnt:
            raise ValueError(f"game index {g} outside 0..{game_cnt - 1}")
    if len(set(out)) != len(out):
        twice = sorted(g for g in set(out) if out.count(g) > 1)
        raise ValueError(f"game index {twice[0]} is given twice")
    return np.array(out, np.int32)


def board_text(frame):
    """the bytes Game.draw appends for one board (game.py:296-300): str(row) + newline per row, then an empty line"""
    return ("".join(str([int(v) for v in row]) + "\n" for row in frame) + "\n").encode("ascii")


class Replay:
    """the frames of the recorded games of one match.  frames / text / write are there once that match is over."""

    def __init__(self, games, height, width, game_cnt, first_turns=64):
        self.games = checked_games(games, game_cnt)
        self.height, self.width = int(height), int(width)
        self.stride = lib().snk_pit_record_stride(self.height, self.width)
        if self.stride < 0:
            raise ValueError(f"no replay of a {height}x{width} board")
        if int(first_turns) < 1:
            raise ValueError(f"first_turns {first_turns}: the log starts with at least one turn")
        self.first_turns = int(first_turns)
        self.grown = 0                  # how often the log was doubled
        self.lengths = None             # int32[len(games)] once the match is over
        self._row = {int(g): i for i, g in enumerate(self.games)}
        self._log = self._slots = self._host = None

    # ---- the match's side ------------------------------------------------------------------------------------------------
    def begin(self, engine):
        """the device list of recorded slots and the first log; the library checks the list once more"""
        r = len(self.games)
        self.grown, self.lengths, self._host = 0, None, None
        self._slots = engine.new((max(r, 1),), torch.int32)
        self._log = engine.new((self.first_turns, max(r, 1), 2, self.stride), torch.int8)
        check(engine.L.snk_pit_record_slots(engine.h, self.games.ctypes.data if r else None, r, _ptr(self._slots), _stream()))

    def _turn_ptr(self, turn):
        return self._log.data_ptr() + (turn - 1) * self._log.shape[1] * 2 * self.stride

    def before_step(self, engine, turn, live, moves):
        if turn > self._log.shape[0]:   # the host counts the turns: double the log, device to device
            log = engine.new((2 * self._log.shape[0],) + tuple(self._log.shape[1:]), torch.int8)
            log[:self._log.shape[0]].copy_(self._log)
            self._log = log
            self.grown += 1
        check(engine.L.snk_pit_record_moves(engine.h, _ptr(live), _ptr(self._slots), len(self.games), _ptr(moves),
                                            self._turn_ptr(turn), _stream()))

    def after_step(self, engine, turn, live):
        check(engine.L.snk_pit_record_boards(engine.h, _ptr(live), _ptr(self._slots), len(self.games), self._turn_ptr(turn),
                                             _stream()))

    def end(self, turns, lengths):
        """the one copy of the log, after the last turn; lengths: the result's verdict turns of all games (on the host)"""
        self.lengths = np.asarray(lengths, np.int32)[self.games]
        self._host = self._log[:turns].cpu().numpy()
        self._log = self._slots = None

    # ---- the reader's side -----------------------------------------------------------------------------------------------
    def frames(self, g):
        """int8[2 * lengths[g]][H][W]: per turn the mid-tick board (game.py:140-141), then the post-tick board (:194-195)"""
        if self._host is None:
            raise RuntimeError("the match this Replay records has not been played")
        if int(g) not in self._row:
            raise KeyError(f"game {g} was not recorded (recorded: {self.games.tolist()})")
        i = self._row[int(g)]
        nc = self.height * self.width
        out = self._host[:int(self.lengths[i]), i, :, :nc]
        return np.ascontiguousarray(out).reshape(-1, self.height, self.width)

    def text(self, g):
        """the bytes Game.draw would have appended to replay.rep over game g"""
        return frames_text(self.frames(g))

    def write(self, g, path="replay.rep", append=True):
        with open(path, "ab" if append else "wb") as f:
            f.write(self.text(g))


def frames_text(frames):
    """int8[k][H][W] -> the k boards in Game.draw's text form"""
    return b"".join(board_text(fr) for fr in np.asarray(frames))


# ---- the tally of a match (snake_engine/tally.py is the module a user imports; the code stands here for the reason above) -------
FATES = ("alive", "wall", "body", "head", "starved")       # the codes snk_pit_tally writes; 0: alive when the verdict came in

TallyRows = namedtuple("TallyRows", "seats fates food length turns")
TallyRows.__doc__ = """one entry per side (Arena: team A, team B; League: every owner of the match).  seats: int64[K] seats the side
held; fates: int64[K][5] of them per fate, in the order of FATES; food: int64[K] food eaten; length: float64[K] mean final length
(a dead seat's: the length it died with); turns: float64[K] mean turns lived -- the turn a seat died on, or its game's length for a
seat alive at the verdict.  The means of a side without a seat are NaN."""


def fate_code(fate):
    """a name of FATES or its code -> the code"""
    if isinstance(fate, str):
        if fate not in FATES:
            raise ValueError(f"fate {fate!r}: one of {FATES}")
        return FATES.index(fate)
    if isinstance(fate, (bool, np.bool_)) or int(fate) != fate or not 0 <= int(fate) < len(FATES):
        raise ValueError(f"fate {fate!r}: a code 0..{len(FATES) - 1} or one of {FATES}")
    return int(fate)


class Tally:
    """every seat's fate in one match: fate, died, food, length, all int32[game_cnt][snake_cnt], there once that match is over.
    fate: a code of FATES; died: the turn the seat died on, 0 for a seat alive at the verdict; food: food eaten; length: the final
    length, of a dead seat the one it died with (eating on the last tick included)."""

    def __init__(self, game_cnt, snake_cnt):
        self.game_cnt, self.snake_cnt = int(game_cnt), int(snake_cnt)
        self.fate = self.died = self.food = self.length = None
        self.owners = self.lengths = None       # uint8[game_cnt][snake_cnt], int32[game_cnt] (the result's verdict turns)
        self.n_owners = 0
        self._dev = None

    @classmethod
    def from_arrays(cls, fate, died, food, length, owners, n_owners, lengths):
        """a Tally of arrays that are on the host already"""
        fate = np.asarray(fate)
        self = cls(*fate.shape)
        self._set(np.stack([np.asarray(a, np.int32) for a in (fate, died, food, length)]), owners, n_owners, lengths)
        return self

    def _set(self, arrays, owners, n_owners, lengths):
        n, S = self.game_cnt, self.snake_cnt
        owners, lengths = np.asarray(owners, np.uint8), np.asarray(lengths, np.int32)
        if arrays.shape != (4, n, S) or owners.shape != (n, S) or lengths.shape != (n,):
            raise ValueError(f"tally arrays {arrays.shape}, owners {owners.shape}, lengths {lengths.shape} for {n} games of {S} snakes")
        if owners.size and int(owners.max()) >= int(n_owners):
            raise ValueError(f"owner {int(owners.max())} of a table of {n_owners} owners")
        self.fate, self.died, self.food, self.length = arrays
        self.owners, self.n_owners, self.lengths = owners, int(n_owners), lengths

    # ---- the match's side ------------------------------------------------------------------------------------------------
    def begin(self, engine):
        """the four arrays as one allocation int32[4][n][S] on the device, zeroed"""
        self.fate = self.died = self.food = self.length = self.owners = self.lengths = None
        self._dev = engine.new((4, self.game_cnt, self.snake_cnt), torch.int32, 0)

    def before_step(self, engine, turn, live, moves):
        d = self._dev
        check(engine.L.snk_pit_tally(engine.h, _ptr(live), self.game_cnt, _ptr(moves), turn, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]),
                                     _ptr(d[3]), _stream()))

    def end(self, owners, n_owners, lengths):
        """the one copy of the arrays, after the last turn; lengths: the result's verdict turns (on the host)"""
        dev, self._dev = self._dev, None
        self._set(dev.cpu().numpy(), owners, n_owners, lengths)

    # ---- the reader's side -----------------------------------------------------------------------------------------------
    def _filled(self):
        if self.fate is None:
            raise RuntimeError("the match this Tally counts has not been played")

    def by_owner(self):
        """TallyRows: one entry per side"""
        self._filled()
        K = self.n_owners
        own = self.owners.reshape(-1).astype(np.int64)
        fate = self.fate.reshape(-1).astype(np.int64)
        lived = np.where(self.fate == 0, self.lengths[:, None], self.died).reshape(-1)
        seats = np.bincount(own, minlength=K)
        fates = np.bincount(own * len(FATES) + fate, minlength=K * len(FATES)).reshape(K, len(FATES))
        food = np.bincount(own, weights=self.food.reshape(-1), minlength=K).astype(np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            length = np.bincount(own, weights=self.length.reshape(-1), minlength=K) / seats
            turns = np.bincount(own, weights=lived, minlength=K) / seats
        return TallyRows(seats, fates, food, length, turns)

    def games(self, owner=None, fate=None):
        """the indices, ascending, of the games in which a seat (of that owner) met that fate (a name of FATES or its code): what
        one hands to record() when the match is replayed from the same seed.  Without a fate: the games the owner sat in"""
        self._filled()
        hit = np.ones(self.fate.shape, bool)
        if owner is not None:
            if not 0 <= int(owner) < self.n_owners:
                raise ValueError(f"owner {owner} outside 0..{self.n_owners - 1}")
            hit &= self.owners == int(owner)
        if fate is not None:
            hit &= self.fate == fate_code(fate)
        return np.flatnonzero(hit.any(axis=1))

    def text(self, names=None):
        """the table of by_owner as text, a line per side; names: the sides' names (default "0", "1", ...)"""
        rows = self.by_owner()
        names = [str(o) for o in range(self.n_owners)] if names is None else [str(v) for v in names]
        if len(names) != self.n_owners:
            raise ValueError(f"{len(names)} names for {self.n_owners} sides")
        wide = max([len(v) for v in names] + [4])
        out = f"{'side':<{wide}} {'seats':>7}" + "".join(f" {f:>8}" for f in FATES) + f" {'food':>8} {'length':>8} {'turns':>8}\n"
        for o, name in enumerate(names):
            out += (f"{name:<{wide}} {rows.seats[o]:>7d}" + "".join(f" {int(c):>8d}" for c in rows.fates[o])
                    + f" {rows.food[o]:>8d} {rows.length[o]:>8.2f} {rows.turns[o]:>8.1f}\n")
        return out


class _Pit:
    """what Arena and League share: the engine and the match's buffers, the recorder, and the one turn loop.  A subclass seats
    the sides by four hooks, each handed the `seat` its own match method made:
        _lists(L, seat)              -> (rows, pairs, games, read, over): rows[i] rows for the i-th greedy side, one after another
                                        in `pairs`; games: (o, slots, alive) for every searching side o that plays this turn;
                                        read: what the turn's one read-back brought; over: nothing is left
        _merge(L, seat, found, keep)    found[o]: the root moves of searching side o, or None; keep: some side is greedy
        _verdict(L, seat, turn)
        _result(seat, turns)         -> the match's result tuple; it has .lengths
        _owners(seat)                -> the owner of every seat, uint8[game_cnt][snake_cnt] on the host (asked for by a tally only)"""

    def __init__(self, height, width, snake_cnt, health_dec, game_cnt, seed):
        if seed is None:
            seed = int(np.random.randint(1 << 62))
        engine = Engine(game_cnt, height, width, snake_cnt, health_dec, 0.15, seed=seed)
        engine.reset()                            # start boards drawn on the device (Philox keyed by the seed and the game's uid)
        self._attach(engine)

    def _attach(self, engine):
        eng = self.engine = engine
        self.height, self.width, self.snake_cnt = eng.H, eng.W, eng.S
        self.health_dec, self.game_cnt = eng.health_dec, eng.n_slots
        self._fresh = True                        # the engine holds start boards no match has played on
        n, S = eng.n_slots, eng.S
        self._live = eng.new((n,), torch.uint8)
        self._pairs = eng.new((n * S, 2), torch.int32)
        self._moves = eng.new((n, S), torch.uint8)
        self._done = eng.new((n,), torch.uint8)
        self._rewards = eng.new((n, S), torch.int8)
        self._winner = eng.new((n,), torch.int32)
        self._length = eng.new((n,), torch.int32)
        self._roots = None                        # the searching turn's buffers, made by the first match that searches
        self._recorder = None                     # the Replay the next match fills
        self._tallier = None                      # the Tally the next match fills

    def record(self, games, first_turns=64):
        """games: distinct game indices in any order (an index out of range or given twice is a ValueError, before anything
        touches the device).  Returns the Replay the next match fills; the recorder is dropped when that match ends.
        first_turns: the turns the log on the device is first sized for (it doubles as the match goes on)."""
        self._recorder = Replay(games, self.height, self.width, self.game_cnt, first_turns)
        return self._recorder

    def tally(self):
        """the Tally the next match fills with every seat's fate; it is dropped when that match ends"""
        self._tallier = Tally(self.game_cnt, self.snake_cnt)
        return self._tallier

    @classmethod
    def from_engine(cls, engine):
        """a pit over the games an engine already holds (slots 0..n_slots-1), e.g. a game runner's"""
        self = cls.__new__(cls)
        self._attach(engine)
        return self

    def import_states(self, states):
        """start boards from the host (snk_game_state records), for parity runs"""
        self.engine.import_states(states)
        self._fresh = True

    def _play(self, sides, seat, init_tape, spawn_tape, counts_log=None):
        """one match of the checked `sides` -> the subclass's result.  init_tape: without one the match plays on the boards the
        pit holds -- fresh ones are drawn on the device when a match has already been played on them"""
        eng, n, S = self.engine, self.game_cnt, self.snake_cnt
        L = eng.L                                 # looked up now: a test may have put a recording proxy there
        live, moves = self._live, self._moves
        greedy = [side for side in sides if not isinstance(side, Searcher)]
        searching = len(greedy) < len(sides)
        rec, self._recorder = self._recorder, None        # held here only: a match that raises has dropped it too
        tal, self._tallier = self._tallier, None
        if init_tape is not None:
            eng.reset(init_tape=init_tape)
        elif not self._fresh:
            eng.reset()
        self._fresh = False
        live.fill_(1)
        self._winner.fill_(-1)
        self._length.zero_()
        if rec is not None:
            rec.begin(eng)
        if tal is not None:
            tal.begin(eng)
        turn = 0
        while True:
            rows, pairs, games, read, over = self._lists(L, seat)
            if over:
                break
            turn += 1
            if counts_log is not None:
                counts_log.append(read)
            if greedy:                            # with no row left it still fills the dense array with 1, for the merge
                m = sum(rows)
                q = mixed_values(eng, greedy, rows, pairs) if m else None
                check(L.snk_pit_moves(_ptr(q), _ptr(pairs), m, n, S, _ptr(moves), _stream()))
            if searching:
                found = [None] * len(sides)
                for o, slots, alive in games:     # team A's or owner 0's searcher first
                    G = int(slots.shape[0])
                    found[o] = sides[o].search(eng, slots, alive).contiguous()
                    if found[o].dtype != torch.uint8 or tuple(found[o].shape) != (G, S):
                        raise EngineError(f"search returned {found[o].dtype} {tuple(found[o].shape)} for {G} games of {S} snakes")
                    sides[o].end_of_turn()
                self._merge(L, seat, found, int(bool(greedy)))
            # the dense moves are in: open games move, games whose verdict is in stay as they are, then the turn's verdict
            tape = None
            if spawn_tape is not None:
                tape = torch.as_tensor(np.ascontiguousarray(spawn_tape(turn), np.int16), device=eng.device)
                if tape.numel() != n:
                    raise ValueError(f"spawn_tape({turn}) has {tape.numel()} entries for {n} games")
            if rec is not None:                   # the mid-tick snakes, from the records the step is about to change
                rec.before_step(eng, turn, live, moves)
            if tal is not None:                   # every seat's fate on this tick, from the same records
                tal.before_step(eng, turn, live, moves)
            check(L.snk_engine_step_active_tape(eng.h, _ptr(live), n, _ptr(moves), _ptr(tape), _ptr(self._done), None, _stream()))
            if rec is not None:                   # by the live flags the step saw: before the verdict clears them
                rec.after_step(eng, turn, live)
            check(L.snk_engine_rewards(eng.h, None, n, _ptr(self._rewards), _stream()))
            self._verdict(L, seat, turn)
        result = self._result(seat, turn)
        if rec is not None:
            rec.end(turn, result.lengths)         # the log's one copy, after the last turn
        if tal is not None:
            tal.end(self._owners(seat), len(sides), result.lengths)       # the tally's one copy
        return result


class Arena(_Pit):

    def __init__(self, height=11, width=11, snake_cnt=4, health_dec=1, game_cnt=1, seed=None):
        super().__init__(height, width, snake_cnt, health_dec, game_cnt, seed)

    def _attach(self, engine):
        super()._attach(engine)
        self._counts = engine.new((2,), torch.int32)
        self._scratch = engine.new((engine.L.snk_pit_scratch_elems(engine.n_slots),), torch.int32)

    # ---- one match -------------------------------------------------------------------------------------------------------
    def match(self, alice, bob, alice_snake_cnt=None, init_tape=None, spawn_tape=None):
        """alice, bob: anything with v_device(planes, mask) -> float32[rows][3] on the device (AlphaNNet: its guarded forward),
        a Searcher around one, or a Scripted; every combination is allowed.  With a Searcher the arena still reads back once per
        turn (G and the two row counts), the searches read back on their own.
        alice_snake_cnt: snakes 0 .. alice_snake_cnt-1 are alice's (default snake_cnt // 2, pit_mp_game_runner.py:17-18).
        init_tape: uint8[game_cnt][3][snake_cnt] recorded start draws (snk_engine_reset); without one the match plays on the
        boards the arena holds -- fresh ones are drawn on the device when a match has already been played on them.
        spawn_tape: callable turn -> int16[game_cnt] recorded food spawns (cell or -1), uploaded each turn.  For parity runs
        only: the upload is a copy from pageable host memory, which waits for the stream every turn -- host to device, so no
        read-back, but a match played with a tape says nothing about the speed of one played without."""
        eng, n, S = self.engine, self.game_cnt, self.snake_cnt
        a_cnt = S // 2 if alice_snake_cnt is None else int(alice_snake_cnt)
        if not 0 <= a_cnt <= S:
            raise ValueError(f"alice_snake_cnt {a_cnt} outside 0..{S}")
        for net in (alice, bob):
            if not isinstance(net, (Searcher, Scripted)) and not hasattr(net, "v_device"):
                raise TypeError(f"{type(net).__name__} has no v_device(planes, mask): the arena evaluates on the device only")
        greedy = [not isinstance(side, Searcher) for side in (alice, bob)]
        roots = None
        if not all(greedy):
            if self._roots is None:
                self._roots = (eng.new((n,), torch.int32), eng.new((n, S), torch.uint8), eng.new((n,), torch.int32),
                               eng.new((3,), torch.int32))
            roots = self._roots                   # slots, alive, rank, counts {nA, nB, G}
            roots[3].zero_()
        return self._play((alice, bob), (a_cnt, greedy, roots), init_tape, spawn_tape)

    def _lists(self, L, seat):
        eng, n, live, pairs = self.engine, self.game_cnt, self._live, self._pairs
        a_cnt, greedy, roots = seat
        counts = self._counts if roots is None else roots[3]
        if roots is not None:
            slots, alive, rank, _ = roots
            check(L.snk_pit_roots(eng.h, _ptr(live), n, _ptr(slots), _ptr(alive), _ptr(rank), _ptr(counts[2:]), _ptr(self._scratch),
                                  _stream()))
        if any(greedy):
            check(L.snk_pit_rows(eng.h, _ptr(live), n, a_cnt, _ptr(pairs), _ptr(counts), _ptr(self._scratch), _stream()))
        read = counts.tolist()                    # the turn's one read-back
        nA, nB = read[:2]
        rows = [cnt for cnt, g in zip((nA, nB), greedy) if g]
        lo = 0 if greedy[0] else nA               # team A's rows come first
        mine = pairs[lo:lo + sum(rows)]
        if roots is None:
            return rows, mine, [], read, nA + nB == 0
        G = read[2]                               # every searching side gets all open games
        return rows, mine, [(o, slots[:G], alive[:G]) for o in (0, 1) if not greedy[o]], read, G == 0

    def _merge(self, L, seat, found, keep):
        a_cnt, _, (_, alive, rank, _) = seat
        check(L.snk_pit_search_moves(_ptr(found[0]), _ptr(found[1]), _ptr(rank), _ptr(alive), self.game_cnt, self.snake_cnt, a_cnt,
                                     keep, _ptr(self._moves), _stream()))

    def _verdict(self, L, seat, turn):
        check(L.snk_pit_verdict(self.engine.h, _ptr(self._done), _ptr(self._rewards), self.game_cnt, seat[0], turn, _ptr(self._live),
                                _ptr(self._winner), _ptr(self._length), _stream()))

    def _result(self, seat, turns):
        a_cnt = seat[0]
        winners = self._winner.cpu().numpy()
        lengths = self._length.cpu().numpy()
        wins_a = int(((winners >= 0) & (winners < a_cnt)).sum())
        wins_b = int((winners >= a_cnt).sum())
        return ArenaResult(winners, lengths, turns, wins_a, wins_b, self.game_cnt - wins_a - wins_b)

    def _owners(self, seat):
        return np.repeat((np.arange(self.snake_cnt) >= seat[0]).astype(np.uint8)[None, :], self.game_cnt, axis=0)

    # ---- the reference's two judges ------------------------------------------------------------------------------------------
    @staticmethod
    def _sides(alice, bob, search, seed):
        """the two sides of one match: the nets themselves, or fresh Searchers around them (search: Searcher's keyword arguments);
        a Scripted stays as it is either way"""
        if search is None:
            return alice, bob
        seeds = [None, None] if seed is None else [seed + 101, seed + 202]
        return tuple(net if isinstance(net, Scripted) else Searcher(net, seed=sd, **search) for net, sd in zip((alice, bob), seeds))

    @staticmethod
    def test_pit(alice, bob, games=300, height=11, width=11, health_dec=1, seed=None, search=None):
        """test_pit.py:24-65: `games` games each of alice alone against three snakes of bob, the same with the roles swapped,
        then the duel of two snakes the reference prints as "2v2".  Returns the rates it prints:
        {"1v3_alice": (win rate, draw rate), "1v3_bob": (win rate, draw rate), "2v2": (alice's win rate, bob's win rate)}
        search=dict(breadth=..., depth=...): both nets move by search (a fresh Searcher each per match)"""
        seeds = [None] * 3 if seed is None else [seed, seed + 1, seed + 2]
        r1 = Arena(height, width, 4, health_dec, games, seeds[0]).match(*Arena._sides(alice, bob, search, seeds[0]), 1)
        r2 = Arena(height, width, 4, health_dec, games, seeds[1]).match(*Arena._sides(bob, alice, search, seeds[1]), 1)
        r3 = Arena(height, width, 2, health_dec, games, seeds[2]).match(*Arena._sides(alice, bob, search, seeds[2]), 1)
        return {"1v3_alice": (r1.wins_a / games, r1.draws / games), "1v3_bob": (r2.wins_a / games, r2.draws / games),
                "2v2": (r3.wins_a / games, r3.wins_b / games)}

    @staticmethod
    def ladder_row(challenger, champion, games=1000, height=11, width=11, seed=None, search=None):
        """pit.py:30-44: `games` games of two snakes, the champion's snake first; a drawn game is half a point for each side.
        Returns the challenger's score, the number pit.py writes to pit.txt (the title changes above 0.51, pit.py:45).
        search=dict(breadth=..., depth=...): both nets move by search"""
        r = Arena(height, width, 2, 1, games, seed).match(*Arena._sides(champion, challenger, search, seed), 1)
        won, lost = r.wins_b + 0.5 * r.draws, r.wins_a + 0.5 * r.draws
        return won / (won + lost)
