"""League: up to sixteen nets in ONE device pit match -- the arena's loop (snake_engine/arena.py, pit_mp_game_runner.py:14-63) with
the team split `id < Alice_snake_cnt` replaced by a table owner[game][seat] with values 0 .. K-1.

A turn of ``League.play``:

    snk_pit_rows_owned            (slot, snake id) of every alive snake of every open game, owner 0's rows first      (:23-35)
    the turn's read-back          the K row counts in one .tolist(): they size the net batches; total 0 ends the match
    snk_engine_observe            one launch over all rows                                                            (:28)
    nets[o].v_device              each owner with rows on its own slice, in owner order; an owner without rows is skipped (:34)
    snk_pit_moves                 greedy moves into the dense move array                                              (:36-38)
    snk_engine_step_active_tape   open games move, games whose verdict is in stay as they are                         (:42)
    snk_engine_rewards
    snk_pit_verdict_owned         a game is over when it is done or at most one owner has snakes left                 (:43-62)

With two nets and owner[g][s] = (s >= a_cnt) every launch and every batch is what ``Arena.match`` issues, so the winners, lengths
and turns are the same bit for bit.  What the table adds: a free-for-all in which every seat belongs to another net, and every
pairing of a round robin in lock step in one engine (``schedule``, ``round_robin``), scored by ``table`` and ``ratings``.

Any owner may instead be an ``arena.Searcher`` (``League.play_search``; ``play`` itself keeps refusing one): a searcher simulates
whole games, so each turn it gets the sub-list of open games in which it holds a seat -- a game that is open, with an alive snake
whose seat is the owner's -- and only its own seats take the moves it finds.  A turn of ``League.play_search``:

    snk_pit_roots_owned           per searching owner the open games it holds a seat in, the lists one after another in owner
                                  order, the alive rows of those games, and per seat the row of the list it reads
    snk_pit_rows_owned            only when some owner is greedy, over a second table made once per match: the searching owners'
                                  bytes out of range, the greedy owners renumbered densely, so their rows are contiguous
    the turn's read-back          the greedy row counts and the K game counts, one tensor, one .tolist(); all zeros ends the match
    the greedy owners             observe + each net on its own slice, one snk_pit_moves (the array is filled with 1)
    searcher.search, end_of_turn  in owner order, each on its own slice of the lists; an owner without a game is skipped for good
    snk_pit_search_moves_owned    merges the found moves into the dense move array
    step, rewards, verdict        as above

With two Searchers and the two-team table this is ``Arena.match`` with the same Searchers, and with no Searcher it is ``play``.
The league's own read-back stays one per turn; the searches read back on their own (snake_engine/arena.py).

An owner of either may be an ``arena.Scripted`` (the fixed yardstick of a table: the same opponent in every run): it counts as a
greedy owner, its slice of the row list is scored by snk_pit_script_values, and the observe launch and the nets run over the
other owners' rows only -- one observe per run of consecutive net owners.  A match without a ``Scripted`` issues exactly the
launches it issued before there was one.

``League.record(games)`` is ``Arena.record``: the Replay it returns is filled by the next ``play`` or ``play_search`` with the
boards of those games (snake_engine/replay.py) -- two more launches per turn, the read-back unchanged, one copy at the end.
"""
from collections import namedtuple

import numpy as np
import torch

from ._lib import check, EngineError
from .arena import Replay, Scripted, Searcher, mixed_values
from .engine import Engine, _ptr, _stream

MAX_OWNERS = 16          # SNK_PIT_MAX_OWNERS of include/snake_engine.h

LeagueResult = namedtuple("LeagueResult", "winners winner_owner lengths turns")
LeagueResult.__doc__ = """winners: int32[game_cnt] winning snake id, -1 for a draw (the reference's None); winner_owner: int32[game_cnt]
the owner of that seat, -1 for a draw; lengths: int32[game_cnt] the turn a game's verdict came in; turns: turns played"""

LeagueTable = namedtuple("LeagueTable", "wins draws games score")
LeagueTable.__doc__ = """wins: int64[K][K], wins[a][b] = games a won in which b held a seat; draws: int64[K][K], games without a winner
in which a and b both held a seat (symmetric); games: int64[K][K], games in which a and b both held a seat (symmetric; in a game
of two owners wins + wins.T + draws); score: float64[K] = (wins[a].sum() + draws[a].sum() / 2) / games[a].sum(), NaN for a net
that met nobody"""


class League:

    def __init__(self, height=11, width=11, snake_cnt=2, health_dec=1, game_cnt=1, seed=None):
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
        self._counts = eng.new((MAX_OWNERS,), torch.int32)
        self._scratch = eng.new((eng.L.snk_pit_owned_scratch_elems(n, MAX_OWNERS),), torch.int32)
        self._moves = eng.new((n, S), torch.uint8)
        self._done = eng.new((n,), torch.uint8)
        self._rewards = eng.new((n, S), torch.int8)
        self._winner = eng.new((n,), torch.int32)
        self._winner_owner = eng.new((n,), torch.int32)
        self._length = eng.new((n,), torch.int32)
        self._roots = None                        # the searching turn's buffers, made by the first match that searches
        self._recorder = None                     # the Replay the next match fills

    def record(self, games, first_turns=64):
        """Arena.record: distinct game indices in any order (out of range or twice: a ValueError before anything touches the
        device) -> the Replay the next play / play_search fills; the recorder is dropped when that match ends"""
        self._recorder = Replay(games, self.height, self.width, self.game_cnt, first_turns)
        return self._recorder

    @classmethod
    def from_engine(cls, engine):
        """a league over the games an engine already holds (slots 0..n_slots-1)"""
        self = cls.__new__(cls)
        self._attach(engine)
        return self

    def import_states(self, states):
        """start boards from the host (snk_game_state records), for parity runs"""
        self.engine.import_states(states)
        self._fresh = True

    def _owner_table(self, nets, owner, searchers=False):
        """the checked table as uint8[game_cnt][snake_cnt] on the host"""
        n, S = self.game_cnt, self.snake_cnt
        if not 1 <= len(nets) <= MAX_OWNERS:
            raise ValueError(f"{len(nets)} nets: a league match takes 1..{MAX_OWNERS}")
        for net in nets:
            if isinstance(net, Scripted):
                continue
            if isinstance(net, Searcher):
                if searchers:
                    continue
                raise TypeError("a Searcher cannot sit in League.play: it simulates whole games (use League.play_search)")
            if not hasattr(net, "v_device"):
                raise TypeError(f"{type(net).__name__} has no v_device(planes, mask): the league evaluates on the device only")
        owner = np.asarray(owner)
        if owner.shape != (n, S) or owner.dtype.kind not in "iu":
            raise ValueError(f"owner table {owner.dtype} {owner.shape}: an integer array [{n}][{S}] expected")
        if owner.size and (owner.min() < 0 or owner.max() >= len(nets)):
            raise ValueError(f"owner values {int(owner.min())}..{int(owner.max())} outside 0..{len(nets) - 1}")
        return np.ascontiguousarray(owner, np.uint8)

    # ---- one match -------------------------------------------------------------------------------------------------------
    def play(self, nets, owner, init_tape=None, spawn_tape=None, counts_log=None):
        """nets: 1..16 objects with v_device(planes, mask) -> float32[rows][3] on the device (or Scripted); owner: integer array
        [game_cnt][snake_cnt] on the host, owner[g][s] = the index in nets of the net that moves snake s of game g.
        init_tape / spawn_tape: as in Arena.match (recorded start draws; callable turn -> int16[game_cnt] recorded food spawns,
        for parity runs only).  counts_log: a list that receives the K row counts of every turn (what the turn's read-back
        brought, no further copy)."""
        eng, n, S = self.engine, self.game_cnt, self.snake_cnt
        nets = list(nets)
        K = len(nets)
        d_owner = torch.as_tensor(self._owner_table(nets, owner), device=eng.device)
        if init_tape is not None:
            eng.reset(init_tape=init_tape)
        elif not self._fresh:
            eng.reset()
        self._fresh = False
        self._live.fill_(1)
        self._winner.fill_(-1)
        self._winner_owner.fill_(-1)
        self._length.zero_()
        rec, self._recorder = self._recorder, None
        if rec is not None:
            rec.begin(eng)
        L = eng.L
        live, pairs, moves = self._live, self._pairs, self._moves
        counts = self._counts[:K]
        scripted = any(isinstance(net, Scripted) for net in nets)
        turn = 0
        while True:
            check(L.snk_pit_rows_owned(eng.h, _ptr(live), n, _ptr(d_owner), K, _ptr(pairs), _ptr(counts), _ptr(self._scratch),
                                       _stream()))
            rows = counts.tolist()                # the turn's one read-back
            m = sum(rows)
            if m == 0:
                break
            turn += 1
            if counts_log is not None:
                counts_log.append(rows)
            if scripted:                          # the kernel scores the scripted rows; observe and nets on the others' only
                q = mixed_values(eng, nets, rows, pairs)
            else:
                planes, mask, _ = eng.observe_all(pairs[:m], want_key=False)
                q = self._values(nets, rows, planes, mask)
            check(L.snk_pit_moves(_ptr(q), _ptr(pairs), m, n, S, _ptr(moves), _stream()))
            tape = None
            if spawn_tape is not None:
                tape = torch.as_tensor(np.ascontiguousarray(spawn_tape(turn), np.int16), device=eng.device)
                if tape.numel() != n:
                    raise ValueError(f"spawn_tape({turn}) has {tape.numel()} entries for {n} games")
            if rec is not None:                   # the mid-tick snakes, from the records the step is about to change
                rec.before_step(eng, turn, live, moves)
            check(L.snk_engine_step_active_tape(eng.h, _ptr(live), n, _ptr(moves), _ptr(tape), _ptr(self._done), None, _stream()))
            if rec is not None:                   # by the live flags the step saw: before the verdict clears them
                rec.after_step(eng, turn, live)
            check(L.snk_engine_rewards(eng.h, None, n, _ptr(self._rewards), _stream()))
            check(L.snk_pit_verdict_owned(eng.h, _ptr(self._done), _ptr(self._rewards), n, _ptr(d_owner), K, turn, _ptr(live),
                                          _ptr(self._winner), _ptr(self._winner_owner), _ptr(self._length), _stream()))
        result = LeagueResult(self._winner.cpu().numpy(), self._winner_owner.cpu().numpy(), self._length.cpu().numpy(), turn)
        if rec is not None:
            rec.end(turn, result.lengths)         # the log's one copy, after the last turn
        return result

    def play_search(self, sides, owner, init_tape=None, spawn_tape=None, counts_log=None):
        """play with any owner moving by search: sides[o] is a net with v_device, a Scripted or a Searcher around a net, in any
        mix (1..16 owners); owner, init_tape and spawn_tape as in play.  The same Searcher object twice is a ValueError: it owns one
        transposition table, aged once a turn.  counts_log: a list that receives the whole read-back of every turn -- the row
        counts of the greedy owners in owner order, then the K counts of games per owner (0 for a greedy owner); without a Searcher
        the K row counts alone, as in play."""
        eng, n, S = self.engine, self.game_cnt, self.snake_cnt
        sides = list(sides)
        K = len(sides)
        table = self._owner_table(sides, owner, searchers=True)
        searching = [isinstance(side, Searcher) for side in sides]
        if len({id(side) for side, s in zip(sides, searching) if s}) != sum(searching):
            raise ValueError("the same Searcher sits twice: it owns one transposition table, aged once a turn (wrap the net twice)")
        search_mask = sum(1 << o for o in range(K) if searching[o])
        greedy = [side for side, s in zip(sides, searching) if not s]
        Kg = len(greedy)
        scripted = any(isinstance(side, Scripted) for side in greedy)
        d_owner = torch.as_tensor(table, device=eng.device)
        d_greedy = None
        if Kg:                                    # the greedy owners' table: searching owners out of range, the others 0..Kg-1
            dense = np.full(256, 255, np.uint8)
            dense[[o for o in range(K) if not searching[o]]] = np.arange(Kg, dtype=np.uint8)
            d_greedy = torch.as_tensor(dense[table], device=eng.device)
        if search_mask and self._roots is None:
            self._roots = (eng.new((n * S,), torch.int32), eng.new((n * S, S), torch.uint8), eng.new((n, S), torch.int32),
                           eng.new((2 * MAX_OWNERS,), torch.int32))
        if init_tape is not None:
            eng.reset(init_tape=init_tape)
        elif not self._fresh:
            eng.reset()
        self._fresh = False
        self._live.fill_(1)
        self._winner.fill_(-1)
        self._winner_owner.fill_(-1)
        self._length.zero_()
        rec, self._recorder = self._recorder, None
        if rec is not None:
            rec.begin(eng)
        L = eng.L
        live, pairs, moves = self._live, self._pairs, self._moves
        if search_mask:
            slots, alive, rank, counts = self._roots
            counts = counts[:Kg + K]              # {the greedy owners' rows, every owner's games}
            counts.zero_()
        else:
            counts = self._counts[:K]             # no searcher: the turn of play
        turn = 0
        while True:
            if search_mask:
                check(L.snk_pit_roots_owned(eng.h, _ptr(live), n, _ptr(d_owner), K, search_mask, _ptr(counts[Kg:]), _ptr(slots),
                                            _ptr(alive), _ptr(rank), _ptr(self._scratch), _stream()))
            if Kg:
                check(L.snk_pit_rows_owned(eng.h, _ptr(live), n, _ptr(d_greedy), Kg, _ptr(pairs), _ptr(counts), _ptr(self._scratch),
                                           _stream()))
            read = counts.tolist()                # the turn's one read-back
            if not any(read):
                break
            turn += 1
            if counts_log is not None:
                counts_log.append(read)
            if Kg:                                # the greedy owners' nets on their own rows; the array is filled with 1
                rows = read[:Kg]
                m, q = sum(rows), None
                if m and scripted:
                    q = mixed_values(eng, greedy, rows, pairs)
                elif m:
                    planes, mask, _ = eng.observe_all(pairs[:m], want_key=False)
                    q = self._values(greedy, rows, planes, mask)
                check(L.snk_pit_moves(_ptr(q), _ptr(pairs), m, n, S, _ptr(moves), _stream()))
            if search_mask:
                found, lo = [], 0
                for o in range(K):                # in owner order, each on its own slice of the lists
                    G = read[Kg + o]
                    if G == 0:                    # a greedy owner, or a searcher that has left every game (for good)
                        continue
                    f = sides[o].search(eng, slots[lo:lo + G], alive[lo:lo + G]).contiguous()
                    if f.dtype != torch.uint8 or tuple(f.shape) != (G, S):
                        raise EngineError(f"search returned {f.dtype} {tuple(f.shape)} for {G} games of {S} snakes")
                    sides[o].end_of_turn()
                    found.append(f)
                    lo += G
                d_found = None if not found else found[0] if len(found) == 1 else torch.cat(found)
                check(L.snk_pit_search_moves_owned(_ptr(d_found), _ptr(rank), n, S, lo, int(Kg > 0), _ptr(moves), _stream()))
            tape = None
            if spawn_tape is not None:
                tape = torch.as_tensor(np.ascontiguousarray(spawn_tape(turn), np.int16), device=eng.device)
                if tape.numel() != n:
                    raise ValueError(f"spawn_tape({turn}) has {tape.numel()} entries for {n} games")
            if rec is not None:                   # the mid-tick snakes, from the records the step is about to change
                rec.before_step(eng, turn, live, moves)
            check(L.snk_engine_step_active_tape(eng.h, _ptr(live), n, _ptr(moves), _ptr(tape), _ptr(self._done), None, _stream()))
            if rec is not None:                   # by the live flags the step saw: before the verdict clears them
                rec.after_step(eng, turn, live)
            check(L.snk_engine_rewards(eng.h, None, n, _ptr(self._rewards), _stream()))
            check(L.snk_pit_verdict_owned(eng.h, _ptr(self._done), _ptr(self._rewards), n, _ptr(d_owner), K, turn, _ptr(live),
                                          _ptr(self._winner), _ptr(self._winner_owner), _ptr(self._length), _stream()))
        result = LeagueResult(self._winner.cpu().numpy(), self._winner_owner.cpu().numpy(), self._length.cpu().numpy(), turn)
        if rec is not None:
            rec.end(turn, result.lengths)         # the log's one copy, after the last turn
        return result

    @staticmethod
    def _values(nets, rows, planes, mask):
        """every net with rows on its own slice, in owner order: float32[m][3]"""
        parts, lo = [], 0
        for net, cnt in zip(nets, rows):
            if cnt:
                parts.append(net.v_device(planes[lo:lo + cnt], mask[lo:lo + cnt]))
                lo += cnt
        q = parts[0] if len(parts) == 1 else torch.cat(parts)
        if q.dtype != torch.float32 or tuple(q.shape) != (lo, 3) or not q.is_cuda:
            raise EngineError(f"v_device returned {q.dtype} {tuple(q.shape)} on {q.device} for {lo} rows: float32 [rows][3] on the device expected")
        return q.contiguous()


# ---- who sits where --------------------------------------------------------------------------------------------------------
SEATS = {"duel": 2, "1v3": 4, "ffa": 4}


def schedule(n_nets, games, seats="duel"):
    """the owner table uint8[n_games][seats] of a round robin among n_nets nets, `games` consecutive games per line-up:
    "duel" (2 seats): every ordered pair (i, j), i != j, in lexicographic order, owner [i, j] (the first seat is snake 0);
    "1v3"  (4 seats): the same pairs, owner [i, j, j, j] (test_pit.py:24-50: one snake of i against three of j);
    "ffa"  (4 seats, at least 4 nets): every ascending 4-combination, its four cyclic rotations one after another."""
    n_nets, games = int(n_nets), int(games)
    if seats not in SEATS:
        raise ValueError(f"seats {seats!r}: one of {sorted(SEATS)}")
    if not 1 <= n_nets <= MAX_OWNERS or games < 1:
        raise ValueError(f"schedule({n_nets}, {games}): 1..{MAX_OWNERS} nets and at least one game expected")
    lines = []
    if seats == "ffa":
        if n_nets < 4:
            raise ValueError(f"a free-for-all needs at least 4 nets, not {n_nets}")
        for a in range(n_nets):
            for b in range(a + 1, n_nets):
                for c in range(b + 1, n_nets):
                    for d in range(c + 1, n_nets):
                        combo = [a, b, c, d]
                        lines += [combo[r:] + combo[:r] for r in range(4)]
    else:
        for i in range(n_nets):
            for j in range(n_nets):
                if i != j:
                    lines.append([i, j] if seats == "duel" else [i, j, j, j])
    return np.repeat(np.array(lines, np.uint8).reshape(-1, SEATS[seats]), games, axis=0)


def table(result, owner, n_nets):
    """the cross table of a played schedule.  A game with the distinct owners O and a winner whose owner is w: wins[w][o] += 1
    for every other o of O; without a winner: draws[a][b] += 1 for every two members of O; games[a][b] += 1 for every two
    members either way.  For a duel score[] is the number pit.py writes (challenger_score, pit.py:37-45)."""
    owner = np.asarray(owner).astype(np.int64)
    wo = np.asarray(result.winner_owner).astype(np.int64)
    K = int(n_nets)
    if owner.ndim != 2 or wo.shape != (owner.shape[0],):
        raise ValueError(f"owner table {owner.shape} against {wo.shape} results")
    if owner.size and (owner.min() < 0 or owner.max() >= K or wo.max() >= K):
        raise ValueError(f"owner values outside 0..{K - 1}")
    present = np.zeros((owner.shape[0], K), np.int64)
    present[np.arange(owner.shape[0])[:, None], owner] = 1
    if not (present[wo >= 0, wo[wo >= 0]] == 1).all():
        raise ValueError("a winner's owner holds no seat of its game")
    met = present.T @ present
    drawn = present[wo < 0]
    won = np.zeros_like(present)
    won[wo >= 0, wo[wo >= 0]] = 1
    wins, draws = won.T @ present, drawn.T @ drawn
    for m in (met, wins, draws):
        np.fill_diagonal(m, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        score = (wins.sum(1) + 0.5 * draws.sum(1)) / met.sum(1)
    return LeagueTable(wins, draws, met, score)


def ratings(wins, draws, iterations=200):
    """Elo-scaled Bradley-Terry strengths float64[K], net 0 at 0.  A drawn game counts half a win each way and one virtual drawn
    game is added between every two nets, so a net without a point keeps a finite rating.  `iterations` minorise-maximise steps
    from equal strengths (Hunter 2004): p_i <- W_i / sum_j n_ij / (p_i + p_j).  Two nets: 400 log10((w + d/2 + 1/2) / (l + d/2 + 1/2))."""
    w = np.asarray(wins, np.float64) + 0.5 * np.asarray(draws, np.float64) + 0.5
    np.fill_diagonal(w, 0.0)
    K = w.shape[0]
    if K == 1:
        return np.zeros(1)
    n, W = w + w.T, w.sum(1)
    p = np.ones(K)
    for _ in range(int(iterations)):
        p = W / (n / (p[:, None] + p[None, :])).sum(1)
        p /= np.exp(np.log(p).mean())
    r = 400.0 * np.log10(p)
    return r - r[0]


def searchers(nets, search, seed=None):
    """a fresh Searcher around every net (search: Searcher's keyword arguments), as Arena._sides makes them; with a seed net o
    searches with seed + 101 * (o + 1).  A Scripted stays as it is."""
    return [net if isinstance(net, Scripted) else Searcher(net, seed=None if seed is None else seed + 101 * (o + 1), **search)
            for o, net in enumerate(nets)]


def round_robin(nets, games=300, seats="duel", height=11, width=11, health_dec=1, seed=None, search=None):
    """every line-up of schedule(len(nets), games, seats) in lock step in one engine -> (LeagueTable, ratings)
    search=dict(breadth=..., depth=...): every net moves by search (a fresh Searcher each, League.play_search).
    Any entry of nets may be a Scripted: it moves by its script with or without search="""
    nets = list(nets)
    owner = schedule(len(nets), games, seats)
    league = League(height, width, SEATS[seats], health_dec, len(owner), seed)
    if search is None:
        result = league.play(nets, owner)
    else:
        result = league.play_search(searchers(nets, search, seed), owner)
    t = table(result, owner, len(nets))
    return t, ratings(t.wins, t.draws)
