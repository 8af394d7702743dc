"""League: up to sixteen sides in ONE device pit match -- the pit's turn (snake_engine/arena.py states it, once; pit_mp_game_runner.py:
14-63) with the team split `id < Alice_snake_cnt` replaced by a table owner[game][seat] with values 0 .. K-1.  What the table
changes is the seating, the three hooks the turn loop calls:

    _lists    snk_pit_rows_owned: the row list bucketed by owner, owner 0's rows first, and the K row counts -- the read-back of
              ``play``; a total of 0 ends the match.  With a Searcher (``play_search``; ``play`` itself keeps refusing one) first
              snk_pit_roots_owned: a searcher simulates whole games, so each turn it gets the open games in which it holds a seat
              with an alive snake -- the lists one after another in owner order, the alive rows of those games, and per seat
              the row of the list it reads.  Then snk_pit_rows_owned only when some owner is greedy, over a second table made once
              per match: the searching owners' bytes out of range, the greedy owners renumbered densely, so their rows are
              contiguous.  The read-back is the greedy row counts, then the K game counts (0 for a greedy owner); all zeros ends
              the match, and a searcher without a game is skipped, for good
    _merge    snk_pit_search_moves_owned: the found moves, one array in owner order, into the dense move array by list row
    _verdict  snk_pit_verdict_owned: a game is over when it is done or at most one owner has snakes left; the winner's owner
              beside the winner
    _owners   the table itself: ``tally()`` (arena.py) counts every seat's fate, and ``Tally.by_owner`` has a row per owner

With two sides and owner[g][s] = (s >= a_cnt) every launch and every batch is what ``Arena.match`` issues, with or without
Searchers, so the winners, lengths and turns are the same bit for bit; without a Searcher ``play_search`` is ``play``.  What the
table adds: a free-for-all in which every seat belongs to another net, and every pairing of a round robin in lock step in one
engine (``schedule``, ``round_robin``), scored by ``table`` and ``ratings``.  An ``arena.Scripted`` owner is the fixed yardstick
of such a table: the same opponent in every run.
"""
from collections import namedtuple

import numpy as np
import torch

from ._lib import check
from .arena import _Pit, Scripted, Searcher
from .engine import _ptr, _stream

MAX_OWNERS = 16          # SNK_PIT_MAX_OWNERS of include/snake_engine.h

LeagueResult = namedtuple("LeagueResult", "winners winner_owner lengths turns")
LeagueResult.__doc__ = """winners: int32[game_cnt] winning snake id, -1 for a draw (the reference's None); winner_owner: int32[game_cnt]
the owner of that seat, -1 for a draw; lengths: int32[game_cnt] the turn a game's verdict came in; turns: turns played"""

LeagueTable = namedtuple("LeagueTable", "wins draws games score")
LeagueTable.__doc__ = """wins: int64[K][K], wins[a][b] = games a won in which b held a seat; draws: int64[K][K], games without a winner
in which a and b both held a seat (symmetric); games: int64[K][K], games in which a and b both held a seat (symmetric; in a game
of two owners wins + wins.T + draws); score: float64[K] = (wins[a].sum() + draws[a].sum() / 2) / games[a].sum(), NaN for a net
that met nobody"""


class League(_Pit):

    def __init__(self, height=11, width=11, snake_cnt=2, health_dec=1, game_cnt=1, seed=None):
        super().__init__(height, width, snake_cnt, health_dec, game_cnt, seed)

    def _attach(self, engine):
        super()._attach(engine)
        n = engine.n_slots
        self._counts = engine.new((MAX_OWNERS,), torch.int32)
        self._scratch = engine.new((engine.L.snk_pit_owned_scratch_elems(n, MAX_OWNERS),), torch.int32)
        self._winner_owner = engine.new((n,), torch.int32)

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
        return self._seated(nets, owner, False, init_tape, spawn_tape, counts_log)

    def play_search(self, sides, owner, init_tape=None, spawn_tape=None, counts_log=None):
        """play with any owner moving by search: sides[o] is a net with v_device, a Scripted or a Searcher around a net, in any
        mix (1..16 owners); owner, init_tape and spawn_tape as in play.  The same Searcher object twice is a ValueError: it owns one
        transposition table, aged once a turn.  counts_log: a list that receives the whole read-back of every turn -- the row
        counts of the greedy owners in owner order, then the K counts of games per owner (0 for a greedy owner); without a Searcher
        the K row counts alone, as in play."""
        return self._seated(sides, owner, True, init_tape, spawn_tape, counts_log)

    def _seated(self, sides, owner, searchers, init_tape, spawn_tape, counts_log):
        """the checks, which come before anything touches the device, and the match's seat"""
        eng, n, S = self.engine, self.game_cnt, self.snake_cnt
        sides = list(sides)
        K = len(sides)
        table = self._owner_table(sides, owner, searchers)
        searching = [isinstance(side, Searcher) for side in sides]
        if len({id(side) for side, s in zip(sides, searching) if s}) != sum(searching):
            raise ValueError("the same Searcher sits twice: it owns one transposition table, aged once a turn (wrap the net twice)")
        search_mask = sum(1 << o for o in range(K) if searching[o])
        Kg = K - sum(searching)
        d_greedy = d_owner = torch.as_tensor(table, device=eng.device)
        if 0 < Kg < K:                            # the greedy owners' table: searching owners out of range, the others 0..Kg-1
            dense = np.full(256, 255, np.uint8)
            dense[[o for o in range(K) if not searching[o]]] = np.arange(Kg, dtype=np.uint8)
            d_greedy = torch.as_tensor(dense[table], device=eng.device)
        if search_mask:
            if self._roots is None:
                self._roots = (eng.new((n * S,), torch.int32), eng.new((n * S, S), torch.uint8), eng.new((n, S), torch.int32),
                               eng.new((2 * MAX_OWNERS,), torch.int32))
            counts = self._roots[3][:Kg + K]      # {the greedy owners' rows, every owner's games}
            counts.zero_()
        else:
            counts = self._counts[:K]             # no searcher: the K row counts
        self._winner_owner.fill_(-1)
        return self._play(sides, (d_owner, K, d_greedy, Kg, search_mask, counts, table), init_tape, spawn_tape, counts_log)

    def _lists(self, L, seat):
        eng, n, live, pairs = self.engine, self.game_cnt, self._live, self._pairs
        d_owner, K, d_greedy, Kg, search_mask, counts, _ = seat
        if search_mask:
            slots, alive, rank, _ = self._roots
            check(L.snk_pit_roots_owned(eng.h, _ptr(live), n, _ptr(d_owner), K, search_mask, _ptr(counts[Kg:]), _ptr(slots),
                                        _ptr(alive), _ptr(rank), _ptr(self._scratch), _stream()))
        if Kg:
            check(L.snk_pit_rows_owned(eng.h, _ptr(live), n, _ptr(d_greedy), Kg, _ptr(pairs), _ptr(counts), _ptr(self._scratch),
                                       _stream()))
        read = counts.tolist()                    # the turn's one read-back
        games, lo = [], 0
        for o, G in enumerate(read[Kg:] if search_mask else ()):
            if G:                                 # 0: a greedy owner, or a searcher that has left every game (for good)
                games.append((o, slots[lo:lo + G], alive[lo:lo + G]))
                lo += G
        return read[:Kg], pairs[:sum(read[:Kg])], games, read, not any(read)

    def _merge(self, L, seat, found, keep):
        found = [f for f in found if f is not None]
        d_found = None if not found else found[0] if len(found) == 1 else torch.cat(found)
        check(L.snk_pit_search_moves_owned(_ptr(d_found), _ptr(self._roots[2]), self.game_cnt, self.snake_cnt,
                                           sum(int(f.shape[0]) for f in found), keep, _ptr(self._moves), _stream()))

    def _verdict(self, L, seat, turn):
        check(L.snk_pit_verdict_owned(self.engine.h, _ptr(self._done), _ptr(self._rewards), self.game_cnt, _ptr(seat[0]), seat[1], turn,
                                      _ptr(self._live), _ptr(self._winner), _ptr(self._winner_owner), _ptr(self._length), _stream()))

    def _owners(self, seat):
        return seat[6]                            # the checked table, still on the host

    def _result(self, seat, turns):
        return LeagueResult(self._winner.cpu().numpy(), self._winner_owner.cpu().numpy(), self._length.cpu().numpy(), turns)


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
