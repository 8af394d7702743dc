"""Arena: whole pit matches on the device -- the reference's pit loop (pit_mp_game_runner.py:14-63) with two greedy agents
(pit_agent.py:10-28) as a fixed sequence of launches per turn and ONE host read-back per turn.

A turn of ``Arena.match``:

    snk_pit_rows                  (slot, snake id) of every alive snake of every open game, team A first   (:23-35)
    the turn's read-back          the two row counts: they size the two net batches
    snk_engine_observe            one launch over the rows                                                 (:28)
    alice.v_device / bob.v_device rows [0, nA) and [nA, nA + nB)                                           (:34)
    snk_pit_moves                 greedy moves into the dense move array                                   (:36-38)
    snk_engine_step_active_tape   open games move, games whose verdict is in stay as they are              (:42)
    snk_engine_rewards
    snk_pit_verdict               winners, game lengths, the open flags                                    (:43-62)

There is no per-game Python loop and nothing else comes back to the host until the match is over.  The host loop of
``utils.pit_mp_game_runner.MPGameRunner.run`` (four synchronising copies, ``np.nonzero`` and a Python loop over the games each
turn) stays as the parity-pinned form; ``MPGameRunner.run_device`` is this one behind the same interface.
"""
from collections import namedtuple

import numpy as np
import torch

from ._lib import check, EngineError
from .engine import Engine, _ptr, _stream

ArenaResult = namedtuple("ArenaResult", "winners lengths turns wins_a wins_b draws")
ArenaResult.__doc__ = """winners: int32[game_cnt] winning snake id, -1 for a draw (the reference's None); lengths: int32[game_cnt]
the turn a game's verdict came in; turns: turns played; wins_a / wins_b: games won by a snake of team A (id < alice_snake_cnt) /
team B; draws: games without a winner"""


class Arena:

    def __init__(self, height=11, width=11, snake_cnt=4, health_dec=1, game_cnt=1, seed=None):
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
        self._counts = eng.new((2,), torch.int32)
        self._scratch = eng.new((eng.L.snk_pit_scratch_elems(n),), torch.int32)
        self._moves = eng.new((n, S), torch.uint8)
        self._done = eng.new((n,), torch.uint8)
        self._rewards = eng.new((n, S), torch.int8)
        self._winner = eng.new((n,), torch.int32)
        self._length = eng.new((n,), torch.int32)

    @classmethod
    def from_engine(cls, engine):
        """an arena over the games an engine already holds (slots 0..n_slots-1), e.g. a game runner's"""
        self = cls.__new__(cls)
        self._attach(engine)
        return self

    def import_states(self, states):
        """start boards from the host (snk_game_state records), for parity runs"""
        self.engine.import_states(states)
        self._fresh = True

    # ---- one match -------------------------------------------------------------------------------------------------------
    def match(self, alice, bob, alice_snake_cnt=None, init_tape=None, spawn_tape=None):
        """alice, bob: anything with v_device(planes, mask) -> float32[rows][3] on the device (AlphaNNet: its guarded forward).
        alice_snake_cnt: snakes 0 .. alice_snake_cnt-1 are alice's (default snake_cnt // 2, pit_mp_game_runner.py:17-18).
        init_tape: uint8[game_cnt][3][snake_cnt] recorded start draws (snk_engine_reset); without one the match plays on the
        boards the arena holds -- fresh ones are drawn on the device when a match has already been played on them.
        spawn_tape: callable turn -> int16[game_cnt] recorded food spawns (cell or -1), uploaded each turn.  For parity runs
        only: the upload is a copy from pageable host memory, which waits for the stream every turn -- host to device, so no
        read-back, but a match played with a tape says nothing about the speed of one played without."""
        eng, n, S = self.engine, self.game_cnt, self.snake_cnt
        L = eng.L
        a_cnt = S // 2 if alice_snake_cnt is None else int(alice_snake_cnt)
        if not 0 <= a_cnt <= S:
            raise ValueError(f"alice_snake_cnt {a_cnt} outside 0..{S}")
        for net in (alice, bob):
            if not hasattr(net, "v_device"):
                raise TypeError(f"{type(net).__name__} has no v_device(planes, mask): the arena evaluates on the device only")
        if init_tape is not None:
            eng.reset(init_tape=init_tape)
        elif not self._fresh:
            eng.reset()
        self._fresh = False
        live, pairs, counts, moves = self._live, self._pairs, self._counts, self._moves
        live.fill_(1)
        self._winner.fill_(-1)
        self._length.zero_()
        turn = 0
        while True:
            check(L.snk_pit_rows(eng.h, _ptr(live), n, a_cnt, _ptr(pairs), _ptr(counts), _ptr(self._scratch), _stream()))
            nA, nB = counts.tolist()              # the turn's one read-back
            m = nA + nB
            if m == 0:
                break
            turn += 1
            planes, mask, _ = eng.observe_all(pairs[:m], want_key=False)
            q = self._values(alice, bob, planes, mask, nA, m)
            check(L.snk_pit_moves(_ptr(q), _ptr(pairs), m, n, S, _ptr(moves), _stream()))
            tape = None
            if spawn_tape is not None:
                tape = torch.as_tensor(np.ascontiguousarray(spawn_tape(turn), np.int16), device=eng.device)
                if tape.numel() != n:
                    raise ValueError(f"spawn_tape({turn}) has {tape.numel()} entries for {n} games")
            check(L.snk_engine_step_active_tape(eng.h, _ptr(live), n, _ptr(moves), _ptr(tape), _ptr(self._done), None, _stream()))
            check(L.snk_engine_rewards(eng.h, None, n, _ptr(self._rewards), _stream()))
            check(L.snk_pit_verdict(eng.h, _ptr(self._done), _ptr(self._rewards), n, a_cnt, turn, _ptr(live), _ptr(self._winner),
                                    _ptr(self._length), _stream()))
        winners = self._winner.cpu().numpy()
        lengths = self._length.cpu().numpy()
        wins_a = int(((winners >= 0) & (winners < a_cnt)).sum())
        wins_b = int((winners >= a_cnt).sum())
        return ArenaResult(winners, lengths, turn, wins_a, wins_b, n - wins_a - wins_b)

    @staticmethod
    def _values(alice, bob, planes, mask, nA, m):
        """the two nets on their rows: float32[m][3], team A's rows first"""
        parts = []
        if nA:
            parts.append(alice.v_device(planes[:nA], mask[:nA]))
        if m > nA:
            parts.append(bob.v_device(planes[nA:m], mask[nA:m]))
        q = parts[0] if len(parts) == 1 else torch.cat(parts)
        if q.dtype != torch.float32 or tuple(q.shape) != (m, 3) or not q.is_cuda:
            raise EngineError(f"v_device returned {q.dtype} {tuple(q.shape)} on {q.device} for {m} rows: float32 [rows][3] on the device expected")
        return q.contiguous()

    # ---- the reference's two judges ------------------------------------------------------------------------------------------
    @staticmethod
    def test_pit(alice, bob, games=300, height=11, width=11, health_dec=1, seed=None):
        """test_pit.py:24-65: `games` games each of alice alone against three snakes of bob, the same with the roles swapped,
        then the duel of two snakes the reference prints as "2v2".  Returns the rates it prints:
        {"1v3_alice": (win rate, draw rate), "1v3_bob": (win rate, draw rate), "2v2": (alice's win rate, bob's win rate)}"""
        seeds = [None] * 3 if seed is None else [seed, seed + 1, seed + 2]
        r1 = Arena(height, width, 4, health_dec, games, seeds[0]).match(alice, bob, 1)
        r2 = Arena(height, width, 4, health_dec, games, seeds[1]).match(bob, alice, 1)
        r3 = Arena(height, width, 2, health_dec, games, seeds[2]).match(alice, bob, 1)
        return {"1v3_alice": (r1.wins_a / games, r1.draws / games), "1v3_bob": (r2.wins_a / games, r2.draws / games),
                "2v2": (r3.wins_a / games, r3.wins_b / games)}

    @staticmethod
    def ladder_row(challenger, champion, games=1000, height=11, width=11, seed=None):
        """pit.py:30-44: `games` games of two snakes, the champion's snake first; a drawn game is half a point for each side.
        Returns the challenger's score, the number pit.py writes to pit.txt (the title changes above 0.51, pit.py:45)"""
        r = Arena(height, width, 2, 1, games, seed).match(champion, challenger, 1)
        won, lost = r.wins_b + 0.5 * r.draws, r.wins_a + 0.5 * r.draws
        return won / (won + lost)
