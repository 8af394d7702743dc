"""Test infrastructure: the CPU statement of a pit match in which a side may move by search, composed from what oracle/ offers
and written from oracle.pit_oracle.pit_run's loop (pit_mp_game_runner.py:14-63).  A searching team is one
oracle.mcts_oracle.SelfPlayOracle(net, base, training=False, depth, breadth, draws) kept over the match (its caches age from
turn to turn as Agent's do, agent.py:30-31, 101-110); each turn its root_turn(open games) simulates all snakes with the team's
net and the team takes its own snakes' moves (Agent.make_moves, agent.py:25-99).  A greedy team takes argmaxs(net.v(states))
(pit_agent.py:10-13).  The merge by snake id, Game.tic(dense, draws=...) with last_spawn logged and the verdict follow pit_run.

The device search sums in another order and calls another libm than NumPy (root Q within 1e-5 of the oracle's, tests/test_mcts_gpu.py),
so a match can only be compared move for move where no decision hangs on the last bits.  The helper measures that on its own side:
  q_gap   the smallest difference between the two largest Q of a row at any root decision a searching team took (> Q_GAP wanted)
  u_edge  the smallest distance of a rollout uniform from an edge of the cdf it was drawn against, over both teams (> U_EDGE wanted)
CASES lists the configurations the GPU test plays; their seeds were chosen on the CPU so that both hold (check_well_posed)."""
import functools

import numpy as np

from conftest import load_golden
from oracle import snake_oracle
from oracle.mcts_oracle import Draws, SelfPlayOracle, argmaxs
from oracle.obs_key import StubNet

KEYS = ("alive", "health", "length", "dir", "nodes", "food", "rewards", "counters")
Q_GAP = 1e-4
U_EDGE = 1e-5
TAPE_LEN = 400_000


class CheckedDraws(Draws):
    """Draws over a tape that remembers how close a uniform ever came to an edge of its cdf"""

    def __init__(self, tape):
        super().__init__(tape=tape)
        self.u_edge = np.inf

    def __call__(self, pmf):
        cdf = np.asarray(pmf, np.float64).cumsum()
        cdf /= cdf[-1]
        self.u_edge = min(self.u_edge, float(np.abs(cdf - self.tape[self.pos]).min()))
        return super().__call__(pmf)


@functools.lru_cache(maxsize=None)
def _start(board):
    """recorded start boards as compact dicts.  "11x11x4": those of recorded pit 0 (tests/golden/pit.npz, the _meta /
    state_from_compact pattern of tests/test_arena_gpu.py -- not its spawn tape, which belongs to another trajectory).  pit.npz
    holds 11x11 boards with four snakes only; "7x7x2": the start boards of the sixteen recorded trajectories of tic_7x7x2.npz"""
    if board == "11x11x4":
        z = load_golden("pit.npz")
        H, W, S, hd, n = (int(v) for v in z["p0_meta"][:5])
        return (H, W, S, hd), [{k: z["p0_init_" + k][g] for k in KEYS} for g in range(n)]
    assert board == "7x7x2"
    z = load_golden("tic_7x7x2.npz")
    geo = tuple(int(z[k]) for k in ("H", "W", "S", "health_dec"))
    return geo, [{k: z["st_" + k][i] for k in KEYS} for i in z["ptr"][:-1]]


def start_games(board, n):
    """the first n start boards as oracle games -> (games, (H, W, S, health_dec))"""
    (H, W, S, hd), boards = _start(board)
    assert n <= len(boards)
    return [snake_oracle.Game.from_compact(H, W, S, hd, 0.15, st) for st in boards[:n]], (H, W, S, hd)


def start_states(board, n):
    """the same boards as snk_game_state records for Arena.import_states"""
    from snake_engine.engine import state_from_compact
    (H, W, S, _), boards = _start(board)
    return [state_from_compact(H, W, S, st) for st in boards[:n]]


def search_pit_run(games, nets, searching, alice_snake_cnt, spawn_seed, tape=None, depth=4, breadth=8, base=100):
    """games: oracle Games (index = game id); nets: the two teams' nets (.v); searching: which team moves by search; the food
    spawns are drawn from RandomState(spawn_seed), two uniforms per open game and turn in game order (game.py:131-133).
    Returns a dict: winners (None for a draw), lengths, turns, spawn_log [turn - 1][game id] (the spawned cell, -1 none, -2 the
    game was closed), games (each on the board of its verdict), tape_pos (Draws.pos per team, None for a greedy one), q_gap, u_edge"""
    S = games[0].g.S
    a_cnt = S // 2 if alice_snake_cnt is None else alice_snake_cnt
    rng = np.random.RandomState(spawn_seed)
    oracles = [SelfPlayOracle(net, base, False, depth, breadth, draws=CheckedDraws(tape)) if s else None
               for net, s in zip(nets, searching)]
    winners, lengths = [None] * len(games), [0] * len(games)
    live = list(range(len(games)))
    spawn_log, q_gap, turn = [], np.inf, 0
    while live:
        turn += 1
        dense = {g: np.ones(S, np.uint8) for g in live}
        for k in (0, 1):                                                    # team A before team B
            mine = (lambda s: s < a_cnt) if k == 0 else (lambda s: s >= a_cnt)
            if oracles[k] is not None:
                rows, V, moves = oracles[k].root_turn([games[g] for g in live])
                for (gi, s), v, m in zip(rows, V, moves):
                    if mine(s):
                        dense[live[gi]][s] = m
                        top = np.sort(np.asarray(v, np.float64))
                        q_gap = min(q_gap, float(top[2] - top[1]))
            else:
                ids = [(g, s) for g in live for s in games[g].alive_ids() if mine(s)]
                states = [games[g].make_state(s) for g, s in ids]
                for (g, s), m in zip(ids, argmaxs(nets[k].v(states)) if states else []):
                    dense[g][s] = m
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
            else:                                                           # :48-60
                ids = games[g].alive_ids()
                if not any(s < a_cnt for s in ids) or not any(s >= a_cnt for s in ids):
                    winners[g] = ids[0]
                else:
                    nxt.append(g)
        live = nxt
    return dict(winners=winners, lengths=lengths, turns=turn, spawn_log=spawn_log, games=games,
                tape_pos=[None if o is None else o.draw.pos for o in oracles], q_gap=q_gap,
                u_edge=min([o.draw.u_edge for o in oracles if o is not None], default=np.inf))


# ---- the configurations of the parity test: (start boards, games, breadth, searching teams, seed) ----
# every match gives alice snake 0 alone (alice_snake_cnt 1: 1 v 3 on 11x11, the duel on 7x7) and searches to depth 4; the
# seed gives the uniform tape (RandomState(seed)) and the food spawns (RandomState(seed + 1000))
_SS, _SG, _GS = (True, True), (True, False), (False, True)
CASES = {
    "7x7x2-b8-search-v-search": ("7x7x2", 6, 8, _SS, 1),
    "7x7x2-b8-search-v-greedy": ("7x7x2", 6, 8, _SG, 1),
    "7x7x2-b8-greedy-v-search": ("7x7x2", 6, 8, _GS, 0),
    "7x7x2-b16-search-v-search": ("7x7x2", 6, 16, _SS, 0),
    "7x7x2-b16-search-v-greedy": ("7x7x2", 6, 16, _SG, 2),
    "7x7x2-b16-greedy-v-search": ("7x7x2", 6, 16, _GS, 0),
    "11x11x4-b8-search-v-search": ("11x11x4", 5, 8, _SS, 0),
    "11x11x4-b8-search-v-greedy": ("11x11x4", 5, 8, _SG, 0),
    "11x11x4-b8-greedy-v-search": ("11x11x4", 5, 8, _GS, 2),
    "11x11x4-b16-search-v-search": ("11x11x4", 4, 16, _SS, 2),
    "11x11x4-b16-search-v-greedy": ("11x11x4", 4, 16, _SG, 2),
    "11x11x4-b16-greedy-v-search": ("11x11x4", 4, 16, _GS, 0),
}


def uniform_tape(seed):
    return np.random.RandomState(seed).random_sample(TAPE_LEN)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the helper's run of CASES[name], computed once and shared (callers must not change it)"""
    board, n, breadth, searching, seed = CASES[name]
    games, geo = start_games(board, n)
    out = search_pit_run(games, (StubNet(0), StubNet(1)), searching, 1, seed + 1000, uniform_tape(seed), 4, breadth)
    out["geometry"] = geo
    return out


def check_well_posed(out):
    assert out["q_gap"] > Q_GAP, f"a root decision hangs on {out['q_gap']:.3e}"
    assert out["u_edge"] > U_EDGE, f"a rollout uniform lies {out['u_edge']:.3e} from a cdf edge"
    assert max(p or 0 for p in out["tape_pos"]) <= TAPE_LEN


class DeviceStub:
    """oracle.obs_key.StubNet(which) behind the v_device contract.  which 0 is tests/stubnet_device.DeviceStubNNet itself (the low
    key word, on the device); which 1 takes the high word, summed on the device with stubnet_device's own integer arithmetic"""

    def __init__(self, which):
        assert which in (0, 1)
        self.which = which

    def v_device(self, planes, mask):
        import torch
        import stubnet_device as sd
        if self.which == 0:
            return sd.DeviceStubNNet().v_device(planes, mask)
        n = planes.shape[0]
        bits = planes.contiguous().view(torch.int32).reshape(n, -1, 3).to(torch.int64) & 0xFFFFFFFF
        p = torch.arange(bits.shape[1], dtype=torch.int64, device=planes.device)[None, :]
        b0, b1, b2 = bits[..., 0], bits[..., 1], bits[..., 2]
        live = ~((b0 == 0) & (b1 == 0x3F800000) & (b2 == 0))
        x = sd._sm64(sd._sm64((p << 32) | b0) ^ ((b1 << 32) | b2))
        hi = sd._sm64(x ^ sd._c(0xD6E8FEB86659FD93))
        khi = torch.where(live, hi, torch.zeros_like(hi)).sum(dim=1)
        cols = [((sd._lsr(khi, 20 * m) if m else khi) & 0xFFFFF).to(torch.float32) * (2.0 ** -20) * 1.8 - 0.9 for m in range(3)]
        q = torch.stack(cols, dim=1)
        return torch.where(mask.bool(), torch.full_like(q, -1.0), q).contiguous()
