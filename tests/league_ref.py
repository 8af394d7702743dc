"""Test infrastructure: the CPU statement of a league match -- oracle.pit_oracle.pit_run's loop (pit_mp_game_runner.py:14-63) over
oracle.snake_oracle games with the team split `s < alice_snake_cnt` replaced by a table owner[game][seat] -- and NumPy models of
the two kernels behind it (snk_pit_rows_owned, snk_pit_verdict_owned) and of snake_engine.league.table.

    rows      every alive snake of every open game, bucketed by its seat's owner (:23-35); inside an owner games ascend and ids
              ascend inside a game; each owner's net sees its own rows (pit_agent.py:10-13)
    verdict   a done game: the last id whose reward is +1, None without one (:43-47); a game that is not done and whose alive
              snakes all belong to one owner: the first alive id (:48-60 with "a team" read as "an owner"); otherwise it stays open

With K = 2 and owner[g][s] = (s >= alice_snake_cnt) this is pit_run itself, which tests/test_league_cpu.py pins to the four
recorded reference pits of tests/golden/pit.npz.

Six stub nets: oracle.obs_key.StubNet(which) for which = 0, 1, 2 and the same three with every unmasked value negated (the masked
-1 stays).  Food is drawn the way Game.tic draws it (game.py:131-133), two uniforms per open game and turn in game order from
RandomState(FOOD_SEED); the cells are logged and the device replays them as its spawn tape.

CASES lists the matches the GPU test plays; check_conditions states what they have to contain (every branch of the verdict, a turn
in which an owner has no row while the match goes on).  The seed was fixed on the CPU with both conditions met."""
import functools

import numpy as np

from conftest import load_golden
from oracle import snake_oracle
from oracle.mcts_oracle import argmaxs
from oracle.obs_key import obstacle_mask, stub_q

KEYS = ("alive", "health", "length", "dir", "nodes", "food", "rewards", "counters")
FOOD_SEED = 7


# ---- the recorded pits' boards ---------------------------------------------------------------------------------------------
def meta(ci):
    """run ci of tests/golden/pit.npz -> (z, prefix, H, W, S, health_dec, n, alice_snake_cnt or None)"""
    z = load_golden("pit.npz")
    p = f"p{ci}_"
    H, W, S, hd, n, a_cnt = (int(v) for v in z[p + "meta"])
    return z, p, H, W, S, hd, n, (None if a_cnt < 0 else a_cnt)


def start_games(ci):
    z, p, H, W, S, hd, n, _ = meta(ci)
    return [snake_oracle.Game.from_compact(H, W, S, hd, 0.15, {k: z[p + "init_" + k][g] for k in KEYS}) for g in range(n)]


def start_states(ci):
    """the same boards as snk_game_state records for League.import_states"""
    from snake_engine.engine import state_from_compact
    z, p, H, W, S, hd, n, _ = meta(ci)
    return [state_from_compact(H, W, S, {k: z[p + "init_" + k][g] for k in KEYS}) for g in range(n)]


def two_team_table(n, S, a_cnt):
    a = S // 2 if a_cnt is None else a_cnt                                  # pit_mp_game_runner.py:17-18
    return np.tile((np.arange(S) >= a).astype(np.uint8), (n, 1))


# ---- the six stub nets -----------------------------------------------------------------------------------------------------
def _negated(q, masked):
    return np.where(masked, np.float32(-1.0), -q).astype(np.float32)


class RefStub:
    """stub net number k of six: stub_q(which = k % 3), for k >= 3 with every unmasked value negated"""

    def __init__(self, k):
        self.which, self.negate = k % 3, k >= 3

    def v(self, X):
        arr = np.array(X, dtype=np.float32)
        q = stub_q(arr, which=self.which)
        return _negated(q, obstacle_mask(arr)) if self.negate else q


class DeviceStub:
    """the same net behind the v_device contract (the values are computed on the host from the device's observations, as
    tests/test_arena_gpu.py's stub does: a parity stub, not a fast one)"""

    def __init__(self, k):
        self.which, self.negate = k % 3, k >= 3

    def v_device(self, planes, mask):
        import torch
        q = stub_q(planes.cpu().numpy(), which=self.which)
        masked = mask.cpu().numpy().astype(bool)
        assert np.array_equal(q == -1.0, masked)
        if self.negate:
            q = _negated(q, masked)
        return torch.as_tensor(q, device=planes.device)


# ---- the loop ----------------------------------------------------------------------------------------------------------------
def league_run(games, nets, owner, spawn_tape=None, food_seed=None):
    """games: oracle Games (index = game id); nets: K objects with .v(states); owner[g][s] in 0..K-1; spawn_tape(turn) -> the
    recorded spawn cell per game id, or food_seed: the spawns are drawn from RandomState(food_seed).  Returns a dict: winners
    (None for a draw), winner_owner (None), lengths, turns, counts [turn - 1] = the K row counts, spawn_log [turn - 1][game id]
    (-2: the game was closed), branch [game id] = which line of the verdict closed the game, boards (each game's compact board
    at its verdict: a game is not ticked again after it)"""
    S, K = games[0].g.S, len(nets)
    owner = np.asarray(owner)
    assert owner.shape == (len(games), S) and owner.min() >= 0 and owner.max() < K
    rng = None if food_seed is None else np.random.RandomState(food_seed)
    winners, lengths, branch = [None] * len(games), [0] * len(games), [None] * len(games)
    live = list(range(len(games)))
    counts, spawn_log, turn = [], [], 0
    while live:
        turn += 1
        states, ids = [[] for _ in range(K)], [[] for _ in range(K)]
        for g in live:                                                      # :26-32, a bucket per owner
            for s, st in zip(games[g].alive_ids(), games[g].get_states()):
                states[owner[g][s]].append(st)
                ids[owner[g][s]].append((g, s))
        counts.append([len(b) for b in ids])
        dense = {g: np.ones(S, np.uint8) for g in live}
        for o in range(K):                                                  # :33-38, every net on its own rows
            if ids[o]:
                for (g, s), m in zip(ids[o], argmaxs(nets[o].v(states[o]))):
                    dense[g][s] = m
        tape = spawn_tape(turn) if spawn_tape is not None else None
        spawn_log.append(np.full(len(games), -2, np.int16))
        nxt = []
        for g in live:
            if rng is not None:
                done = games[g].tic(dense[g], draws=(rng.random_sample(), rng.random_sample()))
            else:
                done = games[g].tic(dense[g], spawn_cell=int(tape[g]) if tape is not None else -1)
            spawn_log[-1][g] = games[g].last_spawn if rng is not None else (int(tape[g]) if tape is not None else -1)
            lengths[g] += 1
            if done:                                                        # :43-47
                for i, r in enumerate(games[g].rewards):
                    if r == 1.0:
                        winners[g] = i
                branch[g] = "done, winner" if winners[g] is not None else "done, draw"
            else:                                                           # :48-60
                alive = games[g].alive_ids()
                if len({int(owner[g][s]) for s in alive}) <= 1:
                    winners[g] = alive[0] if alive else None
                    branch[g] = "one owner left"
                else:
                    nxt.append(g)
        live = nxt
    return dict(winners=winners, winner_owner=[None if w is None else int(owner[g][w]) for g, w in enumerate(winners)],
                lengths=lengths, turns=turn, counts=counts, spawn_log=spawn_log, branch=branch,
                boards=[g.compact() for g in games])


# ---- the matches of the GPU test -----------------------------------------------------------------------------------------------
def six_owner_table(n):
    """[0, k, k, k] for odd g, [k, 0, k, 0] for even g, k = 1 + g % 5"""
    t = np.zeros((n, 4), np.uint8)
    for g in range(n):
        k = 1 + g % 5
        t[g] = [0, k, k, k] if g % 2 else [k, 0, k, 0]
    return t


def ffa_table(n):
    return ((np.arange(n)[:, None] + np.arange(4)[None, :]) % 4).astype(np.uint8)


CASES = {                       # name: (recorded run whose start boards are used, number of stub nets, owner table)
    "six-owners-run0": (0, 6, six_owner_table),
    "six-owners-run1": (1, 6, six_owner_table),
    "six-owners-run2": (2, 6, six_owner_table),
    "ffa-run1": (1, 4, ffa_table),
}


def case_table(name):
    ci, K, make = CASES[name]
    return make(meta(ci)[6])


@functools.lru_cache(maxsize=None)
def reference(name):
    """league_run of CASES[name], computed once and shared (callers must not change it)"""
    ci, K, _ = CASES[name]
    return league_run(start_games(ci), [RefStub(k) for k in range(K)], case_table(name), food_seed=FOOD_SEED)


def check_conditions(out):
    """what a six-owner match has to contain, so that a change of inputs cannot hide a branch"""
    assert set(out["branch"]) == {"done, winner", "done, draw", "one owner left"}, set(out["branch"])
    assert any(0 in row for row in out["counts"]), "no turn in which an owner has no row while the match goes on"


# ---- NumPy models of the two kernels and of the table ----------------------------------------------------------------------------
def rows_owned_model(alive, live, owner, K):
    """snk_pit_rows_owned: (pairs int32[m][2], counts [K]); a seat whose owner byte is >= K has no row"""
    gi, si = np.nonzero(alive.astype(bool) & live.astype(bool)[:, None])    # games ascending, ids ascending inside a game
    ow = owner[gi, si]
    parts = [np.stack([gi[ow == o], si[ow == o]], 1) for o in range(K)]
    return np.concatenate(parts).astype(np.int32).reshape(-1, 2), [len(p) for p in parts]


def verdict_owned_model(alive, done, rewards, owner, turn, live, winner, winner_owner, length):
    """snk_pit_verdict_owned on copies of live / winner / winner_owner / length -> the four arrays after the call"""
    live, winner, winner_owner, length = live.copy(), winner.copy(), winner_owner.copy(), length.copy()
    for g in range(len(live)):
        if not live[g]:
            continue
        if done[g]:
            plus = np.flatnonzero(rewards[g] == 1)
            w = int(plus[-1]) if len(plus) else -1
        else:
            ids = np.flatnonzero(alive[g])
            if len(set(owner[g, ids].tolist())) > 1:
                continue
            w = int(ids[0]) if len(ids) else -1
        winner[g], length[g], live[g] = w, turn, 0
        winner_owner[g] = owner[g, w] if w >= 0 else -1
    return live, winner, winner_owner, length


def table_model(winner_owner, owner, K):
    """snake_engine.league.table game by game -> (wins, draws, games, score)"""
    wins, draws, games = (np.zeros((K, K), np.int64) for _ in range(3))
    for g, w in enumerate(winner_owner):
        O = sorted(set(int(o) for o in owner[g]))
        for a in O:
            for b in O:
                if a != b:
                    games[a][b] += 1
                    if w is None or w < 0:
                        draws[a][b] += 1
        if w is not None and w >= 0:
            assert w in O
            for o in O:
                if o != w:
                    wins[w][o] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        score = (wins.sum(1) + 0.5 * draws.sum(1)) / games.sum(1)
    return wins, draws, games, score
