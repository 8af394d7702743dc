"""CPU tests of the league (snake_engine/league.py): the header declares the three owner-table entry points and the ctypes table
binds them, the ABI number did not move, the module stands on the package alone, and the pure-NumPy pieces -- schedule, table,
ratings -- against hand-made cases and closed forms.  The CPU statement the GPU tests compare with (tests/league_ref.py) is
pinned here to the four pits the unmodified reference recorded."""
import ast
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from conftest import PKG, REPO

NEW = {"snk_pit_owned_scratch_elems": 2, "snk_pit_rows_owned": 9, "snk_pit_verdict_owned": 12}


def _header():
    return open(os.path.join(REPO, "include", "snake_engine.h")).read()


# ---- the boundary ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_owner_entry_points_with_the_lines_they_generalise():
    txt = _header()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == n_args, name
    assert re.search(r"#define SNK_PIT_MAX_OWNERS 16\b", code)
    block = txt[txt.index("snk_pit_rows_owned ("):]
    for name, cite in (("snk_pit_rows_owned", "pit_mp_game_runner.py:23-35"), ("snk_pit_verdict_owned", "pit_mp_game_runner.py:39-62")):
        assert re.search(name + r" \(" + re.escape(cite) + r"\)", block), (name, cite)
    # the two-team entry points keep their argument lists
    for name, n_args in (("snk_pit_rows", 8), ("snk_pit_verdict", 10), ("snk_pit_moves", 7), ("snk_pit_scratch_elems", 1)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == n_args, name


def test_lib_binds_the_owner_entry_points():
    import snake_engine
    from snake_engine import _lib
    L = snake_engine.lib()
    for name, n_args in NEW.items():
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == n_args, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(args), name
    # K columns of tile sums: a tile is 1 024 games
    assert L.snk_pit_owned_scratch_elems(1, 1) >= 1 and L.snk_pit_owned_scratch_elems(5000, 16) >= 16 * 5
    assert L.snk_pit_owned_scratch_elems(300000, 16) >= 16 * 293
    assert L.snk_pit_owned_scratch_elems(10, 0) < 0 and L.snk_pit_owned_scratch_elems(10, 17) < 0


def test_abi_version_is_still_113():
    import snake_engine
    from snake_engine import _lib
    assert _lib.ABI_VERSION == 113 == snake_engine.lib().snk_version()
    assert re.search(r"#define SNK_ABI_VERSION 113\b", _header())


def test_league_stands_on_the_package_alone():
    src = open(os.path.join(PKG, "snake_engine", "league.py")).read()
    mods = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            mods |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add("." * node.level + (node.module or ""))
    assert mods <= {"collections", "numpy", "torch", "._lib", ".engine", ".arena"}, mods
    assert {".arena", ".engine", "._lib"} <= mods
    assert "oracle" not in src.lower()
    import snake_engine.league as G
    assert G.LeagueResult._fields == ("winners", "winner_owner", "lengths", "turns")
    assert G.LeagueTable._fields == ("wins", "draws", "games", "score")
    assert G.MAX_OWNERS == 16
    for name in ("play", "from_engine", "import_states"):
        assert callable(getattr(G.League, name))
    for name in ("schedule", "table", "ratings", "round_robin"):
        assert callable(getattr(G, name))


def test_league_refuses_to_run_without_a_gpu():
    import torch
    import snake_engine
    from snake_engine.league import League
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(snake_engine.EngineError):
        League(7, 7, 2, 1, 4, seed=1)


# ---- schedule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, games", [(2, 1), (3, 8), (6, 5), (16, 2)])
def test_schedule_duel_and_1v3(K, games):
    from snake_engine.league import schedule
    pairs = [(i, j) for i in range(K) for j in range(K) if i != j]
    assert pairs == sorted(pairs)
    duel = schedule(K, games, "duel")
    assert duel.dtype == np.uint8 and duel.shape == (K * (K - 1) * games, 2)
    assert duel.tolist() == [[i, j] for i, j in pairs for _ in range(games)]
    one = schedule(K, games, "1v3")
    assert one.dtype == np.uint8 and one.shape == (K * (K - 1) * games, 4)
    assert one.tolist() == [[i, j, j, j] for i, j in pairs for _ in range(games)]
    seen = {}
    for row in duel.tolist():
        seen[tuple(row)] = seen.get(tuple(row), 0) + 1
    assert seen == {p: games for p in pairs}


@pytest.mark.parametrize("K, games", [(4, 1), (5, 3), (7, 2)])
def test_schedule_ffa(K, games):
    from snake_engine.league import schedule
    t = schedule(K, games, "ffa")
    combos = list(itertools.combinations(range(K), 4))
    assert t.dtype == np.uint8 and t.shape == (len(combos) * 4 * games, 4)
    want = [list(c[r:] + c[:r]) for c in combos for r in range(4) for _ in range(games)]
    assert t.tolist() == want
    seen = {}
    for row in t.tolist():
        assert len(set(row)) == 4
        seen[tuple(row)] = seen.get(tuple(row), 0) + 1
    assert len(seen) == 4 * len(combos) and set(seen.values()) == {games}
    # every net of a combination sits in every seat exactly `games` times
    for c in combos:
        rows = t[[set(r) == set(c) for r in t.tolist()]]
        for seat in range(4):
            assert sorted(rows[:, seat].tolist()) == sorted(list(c) * games)


def test_schedule_refusals():
    from snake_engine.league import schedule
    for args in ((3, 2, "ffa"), (17, 1, "duel"), (0, 1, "duel"), (3, 0, "duel"), (3, 1, "2v2")):
        with pytest.raises(ValueError):
            schedule(*args)


# ---- table -------------------------------------------------------------------------------------------------------------------
def _result(winner_owner):
    from snake_engine.league import LeagueResult
    wo = np.array(winner_owner, np.int32)
    return LeagueResult(np.where(wo >= 0, 0, -1).astype(np.int32), wo, np.ones(len(wo), np.int32), 1)


def test_table_hand_made_games():
    import league_ref
    from snake_engine.league import table
    owner = np.array([[0, 1, 2, 3],        # the four-owner draw
                      [3, 1, 0, 2],        # owner 2 beats three others
                      [0, 1, 1, 1],        # 1 v 3: owner 0 wins
                      [0, 1, 1, 1],        # 1 v 3: owner 1 wins
                      [2, 2, 3, 3],        # a drawn game of two owners
                      [1, 1, 1, 1]],       # one owner alone: nobody is beaten, nobody met
                     np.uint8)
    wo = [-1, 2, 0, 1, -1, 1]
    t = table(_result(wo), owner, 5)
    wins = np.zeros((5, 5), np.int64)
    wins[2, [0, 1, 3]] = 1
    wins[0, 1] += 1
    wins[1, 0] += 1
    draws = np.zeros((5, 5), np.int64)
    draws[:4, :4] = 1 - np.eye(4, dtype=np.int64)
    draws[2, 3] += 1
    draws[3, 2] += 1
    games = np.zeros((5, 5), np.int64)
    games[:4, :4] = 2 * (1 - np.eye(4, dtype=np.int64))
    games[0, 1] += 2
    games[1, 0] += 2
    games[2, 3] += 1
    games[3, 2] += 1
    assert np.array_equal(t.wins, wins) and np.array_equal(t.draws, draws) and np.array_equal(t.games, games)
    assert t.wins.dtype == t.draws.dtype == t.games.dtype == np.int64
    assert np.array_equal(t.draws, t.draws.T) and np.array_equal(t.games, t.games.T)
    want = [(1 + 1.5) / 8, (1 + 1.5) / 8, (3 + 2.0) / 7, (0 + 2.0) / 7]
    assert np.allclose(t.score[:4], want, rtol=0, atol=1e-15) and np.isnan(t.score[4])
    m = league_ref.table_model(wo, owner, 5)
    for a, b in zip(t[:3], m[:3]):
        assert np.array_equal(a, b)
    assert np.array_equal(t.score, m[3], equal_nan=True)
    with pytest.raises(ValueError):
        table(_result([-1, 2, 2, 1, -1, 1]), owner, 5)      # owner 2 holds no seat of game 2


def test_table_of_a_duel_is_the_score_pit_writes():
    """pit.py:37-45: the challenger's score = (its wins + draws / 2) / games, the champion's snake first"""
    import league_ref
    from snake_engine.league import schedule, table
    rng = np.random.RandomState(3)
    owner = schedule(3, 50, "duel")
    seat = rng.randint(-1, 2, size=len(owner))                       # -1 a draw, else the winning seat
    wo = np.where(seat < 0, -1, owner.astype(np.int64)[np.arange(len(owner)), np.maximum(seat, 0)])
    t = table(_result(wo), owner, 3)
    assert np.array_equal(t.wins + t.wins.T + t.draws, t.games) and (t.games[~np.eye(3, dtype=bool)] == 100).all()
    for champion, challenger in ((0, 1), (2, 0)):
        g = (owner[:, 0] == champion) & (owner[:, 1] == challenger)
        won, lost, drawn = (wo[g] == challenger).sum(), (wo[g] == champion).sum(), (wo[g] < 0).sum()
        assert won + lost + drawn == 50
    for a in range(3):
        g = (owner == a).any(1)
        assert t.score[a] == ((wo[g] == a).sum() + 0.5 * (wo[g] < 0).sum()) / g.sum()
    assert ((t.score >= 0) & (t.score <= 1)).all()
    m = league_ref.table_model(wo.tolist(), owner, 3)
    assert all(np.array_equal(a, b) for a, b in zip(t, m))


# ---- ratings -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w, l, d", [(10, 5, 3), (0, 20, 0), (7, 7, 0), (300, 0, 0), (1, 2, 597)])
def test_ratings_two_nets_closed_form(w, l, d):
    from snake_engine.league import ratings
    r = ratings(np.array([[0, w], [l, 0]]), np.array([[0, d], [d, 0]]))
    want = 400 * np.log10((w + d / 2 + 0.5) / (l + d / 2 + 0.5))
    assert r.dtype == np.float64 and r[0] == 0.0
    assert abs(-r[1] - want) <= 1e-9 * max(1.0, abs(want)), (r, want)


def test_ratings_finite_for_a_net_that_loses_everything_and_invariant_under_relabelling():
    from snake_engine.league import ratings
    rng = np.random.RandomState(4)
    K = 5
    wins = rng.randint(0, 30, size=(K, K))
    np.fill_diagonal(wins, 0)
    wins[3] = 0                                                      # net 3 never wins
    draws = rng.randint(0, 5, size=(K, K))
    draws = draws + draws.T
    np.fill_diagonal(draws, 0)
    draws[3] = draws[:, 3] = 0                                       # ... and never draws
    r = ratings(wins, draws)
    assert np.isfinite(r).all() and r[0] == 0.0 and r[3] == r.min() and r[3] < -100
    perm = rng.permutation(K)
    rp = ratings(wins[np.ix_(perm, perm)], draws[np.ix_(perm, perm)])
    assert np.allclose(rp - rp.mean(), (r - r.mean())[perm], rtol=0, atol=1e-6)
    # stronger results, higher rating; the fixed point of the iteration: expected points equal points made
    p = 10 ** (r / 400)
    w = wins + 0.5 * draws + 0.5 * (1 - np.eye(K))
    expected = ((w + w.T) * p[:, None] / (p[:, None] + p[None, :])).sum(1)
    assert np.allclose(expected, w.sum(1), rtol=1e-6)
    assert ratings(np.zeros((1, 1)), np.zeros((1, 1))).tolist() == [0.0]


# ---- the CPU statement against the recorded reference pits ---------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_league_ref_with_the_two_team_table_replays_the_recorded_pit(ci):
    import league_ref
    from oracle.obs_key import StubNet
    z, p, H, W, S, hd, n, a_cnt = league_ref.meta(ci)
    owner = league_ref.two_team_table(n, S, a_cnt)
    out = league_ref.league_run(league_ref.start_games(ci), [StubNet(0), StubNet(1)], owner,
                                spawn_tape=lambda turn: z[p + "spawn"][turn - 1])
    assert [-1 if w is None else w for w in out["winners"]] == z[p + "winners"].tolist()
    assert out["lengths"] == z[p + "lengths"].tolist() and out["turns"] == int(z[p + "lengths"].max())
    assert [None if w is None else int(owner[g][w]) for g, w in enumerate(out["winners"])] == out["winner_owner"]
    a = S // 2 if a_cnt is None else a_cnt
    for row in out["counts"]:
        assert len(row) == 2 and sum(row) > 0
    assert out["counts"][0] == [n * a, n * (S - a)]


@pytest.mark.parametrize("name", ["six-owners-run0", "six-owners-run1", "six-owners-run2"])
def test_the_six_owner_matches_take_every_branch(name):
    """the conditions the GPU test asserts, confirmed here with the food seed it uses"""
    import league_ref
    out = league_ref.reference(name)
    league_ref.check_conditions(out)
    assert 10 <= out["turns"] <= 400 and out["turns"] == max(out["lengths"])
    assert {int(o) for row in league_ref.case_table(name) for o in row} == set(range(6))


def test_the_free_for_all_has_winners_of_all_four_owners():
    import league_ref
    out = league_ref.reference("ffa-run1")
    assert {w for w in out["winner_owner"] if w is not None} == {0, 1, 2, 3}
    assert out["turns"] == max(out["lengths"]) >= 20
