"""CPU tests of the searching league (League.play_search): the header declares snk_pit_roots_owned and snk_pit_search_moves_owned
in the league block and the ctypes table binds them, the ABI number did not move, the CPU statement the GPU test compares with
(tests/league_search_ref.py) reproduces tests/search_pit_ref.py with two owners and is well posed on its committed seeds with
everything in it that the sub-list logic could hide behind, the NumPy models of the two kernels against per-cell loops, and the
plumbing of play_search / round_robin(search=...) that runs before any launch."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import REPO

NEW = {"snk_pit_roots_owned": 12, "snk_pit_search_moves_owned": 8}


def _header():
    return open(os.path.join(REPO, "include", "snake_engine.h")).read()


# ---- the boundary ------------------------------------------------------------------------------------------------------------
def test_header_declares_the_two_entry_points_in_the_league_block():
    txt = _header()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == n_args, name
    block = txt[txt.index("the league: an owner per seat"):txt.index("training half")]
    for name in NEW:
        assert re.search(name + r" \(agent\.py:25-99 behind pit_mp_game_runner\.py:23-38\)", block), name
    assert "snk_pit_roots" in block and "(s >= a_cnt)" in block and "search_mask = 3" in block      # the two-team equivalence
    # no argument list of an older pit entry point changed
    for name, n_args in (("snk_pit_rows", 8), ("snk_pit_moves", 7), ("snk_pit_verdict", 10), ("snk_pit_roots", 9),
                         ("snk_pit_search_moves", 10), ("snk_pit_owned_scratch_elems", 2), ("snk_pit_rows_owned", 9),
                         ("snk_pit_verdict_owned", 12)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == n_args, name


def test_lib_binds_the_two_entry_points_with_argtypes():
    import snake_engine
    from snake_engine import _lib
    L = snake_engine.lib()
    vp, i32 = C.c_void_p, C.c_int
    want = {"snk_pit_roots_owned": [vp, vp, i32, vp, i32, C.c_uint32, vp, vp, vp, vp, vp, vp],
            "snk_pit_search_moves_owned": [vp, vp, i32, i32, i32, i32, vp, vp]}
    for name, args in want.items():
        assert _lib.PROTOTYPES[name] == (C.c_int, args), name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    assert _lib.ABI_VERSION == 113 == L.snk_version()
    assert re.search(r"#define SNK_ABI_VERSION 113\b", _header())


def test_bad_arguments_are_refused_before_any_launch():
    import snake_engine
    L = snake_engine.lib()
    assert L.snk_pit_roots_owned(None, None, 0, None, 2, 3, None, None, None, None, None, None) < 0
    assert b"snk_pit_roots_owned" in L.snk_last_error()
    assert L.snk_pit_search_moves_owned(None, None, -1, 4, 0, 0, None, None) < 0 and b"snk_pit_search_moves_owned" in L.snk_last_error()
    assert L.snk_pit_search_moves_owned(None, None, 5, 9, 0, 0, None, None) < 0            # more snakes than a game can have
    assert L.snk_pit_search_moves_owned(None, None, 5, 4, 21, 0, None, None) < 0           # more rows than seats
    assert L.snk_pit_search_moves_owned(None, None, 5, 4, -1, 0, None, None) < 0
    assert L.snk_pit_search_moves_owned(None, None, 5, 4, 0, 0, None, None) < 0            # NULL arrays
    assert L.snk_pit_search_moves_owned(None, None, 0, 4, 0, 0, None, None) == 0           # no game: nothing to do


# ---- the statement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["7x7x2-b8-search-v-search", "7x7x2-b16-greedy-v-search", "11x11x4-b8-search-v-greedy"])
def test_two_owners_with_the_two_team_table_are_search_pit_ref(oracle, name):
    """K = 2 and owner[g][s] = (s >= a_cnt): every open game has both teams, so each owner's list is all open games and the
    statement is search_pit_run draw for draw"""
    import league_ref as LR
    import league_search_ref as R
    import search_pit_ref as SR
    from oracle.obs_key import StubNet
    board, n, breadth, searching, seed = SR.CASES[name]
    want = SR.reference(name)
    games, geo = SR.start_games(board, n)
    tape = SR.uniform_tape(seed)
    out = R.league_search_run(games, (StubNet(0), StubNet(1)), searching, LR.two_team_table(n, geo[2], 1), seed + 1000, [tape, tape],
                              4, breadth)
    assert out["winners"] == want["winners"] and out["lengths"] == want["lengths"] and out["turns"] == want["turns"]
    assert len(out["spawn_log"]) == len(want["spawn_log"])
    assert all(np.array_equal(a, b) for a, b in zip(out["spawn_log"], want["spawn_log"]))
    assert out["tape_pos"] == want["tape_pos"]
    assert out["q_gap"] == want["q_gap"] and out["u_edge"] == want["u_edge"]
    n_open = [int((row >= -1).sum()) for row in out["spawn_log"]]
    assert all(len(lst[o]) == n_open[t] for t, lst in enumerate(out["lists"]) for o in (0, 1) if searching[o])


def test_no_searcher_is_league_run(oracle):
    import league_ref as LR
    import league_search_ref as R
    import search_pit_ref as SR
    table = R.four_table()
    nets = [LR.RefStub(k) for k in range(4)]
    out = R.league_search_run(SR.start_games("11x11x4", 5)[0], nets, (False,) * 4, table, 7)
    want = LR.league_run(SR.start_games("11x11x4", 5)[0], nets, table, food_seed=7)
    for k in ("winners", "winner_owner", "lengths", "turns", "branch"):
        assert out[k] == want[k], k
    assert out["counts"] == [row + [0] * 4 for row in want["counts"]]
    assert all(np.array_equal(a, b) for a, b in zip(out["spawn_log"], want["spawn_log"]))


@pytest.mark.parametrize("name", list(__import__("league_search_ref").CASES))
def test_the_committed_cases_are_well_posed_and_hide_nothing(oracle, name):
    import league_search_ref as R
    out = R.reference(name)
    board, breadth, searching, seed = R.CASES[name]
    print(f"\n{name}: {out['turns']} turns, q_gap {out['q_gap']:.3e}, u_edge {out['u_edge']:.3e}, draws {out['tape_pos']}, "
          f"{R.conditions(out, searching, R.TABLES[board]())}")
    R.check_well_posed(out)
    R.check_conditions(name, out)
    assert breadth in (8, 16)
    assert [p is not None for p in out["tape_pos"]] == list(searching) and all(p > 0 for p in out["tape_pos"] if p is not None)
    assert max(out["lengths"]) == out["turns"] == len(out["spawn_log"]) == len(out["counts"])
    assert all(len(row) == searching.count(False) + len(searching) for row in out["counts"])


def test_the_cases_cover_what_the_issue_names():
    import league_search_ref as R
    from snake_engine.league import schedule
    assert np.array_equal(R.duel_table(), schedule(3, 1, "duel"))
    four = R.four_table().tolist()
    assert any(len(set(row)) == 2 and row.count(row[0]) == 1 for row in four)          # a 1 v 3 line-up
    assert any(len(set(row)) == 4 for row in four)                                       # a four-owner line-up
    cases = list(R.CASES.values())
    assert {c[1] for c in cases} == {8, 16} and {c[0] for c in cases} == {"7x7x2", "11x11x4"}
    for board in ("7x7x2", "11x11x4"):
        kinds = {(all(c[2]), any(c[2])) for c in cases if c[0] == board}
        assert (True, True) in kinds and (False, True) in kinds                          # every owner searching, and a mix
    assert max(len(c[2]) for c in cases) >= 3                                            # three distinct nets and more


# ---- the NumPy models against per-cell loops ---------------------------------------------------------------------------------------
def _roots_loop(alive, live, owner, K, mask):
    n, S = alive.shape
    counts, slots, rank = [0] * K, [], -np.ones((n, S), np.int32)
    for o in range(K):
        if not (mask >> o) & 1:
            continue
        for g in range(n):
            seats = [s for s in range(S) if live[g] and alive[g][s] and owner[g][s] == o]
            if seats:
                for s in seats:
                    rank[g][s] = len(slots)
                slots.append(g)
                counts[o] += 1
    return counts, slots, rank


@pytest.mark.parametrize("K, mask", [(1, 1), (2, 3), (3, 0b101), (3, 0b010), (16, 0xFFFF), (16, 0x5555), (2, 0b10100)])
def test_roots_owned_model(K, mask):
    import league_search_ref as R
    rng = np.random.RandomState(K + mask)
    n, S = 37, 4
    alive, live = (rng.rand(n, S) < 0.6).astype(np.uint8), (rng.rand(n) < 0.7).astype(np.uint8)
    owner = rng.randint(0, K + 2, size=(n, S)).astype(np.uint8)                          # K and K + 1: out of range
    counts, slots, rows, rank = R.roots_owned_model(alive, live, owner, K, mask)
    if mask & ((1 << K) - 1) == 0:
        assert counts == [0] * K and slots is None and rows is None and rank is None
        return
    want = _roots_loop(alive, live, owner, K, mask)
    assert counts == want[0] and slots.tolist() == want[1] and np.array_equal(rank, want[2])
    assert np.array_equal(rows, alive[slots]) and sum(counts) <= n * S
    assert all(counts[o] == 0 for o in range(K) if not (mask >> o) & 1)


def test_roots_owned_model_by_hand():
    import league_search_ref as R
    #                 owners       alive        open
    alive = np.array([[1, 1, 1, 1], [0, 1, 1, 0], [1, 1, 0, 0], [1, 1, 1, 1]], np.uint8)
    owner = np.array([[0, 1, 1, 2], [0, 1, 2, 2], [2, 2, 0, 1], [0, 0, 0, 0]], np.uint8)
    live = np.array([1, 1, 1, 0], np.uint8)
    counts, slots, rows, rank = R.roots_owned_model(alive, live, owner, 3, 0b101)
    assert counts == [1, 0, 3] and slots.tolist() == [0, 0, 1, 2]
    assert rank.tolist() == [[0, -1, -1, 1], [-1, -1, 2, -1], [3, 3, -1, -1], [-1, -1, -1, -1]]
    assert np.array_equal(rows, alive[[0, 0, 1, 2]])
    found = np.arange(16, dtype=np.uint8).reshape(4, 4) % 3
    before = np.full((4, 4), 2, np.uint8)
    assert R.search_moves_owned_model(found, rank, 4, 0, before).tolist() == [[0, 1, 1, 1], [1, 1, 1, 1], [0, 1, 1, 1], [1, 1, 1, 1]]
    assert R.search_moves_owned_model(found, rank, 4, 1, before).tolist() == [[0, 2, 2, 1], [2, 2, 1, 2], [0, 1, 2, 2], [2, 2, 2, 2]]


# ---- the plumbing that runs before any launch ----------------------------------------------------------------------------------------
class _Net:
    def v_device(self, planes, mask):
        raise AssertionError("no evaluation in a CPU test")


def _bare_league(n, S):
    from snake_engine.league import League
    league = League.__new__(League)
    league.engine, league.game_cnt, league.snake_cnt = None, n, S
    return league


def test_play_search_signature_and_what_it_refuses_before_it_touches_the_device():
    from snake_engine.arena import Searcher
    from snake_engine.league import League
    assert list(inspect.signature(League.play_search).parameters) == ["self", "sides", "owner", "init_tape", "spawn_tape", "counts_log"]
    assert list(inspect.signature(League.play).parameters) == ["self", "nets", "owner", "init_tape", "spawn_tape", "counts_log"]
    league, net, ok = _bare_league(4, 2), _Net(), np.zeros((4, 2), np.uint8)
    one = Searcher(net, breadth=8, depth=4, seed=1)
    with pytest.raises(ValueError, match="twice"):
        league.play_search([one, net, one], ok)
    with pytest.raises(TypeError):
        league.play_search([one, object()], ok)
    with pytest.raises(ValueError):
        league.play_search([Searcher(net, 8, 4)] * 0, ok)
    with pytest.raises(ValueError):
        league.play_search([Searcher(net, 8, 4) for _ in range(17)], ok)
    with pytest.raises(ValueError):
        league.play_search([one, net], np.array([[0, 1], [1, 0], [0, 2], [1, 1]]))
    with pytest.raises(TypeError, match="play_search"):
        league.play([net, one], ok)                                                    # play itself keeps refusing a Searcher


def test_round_robin_wraps_every_net_in_a_fresh_searcher(monkeypatch):
    from snake_engine import league as G
    from snake_engine.arena import Searcher
    calls = []

    class Fake:
        def __init__(self, *a):
            calls.append(("init", a))

        def play(self, nets, owner):
            calls.append(("play", list(nets), owner))
            return G.LeagueResult(np.full(len(owner), -1, np.int32), np.full(len(owner), -1, np.int32), np.ones(len(owner), np.int32), 1)

        def play_search(self, sides, owner):
            calls.append(("play_search", list(sides), owner))
            return self.play([], owner)
    monkeypatch.setattr(G, "League", Fake)
    nets = [_Net() for _ in range(3)]
    assert inspect.signature(G.round_robin).parameters["search"].default is None
    G.round_robin(nets, games=2, seats="duel", height=7, width=7, seed=5, search=dict(breadth=16, depth=4))
    assert calls[0] == ("init", (7, 7, 2, 1, 12, 5))
    kind, sides, owner = calls[1]
    assert kind == "play_search" and np.array_equal(owner, G.schedule(3, 2, "duel"))
    assert all(isinstance(s, Searcher) for s in sides) and [s.net for s in sides] == nets
    assert [(s.breadth, s.depth, s.seed) for s in sides] == [(16, 4, 5 + 101 * (o + 1)) for o in range(3)]
    assert len({id(s) for s in sides}) == 3 and all(s.mcts is None for s in sides)
    del calls[:]
    G.round_robin(nets, games=2, seats="duel", height=7, width=7, seed=5)
    assert [c[0] for c in calls] == ["init", "play"] and calls[1][1] == nets
    del calls[:]
    G.round_robin(nets, games=1, seats="1v3", search=dict(breadth=8))                  # no seed: every searcher draws its own
    assert calls[1][0] == "play_search" and len({s.seed for s in calls[1][1]}) == 3
