"""GPU test of the pit's sequence of library calls: every form of Arena.match, League.play and League.play_search issues a
prologue, then per turn the pattern written out below, then the list launches that see nothing left.  The sequence is taken by
the proxy of tests/pit_calls.py in ``engine.L``, the turn's read-backs by the .tolist() calls made in arena.py / league.py, the
net batches by a counting net (as in tests/test_script_gpu.py), and Searcher.search is the stub of the read-back tests that
returns all-straight moves, so the sequence holds the pit's own calls only.  The patterns were written against the arena and the
league as they stood before the one turn loop (four hand-kept copies of the turn) and hold unchanged for the one loop."""
import sys

import numpy as np
import pytest

from pit_calls import Calls

pytestmark = pytest.mark.gpu

SHAPES = {"7x7x2": (7, 7, 2, 8), "11x11x4": (11, 11, 4, 24)}            # height, width, snakes, games; a_cnt is 1
TICK = ["snk_engine_step_active_tape", "snk_engine_rewards"]
RECORDED_TICK = ["snk_pit_record_moves", "snk_engine_step_active_tape", "snk_pit_record_boards", "snk_engine_rewards"]
RECORDED = [5, 0, 3]

# sides: N a net, C a Scripted, S a Searcher.  Per form: the sides, with a recorder or not, the list launches of a turn, and what
# follows them up to the tick.  In an open game of the arena both teams have a snake alive, so its patterns are fixed lists
ARENA = {
    "net/net": ("NN", False, ["snk_pit_rows"], ["snk_engine_observe", "snk_pit_moves"]),
    "net/Scripted": ("NC", False, ["snk_pit_rows"], ["snk_engine_observe", "snk_pit_script_values", "snk_pit_moves"]),
    "Scripted/Scripted": ("CC", False, ["snk_pit_rows"], ["snk_pit_script_values", "snk_pit_script_values", "snk_pit_moves"]),
    "Searcher/Searcher": ("SS", False, ["snk_pit_roots"], ["snk_pit_search_moves"]),
    "Searcher/net": ("SN", False, ["snk_pit_roots", "snk_pit_rows"], ["snk_engine_observe", "snk_pit_moves", "snk_pit_search_moves"]),
    "net/Searcher": ("NS", False, ["snk_pit_roots", "snk_pit_rows"], ["snk_engine_observe", "snk_pit_moves", "snk_pit_search_moves"]),
    "Searcher/Scripted": ("SC", False, ["snk_pit_roots", "snk_pit_rows"],
                          ["snk_pit_script_values", "snk_pit_moves", "snk_pit_search_moves"]),
    "net/net recorded": ("NN", True, ["snk_pit_rows"], ["snk_engine_observe", "snk_pit_moves"]),
}

# an owner of the league can run out of rows or games while the match goes on: what follows the lists is a function of the turn's
# read-back r (the greedy owners' row counts in owner order, then -- with a Searcher -- the three game counts)
LEAGUE = {
    "play: three nets": ("play", "NNN", False, ["snk_pit_rows_owned"], lambda r: ["snk_engine_observe", "snk_pit_moves"]),
    "play: net, Scripted, net": ("play", "NCN", False, ["snk_pit_rows_owned"], lambda r: (
        ["snk_engine_observe"] * bool(r[0]) + ["snk_pit_script_values"] * bool(r[1]) + ["snk_engine_observe"] * bool(r[2])
        + ["snk_pit_moves"])),
    "play_search: no Searcher": ("play_search", "NNN", False, ["snk_pit_rows_owned"],
                                 lambda r: ["snk_engine_observe", "snk_pit_moves"]),
    "play_search: Searcher, net, Searcher": ("play_search", "SNS", False, ["snk_pit_roots_owned", "snk_pit_rows_owned"], lambda r: (
        ["snk_engine_observe"] * bool(r[0]) + ["snk_pit_moves", "snk_pit_search_moves_owned"])),
    "play_search: three Searchers": ("play_search", "SSS", False, ["snk_pit_roots_owned"], lambda r: ["snk_pit_search_moves_owned"]),
    "play_search: Searcher, Scripted, net": ("play_search", "SCN", False, ["snk_pit_roots_owned", "snk_pit_rows_owned"], lambda r: (
        ["snk_pit_script_values"] * bool(r[0]) + ["snk_engine_observe"] * bool(r[1]) + ["snk_pit_moves", "snk_pit_search_moves_owned"])),
    "play_search: Searcher, Scripted, net recorded": ("play_search", "SCN", True, ["snk_pit_roots_owned", "snk_pit_rows_owned"], lambda r: (
        ["snk_pit_script_values"] * bool(r[0]) + ["snk_engine_observe"] * bool(r[1]) + ["snk_pit_moves", "snk_pit_search_moves_owned"])),
}


class _CountingNet:
    """the device stub net; notes (its owner, the rows of the batch) in a list all nets of a match share"""

    def __init__(self, owner, batches):
        self.owner, self.batches = owner, batches

    def v_device(self, planes, mask):
        from stubnet_device import stub_q_device
        self.batches.append((self.owner, int(planes.shape[0])))
        return stub_q_device(planes, mask)


def _sides(kinds, batches):
    from snake_engine.arena import Scripted, Searcher
    make = {"N": lambda o: _CountingNet(o, batches), "C": lambda o: Scripted(), "S": lambda o: Searcher(_CountingNet(o, batches), 8, 4)}
    return [make[k](o) for o, k in enumerate(kinds)]


def _watched(monkeypatch, pit, S, play):
    """play() on `pit` -> (its result, the library calls, the read-backs made in arena.py / league.py, the searched game counts)"""
    import torch
    from snake_engine import arena as A
    reads, searched = [], []
    tolist = torch.Tensor.tolist

    def noted(self):
        out = tolist(self)
        if sys._getframe(1).f_code.co_filename.endswith(("arena.py", "league.py")):
            reads.append(out)
        return out

    def straight(self, engine, slots, alive):
        searched.append(int(slots.shape[0]))
        assert alive.shape == (slots.shape[0], S) and slots.dtype == torch.int32 and alive.dtype == torch.uint8
        return torch.ones((slots.shape[0], S), dtype=torch.uint8, device=slots.device)
    calls = pit.engine.L = Calls(pit.engine.L)
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "tolist", noted)
        mp.setattr(A.Searcher, "search", straight)
        res = play()
    return res, calls.names, reads, searched


def _expected(prologue, lists, turns, tick, verdict):
    """turns: per turn the calls between the lists and the tick"""
    seq = list(prologue)
    for middle in turns:
        seq += lists + middle + tick + [verdict]
    return seq + lists                                                 # the lists that see nothing left


@pytest.mark.parametrize("form", list(ARENA))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_arena_match(monkeypatch, shape, form):
    from snake_engine.arena import Arena
    H, W, S, n = SHAPES[shape]
    kinds, recorded, lists, middle = ARENA[form]
    arena = Arena(H, W, S, 1, n, seed=3)
    batches = []
    sides = _sides(kinds, batches)
    rep = arena.record(RECORDED) if recorded else None
    res, names, reads, searched = _watched(monkeypatch, arena, S, lambda: arena.match(sides[0], sides[1], 1))
    assert res.turns >= 2 and len(reads) == res.turns + 1, "one read-back per turn and the one that sees nothing left"
    width = 3 if "S" in kinds else 2                                   # {nA, nB} or {nA, nB, G}
    assert all(len(r) == width for r in reads) and not any(reads[-1]) and all(r[-1] for r in reads[:-1])
    assert names == _expected(["snk_pit_record_slots"] if recorded else [], lists, [middle] * res.turns,
                              RECORDED_TICK if recorded else TICK, "snk_pit_verdict")
    assert batches == [(o, r[o]) for r in reads[:-1] for o in (0, 1) if kinds[o] == "N"], "each net on its own team's rows"
    assert searched == [r[2] for r in reads[:-1] for k in kinds if k == "S"], "every searching side gets all open games"
    assert res.wins_a + res.wins_b + res.draws == n and res.lengths.max() == res.turns
    assert rep is None or all(len(rep.frames(g)) == 2 * res.lengths[g] for g in RECORDED)


@pytest.mark.parametrize("form", list(LEAGUE))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_league_play_and_play_search(monkeypatch, shape, form):
    from snake_engine.league import League
    H, W, S, n = SHAPES[shape]
    method, kinds, recorded, lists, middle = LEAGUE[form]
    league = League(H, W, S, 1, n, seed=3)
    owner = (np.arange(n)[:, None] + np.arange(S)[None, :]) % 3        # every game seats two owners (7x7x2) or all three
    batches, counts = [], []
    sides = _sides(kinds, batches)
    rep = league.record(RECORDED) if recorded else None
    res, names, reads, searched = _watched(monkeypatch, league, S, lambda: getattr(league, method)(sides, owner, counts_log=counts))
    assert res.turns >= 2 and len(reads) == res.turns + 1 and counts == reads[:-1] and not any(reads[-1])
    greedy = [o for o, k in enumerate(kinds) if k != "S"]
    Kg = len(greedy)
    assert all(len(r) == (Kg + 3 if "S" in kinds else 3) for r in reads)
    assert names == _expected(["snk_pit_record_slots"] if recorded else [], lists, [middle(r) for r in counts],
                              RECORDED_TICK if recorded else TICK, "snk_pit_verdict_owned")
    assert batches == [(o, r[i]) for r in counts for i, o in enumerate(greedy) if kinds[o] == "N" and r[i]], "each net on its slice"
    assert searched == [G for r in counts for G in r[Kg:] if G], "an owner without a game is skipped"
    assert res.lengths.max() == res.turns and (res.lengths >= 1).all()
    assert rep is None or all(len(rep.frames(g)) == 2 * res.lengths[g] for g in RECORDED)
