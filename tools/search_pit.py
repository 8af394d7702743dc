"""What the search buys over the raw net, and what it costs: Arena.test_pit-style matches between a side that moves by search
(snake_engine.arena.Searcher) and a greedy side of the SAME net, 11x11.

    python tools/search_pit.py [--games 300] [--breadth 16] [--depth 8] [--blocks 4] [--weights CKPT] [--seed 1]
                               [--time] [--pairs 2] [--log profiles/arena_search.log] [--baseline [script|look|deep2|deep3|deep4|play|playPxT|terr|lookt|deep2t|playt|lookth40|...]] [--replay K DIR] [--tally]

Strength (default): 1 v 3 with the searcher alone, 1 v 3 with the searcher's three against the greedy one, and the duel; win and
draw rates of the searching side with their binomial 95 % intervals (Wilson), ms per turn and net evaluations per turn.
--time: greedy v greedy, search v greedy and search v search on the same start boards and engine seed, alternating inside this
one process, `--pairs` times; ms per turn (host clock around a match that ends in a device synchronise), net evaluations per
turn, and the host time DeviceMCTS._ensure took (its buffers are made again whenever the number of open games changes).
--baseline: the net against the scripted opponent (snake_engine.arena.Scripted with the whole policy, the fixed yardstick) instead
of against itself: the greedy net in the duel and in 1 v 3 both ways, then the net moving by search in the duel; the net side's
win and draw rates with the same intervals.  --baseline look: the same against the lookahead yardstick
(snake_engine.arena.Lookahead: the script one tick deep); --baseline deep2 (deep3, deep4): against snake_engine.arena.Deep of that depth;
--baseline play (playPxT, e.g. play8x16): against snake_engine.arena.Playout with its defaults (P playouts of T ticks);
--baseline terr: against snake_engine.arena.Territory with its defaults (the script with Voronoi territory in place of space);
--baseline lookt, deep2t, deep3t, playt (lookth40, deep2th40, playth40): against that search with leaf=Territory()
(Territory(hungry=40)), the names of tools/leaf_names.py.
--replay K DIR: the first match the run reports (strength or --baseline) records its first K games (Arena.record) and writes them
as DIR/game_<g>.rep, the text of the reference's replay.rep: two boards per tick.
--tally: the first match the run reports also counts every seat's fate on the device (Arena.tally) and prints the table: per side
the seats, how many were alive at the verdict, hit a wall, ran into a body, lost a head-on or starved, food eaten, mean final
length and mean turns lived.
The lines are appended to --log behind a line that names the device."""
import argparse
import math
import os
import statistics
import sys
import time

import leaf_names
import playout_names

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "alphasnake-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def wilson(k, n, z=1.959964):
    """the binomial 95 % interval of k successes in n trials"""
    if n == 0:
        return 0.0, 1.0
    p, d = k / n, 1 + z * z / n
    c, h = (p + z * z / (2 * n)) / d, z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n)) / d
    return max(0.0, c - h), min(1.0, c + h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=300)
    ap.add_argument("--breadth", type=int, nargs="+", default=[16])
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--weights", default=None, help="a saved model (.h5) (default: generation-0 Glorot weights, seed 1)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--log", default=None)
    ap.add_argument("--baseline", nargs="?", const="script", default=None,
                    type=lambda v: v if v in ("script", "look", "deep2", "deep3", "deep4", "terr") or playout_names.parse(v) is not None
                    or leaf_names.parse(v) is not None
                    else ap.error(f"--baseline {v}: script, look, deep2, deep3, deep4, terr, play or playPxT, or one of those searches with t or thN behind it"))
    ap.add_argument("--replay", nargs=2, default=None, metavar=("K", "DIR"))
    ap.add_argument("--tally", action="store_true")
    a = ap.parse_args()
    import torch
    from snake_engine import arena as arena_module
    from snake_engine.arena import Arena, Deep, Lookahead, Playout, Scripted, Searcher, Territory
    from snake_engine.mcts import DeviceMCTS
    from snake_engine.net import glorot_uniform_weights
    from utils.alpha_nnet import AlphaNNet

    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)

    def say(s):                                     # the log grows as the run goes: a run that is cut short leaves what it had
        print(s, flush=True)
        if a.log:
            with open(a.log, "a") as f:
                f.write(s + "\n")

    if a.weights:
        net, what = AlphaNNet(model_name=a.weights), os.path.basename(a.weights)
    else:
        net = AlphaNNet(input_shape=(21, 21, 3), _weights=glorot_uniform_weights((21, 21, 3), a.blocks, seed=1))
        what = f"generation-0 Glorot net ({a.blocks} blocks, seed 1)"
    prop = torch.cuda.get_device_properties(0)
    say(f"search_pit: 11x11, {what} on both sides, depth {a.depth}, {a.games} games per match, "
        f"{torch.cuda.get_device_name(0)} ({prop.gcnArchName}, {prop.multi_processor_count} CUs), ROCm / HIP {torch.version.hip}, "
        f"torch {torch.__version__}")

    ensure_s = [0.0]
    ensure = DeviceMCTS._ensure

    def timed_ensure(self, G, health_dec):
        t0 = time.perf_counter()
        out = ensure(self, G, health_dec)
        ensure_s[0] += time.perf_counter() - t0
        return out
    DeviceMCTS._ensure = timed_ensure

    pending = [a.replay]

    def recorder(arena):
        """the Replay of the first reported match, None for every later one"""
        want, pending[0] = pending[0], None
        return None if want is None else arena.record(range(min(int(want[0]), arena.game_cnt)))

    def write_replay(rep):
        if rep is not None:
            os.makedirs(a.replay[1], exist_ok=True)
            for g in rep.games.tolist():
                rep.write(g, os.path.join(a.replay[1], f"game_{g}.rep"), append=False)
            say(f"replay: games 0..{len(rep.games) - 1} of this match written to {a.replay[1]}/game_<g>.rep")

    counting = [a.tally]

    def tallier(arena):
        """the Tally of the first reported match, None for every later one"""
        want, counting[0] = counting[0], False
        return arena.tally() if want else None

    def write_tally(tal, names):
        if tal is not None:
            say("tally of this match:\n" + tal.text(names).rstrip("\n"))

    def play(snakes, a_cnt, searching, breadth, seed, start=None, record=False):
        """one match; searching: which sides move by search -> (result, seconds, net evaluations of the searchers, start boards)"""
        arena = Arena(11, 11, snakes, 1, a.games, seed)
        if start is None:
            start = arena.engine.export()
        else:
            arena.import_states(start)
        sides = [Searcher(net, breadth, a.depth, seed=seed + 11 * k) if s else net for k, s in enumerate(searching)]
        rep = recorder(arena) if record else None
        tal = tallier(arena) if record else None
        ensure_s[0] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = arena.match(sides[0], sides[1], a_cnt)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        write_replay(rep)
        write_tally(tal, ["search" if s else "greedy" for s in searching])
        evals = sum(s.stats["net_evals"] for s in sides if isinstance(s, Searcher))
        return res, dt, evals, start

    play(4, 1, (True, False), 8, 99)                       # first launches, plans and range-guard scales settle outside the timing
    play(4, 1, (False, False), 8, 99)
    if a.baseline:
        script, who_b = (Lookahead(), "lookahead") if a.baseline == "look" else (Scripted(), "script")
        if leaf_names.parse(a.baseline) is not None:
            script, who_b = leaf_names.player(a.baseline, arena_module), a.baseline
        elif a.baseline.startswith("deep"):
            script, who_b = Deep(depth=int(a.baseline[4])), a.baseline
        if a.baseline == "terr":
            script, who_b = Territory(), "territory"
        if playout_names.parse(a.baseline) is not None:
            script, who_b = Playout(**playout_names.parse(a.baseline)), a.baseline
        lineups = [("duel, the net first", 2, 1, 0), ("1v3, the net alone", 4, 1, 0), (f"1v3, three of the net against the {who_b}", 4, 3, 0)]
        movers = [("greedy net", None, lineups)] + [(f"search breadth {b:3d}", b, lineups[:1]) for b in a.breadth]
        for mover, breadth, ups in movers:
            for i, (name, snakes, a_cnt, who) in enumerate(ups):
                side = net if breadth is None else Searcher(net, breadth, a.depth, seed=a.seed + 11)
                arena = Arena(11, 11, snakes, 1, a.games, a.seed + i)
                rep, tal = recorder(arena), tallier(arena)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = arena.match(side, script, a_cnt)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                write_replay(rep)
                write_tally(tal, ["net", who_b])
                wins = (res.wins_a, res.wins_b)[who]
                (wl, wh), (dl, dh) = wilson(wins, a.games), wilson(res.draws, a.games)
                say(f"baseline: {mover} against the {who_b}, {name}: net wins {wins / a.games:.3f} [{wl:.3f}, {wh:.3f}], draws "
                    f"{res.draws / a.games:.3f} [{dl:.3f}, {dh:.3f}], {who_b} wins {(a.games - wins - res.draws) / a.games:.3f}; "
                    f"{res.turns} turns, {dt / res.turns * 1e3:.3f} ms per turn")
    elif a.time:
        forms = [("greedy v greedy", (False, False)), ("search v greedy", (True, False)), ("search v search", (True, True))]
        for breadth in a.breadth:
            start, per = None, {name: [] for name, _ in forms}
            for k in range(a.pairs):
                for name, searching in forms:
                    res, dt, evals, start = play(4, 1, searching, breadth, a.seed, start)
                    per[name].append(dt / res.turns * 1e3)
                    say(f"time: breadth {breadth:3d} rep {k} {name}: {res.turns:4d} turns, {dt:8.3f} s, {dt / res.turns * 1e3:9.3f} ms per "
                        f"turn, {evals / res.turns:10.1f} search evaluations per turn, _ensure {ensure_s[0] * 1e3:7.1f} ms of the match "
                        f"({100 * ensure_s[0] / dt:.2f} %), wins {res.wins_a}-{res.wins_b}, draws {res.draws}")
            say(f"time: breadth {breadth:3d} median ms per turn: " + ", ".join(f"{n} {statistics.median(v):.3f}" for n, v in per.items()))
    else:
        for breadth in a.breadth:
            seats = [("1v3, the searcher alone", 4, 1, (True, False), 0), ("1v3, three searchers against one", 4, 1, (False, True), 1),
                     ("duel, the searcher first", 2, 1, (True, False), 0)]
            for i, (name, snakes, a_cnt, searching, who) in enumerate(seats):
                res, dt, evals, _ = play(snakes, a_cnt, searching, breadth, a.seed + i, record=True)
                wins = (res.wins_a, res.wins_b)[who]
                (wl, wh), (dl, dh) = wilson(wins, a.games), wilson(res.draws, a.games)
                say(f"strength: breadth {breadth:3d} {name}: search wins {wins / a.games:.3f} [{wl:.3f}, {wh:.3f}], draws "
                    f"{res.draws / a.games:.3f} [{dl:.3f}, {dh:.3f}], greedy wins {(a.games - wins - res.draws) / a.games:.3f}; "
                    f"{res.turns} turns, {dt / res.turns * 1e3:.3f} ms per turn, {evals / res.turns:.1f} search evaluations per turn")


if __name__ == "__main__":
    main()
