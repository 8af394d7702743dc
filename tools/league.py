"""A league of K nets in one device pit match (snake_engine.league): the cross table, the scores and Elo-scaled Bradley-Terry
ratings of a round robin, 11x11.

    python tools/league.py [--nets 6] [--games 300] [--seats duel|1v3|ffa] [--blocks 4] [--models NAME G0 G1 ...] [--seed 1]
                           [--search B [--depth 8]] [--time] [--pairs 3] [--log profiles/league_ab.log] [--baseline [FLAGS ...]]
                           [--replay K DIR] [--tally]

--nets K plays generation-0 Glorot nets of --blocks blocks, seeds 1..K; --models NAME G0 G1 ... loads NAME<G>.h5 instead (e.g.
--models models/gen 0 15 30).  Every line-up of snake_engine.league.schedule plays --games games, all in lock step in one engine.
--time (duel and 1v3): the league form -- one League.play of all pairings -- against the form the arena offers without it -- one
Arena.match(net_i, net_j, 1) of --games games per ordered pair, one after another -- alternating inside this one process,
`--pairs` times; a host clock around a form that ends in a device synchronise.  Seconds per form, turns played, rows evaluated,
then the medians and their ratio.  The lines are appended to --log behind a line that names the device.
--search B: every seat moves by search (a fresh snake_engine.arena.Searcher of breadth B and --depth around each net per form:
League.play_search against one Arena.match of two Searchers per ordered pair); the time lines then also give the net evaluations
of the searches (Searcher.stats) and, since a searching turn is bound by them, the microseconds per evaluation.
--baseline [FLAGS ...]: scripted owners (snake_engine.arena.Scripted, the fixed yardstick: the same opponent in every run) join the
table and the ratings behind the nets, one per FLAGS value (bits 1 space, 2 heads, 4 food; no value: 7, the whole policy).  A
value look or lookN is the lookahead yardstick (snake_engine.arena.Lookahead: the script one tick deep) with flags 7 or N.  A
scripted owner moves by its script under --search too.  --nets 0 --baseline 0 1 3 7 is the round robin of four flag settings,
--nets 0 --baseline 0 1 3 7 look the same with the lookahead in it.  deep2, deep3, deep4 (a flags digit may follow, as in look5)
are the deep yardstick (snake_engine.arena.Deep: the script that many ticks deep); the board's snake count limits the depth.
play and playPxT (play8x16: 8 playouts of 16 ticks) are the playout yardstick (snake_engine.arena.Playout: flat Monte-Carlo over
the script, with its defaults or P playouts and horizon T).  terr and terrhN (terrh40: the food term counts only at health 40 or
less; a flags digit may follow terr, as in look5: terr5, terr5h40) are the territory yardstick (snake_engine.arena.Territory: the
script with Voronoi territory in place of space).  A t behind look, deepN, play or playPxT puts territory at the leaf of that search
(lookt, deep2t, deep3t, playt: leaf=Territory()), thN the territory with that threshold (lookth40, deep2th40, playth40).
--replay K DIR (not with --time): the round robin records its first K games (League.record) and writes them as DIR/game_<g>.rep,
the text of the reference's replay.rep: two boards per tick.
--tally (not with --time): the round robin also counts every seat's fate on the device (League.tally) and the table is printed
behind the cross table: per net the seats, how many were alive at the verdict, hit a wall, ran into a body, lost a head-on or
starved, food eaten, mean final length and mean turns lived."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "alphasnake-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def format_table(names, t, r):
    """the cross table (wins of the row's net over the column's, draws behind a slash), the scores and the ratings as lines"""
    K = len(names)
    wide = max(7, max(len(n) for n in names) + 1)
    lines = [" " * wide + "".join(f"{n:>{wide + 2}s}" for n in names) + f"{'score':>9s}{'rating':>9s}"]
    for a in range(K):
        cells = "".join(f"{'-':>{wide + 2}s}" if a == b else f"{f'{t.wins[a][b]}/{t.draws[a][b]}':>{wide + 2}s}" for b in range(K))
        lines.append(f"{names[a]:<{wide}s}{cells}{t.score[a]:9.3f}{r[a]:+9.1f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", type=int, default=6)
    ap.add_argument("--games", type=int, default=300)
    ap.add_argument("--seats", choices=("duel", "1v3", "ffa"), default="duel")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--models", nargs="+", default=None, metavar="NAME G0 G1 ...")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--search", type=int, default=None, metavar="B")
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--log", default=None)
    ap.add_argument("--baseline", nargs="*", default=None, metavar="FLAGS")
    ap.add_argument("--replay", nargs=2, default=None, metavar=("K", "DIR"))
    ap.add_argument("--tally", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import leaf_names
    import playout_names
    from snake_engine import arena
    from snake_engine.arena import Arena, Deep, Lookahead, Playout, Scripted, Searcher, Territory
    from snake_engine.league import SEATS, League, ratings, schedule, searchers, table
    from snake_engine.net import glorot_uniform_weights
    from utils.alpha_nnet import AlphaNNet

    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)

    def say(s):                                     # the log grows as the run goes: a run that is cut short leaves what it had
        print(s, flush=True)
        if a.log:
            with open(a.log, "a") as f:
                f.write(s + "\n")

    if a.models:
        names = [f"{os.path.basename(a.models[0])}{g}" for g in a.models[1:]]
        nets = [AlphaNNet(model_name=f"{a.models[0]}{g}.h5") for g in a.models[1:]]
        what = "checkpoints " + " ".join(names)
    else:
        names = [f"seed{s}" for s in range(1, a.nets + 1)]
        nets = [AlphaNNet(input_shape=(21, 21, 3), _weights=glorot_uniform_weights((21, 21, 3), a.blocks, seed=s))
                for s in range(1, a.nets + 1)]
        what = f"generation-0 Glorot nets ({a.blocks} blocks, seeds 1..{a.nets})"

    class Counted:
        """a net that counts the rows it is given (a host counter: no synchronisation)"""
        rows = 0

        def __init__(self, net):
            self.net = net

        def v_device(self, planes, mask):
            Counted.rows += planes.shape[0]
            return self.net.v_device(planes, mask)

    if not a.search:                                # a searcher talks to its net's range guard directly: no wrapper in between
        nets = [Counted(net) for net in nets]
    if a.baseline is not None:
        for flags in a.baseline or ["7"]:
            if leaf_names.parse(flags) is not None:               # lookt, deep2th40, playt: a search with territory at the leaf
                names.append(flags)
                nets.append(leaf_names.player(flags, arena))
            elif playout_names.parse(flags) is not None:          # play, play8x16: the playout yardstick
                names.append(flags)
                nets.append(Playout(**playout_names.parse(flags)))
            elif flags.startswith("terr"):            # terr, terr5, terrh40, terr5h40: the territory yardstick
                digits, _, hungry = flags[4:].partition("h")
                side = Territory(int(digits or 7), int(hungry or 100))
                names.append(f"terr{side.flags}" + (f"h{side.hungry}" if side.hungry != 100 else ""))
                nets.append(side)
            elif flags.startswith("deep"):            # deep2, deep3, deep4; deep25: the deep yardstick, depth 2, flags 5
                names.append(f"deep{int(flags[4])}_{int(flags[5:] or 7)}")
                nets.append(Deep(int(flags[5:] or 7), int(flags[4])))
            elif flags.startswith("look"):            # look, look5: the lookahead yardstick
                names.append(f"look{int(flags[4:] or 7)}")
                nets.append(Lookahead(int(flags[4:] or 7)))
            else:
                names.append(f"script{int(flags)}")
                nets.append(Scripted(int(flags)))
        what += f" and {len(a.baseline or ['7'])} scripted owners"
    K, S = len(nets), SEATS[a.seats]
    owner = schedule(K, a.games, a.seats)
    prop = torch.cuda.get_device_properties(0)
    say(f"league: 11x11, {a.seats}, {K} nets: {what}, {a.games} games per line-up, {len(owner)} games in all, "
        f"{torch.cuda.get_device_name(0)} ({prop.gcnArchName}, {prop.multi_processor_count} CUs), ROCm / HIP {torch.version.hip}, "
        f"torch {torch.__version__}" + (f"; every seat searches, breadth {a.search}, depth {a.depth}" if a.search else ""))
    search = dict(breadth=a.search, depth=a.depth) if a.search else None

    tallies = []

    def league_form(seed, replay=None, tally=False):
        """one League.play (play_search) of every line-up -> (result, seconds, rows evaluated, the searches' net evaluations);
        replay: (K, DIR), the first K games are recorded and written when the match is over; tally: the match's Tally is left in
        `tallies`"""
        Counted.rows = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        league = League(11, 11, S, 1, len(owner), seed)                     # both forms pay for their engines inside the clock
        sides = searchers(nets, search, seed) if search else nets           # ... and for their searchers' tables
        rep = league.record(range(min(int(replay[0]), len(owner)))) if replay else None
        if tally:
            tallies.append(league.tally())
        res = league.play_search(sides, owner) if search else league.play(nets, owner)
        torch.cuda.synchronize()
        if rep is not None:
            os.makedirs(replay[1], exist_ok=True)
            for g in rep.games.tolist():
                rep.write(g, os.path.join(replay[1], f"game_{g}.rep"), append=False)
            say(f"replay: games 0..{len(rep.games) - 1} written to {replay[1]}/game_<g>.rep")
        return res, time.perf_counter() - t0, Counted.rows, sum(s.stats["net_evals"] for s in sides if isinstance(s, Searcher)) if search else 0

    def arena_form(seed):
        """one Arena.match per ordered pair, one after another -> (winner owners in schedule order, seconds, turns, rows, the
        searches' net evaluations)"""
        wo, turns, evals, Counted.rows = [], 0, 0, 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(K):
            for j in range(K):
                if i != j:
                    sd = seed + 31 * (i * K + j)
                    sides = searchers((nets[i], nets[j]), search, sd) if search else (nets[i], nets[j])
                    r = Arena(11, 11, S, 1, a.games, sd).match(sides[0], sides[1], 1)
                    evals += sum(s.stats["net_evals"] for s in sides if isinstance(s, Searcher)) if search else 0
                    wo.append(np.where(r.winners < 0, -1, np.where(r.winners < 1, i, j)))
                    turns += r.turns
        torch.cuda.synchronize()
        return np.concatenate(wo), time.perf_counter() - t0, turns, Counted.rows, evals

    Arena(11, 11, S, 1, 64, 99).match(nets[0], nets[-1], 1)    # first launches, plans and range-guard scales settle outside the timing
    if search:                                                 # ... and the search's, on a small match of each form
        warm = schedule(K, 2, a.seats)
        Arena(11, 11, S, 1, 8, 99).match(*searchers((nets[0], nets[-1]), search, 1), 1)
        League(11, 11, S, 1, len(warm), 99).play_search(searchers(nets, search, 99), warm)
    else:
        League(11, 11, S, 1, len(owner), 99).play(nets, owner)
    if a.time:
        if a.seats == "ffa":
            raise SystemExit("--time compares with Arena.match, which has no free-for-all")
        per = {"league": [], "arena": []}
        evals_text = lambda evals, dt: f", {evals} net evaluations by the searches, {dt / evals * 1e6:.2f} us each" if evals else ""
        for k in range(a.pairs):
            res, dt, rows, evals = league_form(a.seed)
            per["league"].append(dt)
            say(f"time: pair {k} league form: 1 match of {len(owner)} games, {res.turns} turns, {rows} rows evaluated, "
                f"{dt:8.3f} s, {dt / res.turns * 1e3:.3f} ms per turn" + evals_text(evals, dt))
            wo, dt, turns, rows, evals = arena_form(a.seed)
            per["arena"].append(dt)
            say(f"time: pair {k} arena form: {K * (K - 1)} matches of {a.games} games, {turns} turns, {rows} rows evaluated, "
                f"{dt:8.3f} s, {dt / turns * 1e3:.3f} ms per turn" + evals_text(evals, dt))
        ml, ma = statistics.median(per["league"]), statistics.median(per["arena"])
        say(f"time: median seconds: league form {ml:.3f} (min {min(per['league']):.3f}, max {max(per['league']):.3f}), arena form "
            f"{ma:.3f} (min {min(per['arena']):.3f}, max {max(per['arena']):.3f}), ratio of medians arena / league {ma / ml:.2f}x")
        return
    res, dt, _, _ = league_form(a.seed, a.replay, a.tally)
    t = table(res, owner, K)
    say(f"{res.turns} turns, {dt:.3f} s, {dt / res.turns * 1e3:.3f} ms per turn; wins of the row's net over the column's / draws")
    for line in format_table(names, t, ratings(t.wins, t.draws)):
        say(line)
    for tal in tallies:
        say("every seat's fate:\n" + tal.text(names).rstrip("\n"))


if __name__ == "__main__":
    main()
