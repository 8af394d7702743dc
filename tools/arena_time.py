"""The pit match, host loop against device loop: `MPGameRunner.run` and `MPGameRunner.run_device` on the same start boards, the
same engine seed (so the same food spawns) and the same two nets (generation-0 Glorot weights, two seeds), 11x11 with 4 snakes.

    python tools/arena_time.py [games ...] [--pairs 3] [--blocks 4] [--log profiles/arena_ab.log] [--record K]

For every game count (default 300 and 4096) the two forms alternate inside this one process, `--pairs` times; a line per
match with its turns, seconds and ms per turn, then the medians.  The winners of the two forms are compared: they play the
same match.
--record K: instead, what a replay recorder costs: Arena.match of the same two nets without a recorder and with one on the first K
games (Arena.record), alternating inside this one process on the same start boards, `--pairs` times; ms per turn of both, the
medians and the added time per turn.  The recorded match's winners and frame counts are checked against the plain one's."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "alphasnake-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("games", nargs="*", type=int, default=[300, 4096])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--log", default=None)
    ap.add_argument("--record", type=int, default=None, metavar="K")
    a = ap.parse_args()
    import numpy as np
    import torch
    from snake_engine.net import glorot_uniform_weights
    from utils.alpha_nnet import AlphaNNet
    from utils.pit_agent import Agent
    from utils.pit_mp_game_runner import MPGameRunner

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nets = [AlphaNNet(input_shape=(21, 21, 3), _weights=glorot_uniform_weights((21, 21, 3), a.blocks, seed=s)) for s in (1, 2)]
    alice, bob = Agent(nets[0]), Agent(nets[1])

    def play(form, n, start):
        np.random.seed(0)
        gr = MPGameRunner(11, 11, 4, 1, n, seed=7)
        if start is None:
            start = gr.engine.export()
        else:
            gr.engine.import_states(start)
            for g in gr.games.values():
                g._dirty()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        winners = getattr(gr, form)(alice, bob, 1)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lengths = np.array([s.counters[5] for s in gr.engine.export()])
        return winners, int(lengths.max()), dt, start

    say(f"arena_time: 11x11, 4 snakes (1 v 3), {a.blocks}-block Glorot nets (seeds 1, 2), {a.pairs} alternating pairs per size, "
        f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}, "
        f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs), ROCm / HIP {torch.version.hip}, torch {torch.__version__}")
    def write_log():
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, "w") as f:
                f.write("\n".join(lines) + "\n")

    def match(n, start, record):
        from snake_engine.arena import Arena
        arena = Arena(11, 11, 4, 1, n, seed=7)
        if start is None:
            start = arena.engine.export()
        else:
            arena.import_states(start)
        rep = arena.record(range(min(record, n))) if record else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = arena.match(nets[0], nets[1], 1)
        torch.cuda.synchronize()
        return res, time.perf_counter() - t0, start, rep

    if a.record is not None:
        say(f"arena_time --record {a.record}: Arena.match greedy against greedy, 11x11, 4 snakes (1 v 3), {a.blocks}-block Glorot nets, "
            f"{a.pairs} alternating pairs per size, {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), "
            f"ROCm / HIP {torch.version.hip}, torch {torch.__version__}")
        match(64, None, 0)                                 # first launches, plans and range-guard scales settle outside the timing
        match(64, None, min(a.record, 64))
        for n in a.games:
            start, per = None, {"plain": [], "recorded": []}
            for k in range(a.pairs):
                won = {}
                for form, record in (("plain", 0), ("recorded", a.record)):
                    res, dt, start, rep = match(n, start, record)
                    won[form] = res.winners.tolist()
                    per[form].append(dt / res.turns * 1e3)
                    say(f"games {n:5d} pair {k} {form:8s}: {res.turns:4d} turns, {dt:7.3f} s, {dt / res.turns * 1e3:8.3f} ms per turn")
                    if rep is not None:
                        ok = all(len(rep.frames(g)) == 2 * res.lengths[g] for g in rep.games.tolist())
                        say(f"games {n:5d} pair {k} recorded {len(rep.games)} games, the log doubled {rep.grown} times, frame counts right: {ok}")
                say(f"games {n:5d} pair {k} winners identical: {won['plain'] == won['recorded']}")
            p, r = statistics.median(per["plain"]), statistics.median(per["recorded"])
            say(f"games {n:5d} median ms per turn: plain {p:.3f}, recorded {r:.3f}, added {(r - p) * 1e3:.1f} us per turn")
        write_log()
        return

    _, _, _, _ = play("run_device", 64, None)              # first launches, plans and range-guard scales settle outside the timing
    _, _, _, _ = play("run", 64, None)
    for n in a.games:
        start, per = None, {"run": [], "run_device": []}
        for k in range(a.pairs):
            won = {}
            for form in ("run", "run_device"):
                won[form], turns, dt, start = play(form, n, start)
                per[form].append(dt / turns * 1e3)
                say(f"games {n:5d} pair {k} {form:10s}: {turns:4d} turns per match, {dt:7.3f} s, {dt / turns * 1e3:8.3f} ms per turn")
            same = won["run"] == won["run_device"]
            say(f"games {n:5d} pair {k} winners identical: {same}")
        h, d = statistics.median(per["run"]), statistics.median(per["run_device"])
        say(f"games {n:5d} median ms per turn: run {h:.3f}, run_device {d:.3f}, ratio {h / d:.2f}x")
    write_log()


if __name__ == "__main__":
    main()
