"""share of root moves on which two tower forms agree: the same boards (same runner seed), the same agent seed, one greedy root
turn (training=False: argmax of Q) per form -- informational:
    mx_agreement.py [form_a] [form_b] [games] [breadth]      (default bf16 mxfp8 512 16; 19x19 boards, 8 snakes, 10 blocks)"""
import os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "alphasnake-zero_amd")]
import numpy as np
from snake_engine import net
from utils.agent import Agent
from utils.alpha_nnet import AlphaNNet
from utils.mp_game_runner import MPGameRunner

forms = sys.argv[1:3] if len(sys.argv) > 2 else ["bf16", "mxfp8"]
games = int(sys.argv[3]) if len(sys.argv) > 3 else 512
breadth = int(sys.argv[4]) if len(sys.argv) > 4 else 16
H = W = 19
ws = net.glorot_uniform_weights((2 * H - 1, 2 * W - 1, 3), blocks=10, seed=0)
MPGameRunner.verbose, MPGameRunner.init = False, "device"
out = {}
for form in forms:
    os.environ["SNK_CONV_ALGO"] = form
    gr = MPGameRunner(H, W, 8, 1, games, seed=2024)
    agent = Agent(AlphaNNet(input_shape=(2 * H - 1, 2 * W - 1, 3), _weights=ws), 2, False, 8, breadth, seed=7)
    seen = []
    mm = agent.make_moves

    def spy(g_, ids, mm=mm, seen=seen):
        r = mm(g_, ids)
        seen.append((list(map(tuple, np.asarray(ids).tolist())), np.asarray(r).copy()))
        return r
    agent.make_moves = spy
    gr.run(agent, max_turns=1)
    out[form] = seen[0]
(ia, ma), (ib, mb) = out[forms[0]], out[forms[1]]
assert ia == ib, "the two runs saw different root rows"
print(f"{forms[0]} vs {forms[1]}: {games} games (19x19, 8 snakes), breadth {breadth}, {len(ma)} root rows: "
      f"moves agree on {np.mean(ma == mb):.4f}")
