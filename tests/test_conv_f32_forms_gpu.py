"""The float32 forms of the 3x3 tower layer (csrc/net.hip: k_conv3x3_f32<16, 3> and <32, 2>, k_conv3x3_wino_f32<8> and <4>) against
the float64 model tests/conv_f32_ref.py.  The cases, tolerances and exact properties are in tests/helpers/conv_f32_runner.py.
SNK_CONV_BK and SNK_WINO_WAVES are read once per process, so each configuration is one fresh child process, run once per module, one
after the other; a child that fails fails the test with the tail of its output, nothing is retried."""
import functools
import os
import subprocess
import sys

import pytest

import conv_f32_ref as R

pytestmark = pytest.mark.gpu

RUNNER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "conv_f32_runner.py")


@functools.lru_cache(maxsize=None)
def child(config):
    env = {k: v for k, v in os.environ.items() if k not in R.ENV_NAMES}
    env.update(R.CONFIGS[config])
    return subprocess.run([sys.executable, RUNNER, config], capture_output=True, text=True, env=env, timeout=300)


def digests(config):
    out = child(config)
    assert out.returncode == 0, f"exit status {out.returncode}\n{out.stdout[-1500:]}\n{out.stderr[-3000:]}"
    d = dict(line.split()[1:3] for line in out.stdout.splitlines() if line.startswith("digest "))
    assert set(d) == {"direct", "winograd"} and all(len(v) == 64 for v in d.values()), d
    return d


@pytest.mark.parametrize("config", list(R.CONFIGS))
def test_forms(config):
    out = child(config)
    assert out.returncode == 0, f"exit status {out.returncode}\n{out.stdout[-1500:]}\n{out.stderr[-3000:]}"
    assert out.stdout.strip().endswith(f"conv f32 forms {config}: ok"), out.stdout[-1500:]


def test_bk32_is_another_kernel():
    """SNK_CONV_BK=32 reached the launcher: BK changes the order in which the (tap, channel chunk) products are accumulated -- nine
    taps of 16 channels, then the next 16, against nine taps of 32 -- so the same bits over the 282 240 outputs of the random
    (5, 21, 21) layer would mean that the variable was not read and k_conv3x3_f32<16, 3> ran twice.
    There is no such check for SNK_WINO_WAVES: NW moves positions between wavefronts, not the order in which a position's input
    channels are accumulated, so k_conv3x3_wino_f32<4> and <8> may well give the same bits.  That the second child ran <4> rests on
    the runner's assertion about its environment and on tests/test_conv_f32_ref_cpu.py::test_constants_and_configurations, which
    reads the variable's name, its default and the launcher's comparison from the source."""
    a, b = digests("default"), digests("bk32_nw4")
    assert a["direct"] != b["direct"]
