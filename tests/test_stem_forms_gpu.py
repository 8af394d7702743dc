"""Every launch form of the inference stem (csrc/net.hip: k_stem_conv_mfma in its full-canvas, sub-rectangle, f16 / bf16-output and
raw forms, and the k_stem_conv fallback) against the float64 model tests/stem_head_ref.py.  The cases, tolerances and exact
properties are in tests/helpers/stem_forms_runner.py.  SNK_STEM, SNK_STEM_GRID and SNK_STEM_GROUP are read once per process, so each
configuration is one fresh child process; a child that fails fails the test with the tail of its output, nothing is retried."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

RUNNER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "stem_forms_runner.py")
CONFIGS = {"default": {},                                                  # G from the LDS footprint, 512 persistent blocks
           "group1": {"SNK_STEM_GROUP": "1"},                              # one image per block iteration
           "group2_grid3": {"SNK_STEM_GROUP": "2", "SNK_STEM_GRID": "3"}}  # the full-canvas float32 entry on 3 blocks


@pytest.mark.parametrize("config", list(CONFIGS))
def test_stem_forms(config):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SNK_STEM")}
    env.update(CONFIGS[config])
    out = subprocess.run([sys.executable, RUNNER, config], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, f"exit status {out.returncode}\n{out.stdout[-1500:]}\n{out.stderr[-3000:]}"
    assert out.stdout.strip().endswith(f"stem forms {config}: ok"), out.stdout[-1500:]
