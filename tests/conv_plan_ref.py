"""Plain-Python restatement of conv_f16s_plan, the planning loop of conv_f16s_launch (csrc/conv_split.hip): how one host routine cuts the images of
every tower convolution -- inference and training -- into blocks of M tiles.

    plan(n, H, W, a16) -> Plan(n_blk, tiles_base, tiles_rem, NI)

  T          ceil(H W / 32) M tiles of 32 pixels per image
  n_blk      blocks per image: the smallest count from ceil(T / 8) on whose largest block (its pixels' rows plus one row above and
             below) fits the LDS buffer and the staging items of the frame -- the float32 frame (a16 = False: the split f16s form,
             the single-pass f16 form with float32 tensors, every training mode) or the 16-bit frame (a16 = True: f16 / bf16 / MX-FP8
             activations in HBM)
  re-cut     a batch of at most SNK_CONV_FINE_MAX (40) images whose grid would have fewer than 512 blocks is cut finer, to about 512
  NI         ceil(T / n_blk): the tile count the kernel is compiled for (k_conv3x3_f16s<NI, ...>)
  block b    of an image has tiles_base + (b < tiles_rem) tiles, so with tiles_rem > 0 the blocks b >= tiles_rem run NI - 1 tiles

What this catches, and what it does not: the loop below was written from the C++ by hand and the constants are read from the source
with a regular expression.  tests/test_conv_tiles_cpu.py asserts the plans of the shapes tests/test_conv_tiles_gpu.py runs, so a
CHANGED CONSTANT (HS_NPB, HS_NST, HS_NST16, HS_BUF16, HS_LDP, HS_GAP16_FULL, the SNK_CONV_FINE_MAX default) that moves one of those
shapes to another kernel body fails there instead of silently leaving a body untested.  A REWRITTEN LOOP in conv_f16s_plan is not
seen: this file would go on stating the old one.  Whoever changes the loop changes this restatement with it.
"""
import os
import re
from collections import namedtuple

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alphasnake-zero_amd", "csrc", "conv_split.hip")

Plan = namedtuple("Plan", "n_blk tiles_base tiles_rem NI")

_NAMES = ("HS_NPB", "HS_NST", "HS_NST16", "HS_BUF16", "HS_LDP", "HS_GAP16_FULL")


def constants(path=SRC):
    """{name: int} of the #defines the loop uses, and FINE_MAX: the default of SNK_CONV_FINE_MAX"""
    with open(path) as f:
        text = f.read()
    out = {}
    for name in _NAMES:
        m = re.findall(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    m = re.findall(r'getenv\("SNK_CONV_FINE_MAX"\)\s*\?\s*atoi\(getenv\("SNK_CONV_FINE_MAX"\)\)\s*:\s*(\d+)\s*;', text)
    assert len(m) == 1, m
    out["FINE_MAX"] = int(m[0])
    return out


def plan(n, H, W, a16, c=None):
    """the plan of a launch of n images of H x W pixels; a16: the 16-bit frame.  Raises ValueError where the launch is refused."""
    c = c or constants()
    if not (n >= 1 and H >= 1 and W >= 3):
        raise ValueError("bad shape")
    P = W + 1
    nst_px = 64 * (c["HS_NST16"] if a16 else c["HS_NST"])
    T = (H * W + 31) // 32
    n_blk = (T + 7) // 8
    while True:
        tiles_max = (T + n_blk - 1) // n_blk
        rows_out = min((tiles_max * 32 + W - 2) // W + 1, H)
        if a16:
            fits = (rows_out + 2) * (W * c["HS_LDP"] + c["HS_GAP16_FULL"]) <= c["HS_BUF16"]
        else:
            fits = (rows_out + 2) * P + 1 <= c["HS_NPB"]
        fits = fits and min(rows_out + 2, H) * W <= nst_px
        if fits or tiles_max == 1:
            break
        n_blk += 1
    if not fits:
        raise ValueError("width not supported")
    if n <= c["FINE_MAX"] and n * n_blk < 512:
        n_blk = min(T, max(n_blk, (512 + n - 1) // n))
        tiles_max = (T + n_blk - 1) // n_blk
    return Plan(n_blk, T // n_blk, T % n_blk, tiles_max)


def block_tiles(p):
    """tile counts of an image's blocks, in block order"""
    return [p.tiles_base + (b < p.tiles_rem) for b in range(p.n_blk)]
