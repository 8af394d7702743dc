"""The MX-FP8 tower (SNK_CONV_ALGO=mxfp8) without a GPU: its five entry points in the C ABI and the ctypes bindings, and the
NumPy restatement of the quantization rule (tests/mxfp8_ref.py) on hand-worked blocks."""
import os
import re

import numpy as np

import mxfp8_ref as mx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("snk_conv3x3_prepare_weights_mxfp8", "snk_conv3x3_bn_mxfp8_act16", "snk_conv3x3_bn_mxfp8_act16_rect",
                "snk_conv3x3_bn_mxfp8_act16_head", "snk_mxfp8_quantize_bf16")


def test_entry_points_declared_and_bound():
    from snake_engine import _lib
    hdr = open(os.path.join(REPO, "include", "snake_engine.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.PROTOTYPES, name
    assert _lib.ABI_VERSION == 113 == int(re.search(r"#define SNK_ABI_VERSION (\d+)", hdr).group(1))
    # the bf16 tower's argument lists, so that net.py's call sites take either
    P = _lib.PROTOTYPES
    assert P["snk_conv3x3_bn_mxfp8_act16"] == P["snk_conv3x3_bn_bf16_act16"]
    assert P["snk_conv3x3_bn_mxfp8_act16_rect"] == P["snk_conv3x3_bn_bf16_act16_rect"]
    assert P["snk_conv3x3_bn_mxfp8_act16_head"] == P["snk_conv3x3_bn_bf16_act16_head"]
    assert P["snk_conv3x3_prepare_weights_mxfp8"] == P["snk_conv3x3_prepare_weights_bf16"]


def test_net_accepts_the_form(monkeypatch):
    from snake_engine import net
    src = open(net.__file__).read()
    assert '"mxfp8"' in src and "snk_conv3x3_bn_mxfp8_act16_head" in src


def _block(*vals):
    b = np.zeros(32, np.float32)
    b[:len(vals)] = vals
    return b


def _q(b):
    c, s = mx.quantize_blocks(b[None])
    return c[0], int(s[0])


def test_all_zeros():
    c, s = _q(np.zeros(32, np.float32))
    assert s == 0 and not c.any()                    # E = -127


def test_amax_exactly_448_times_a_power_of_two():
    for k, sbyte in ((0, 127), (3, 130), (-10, 117)):
        c, s = _q(_block(448.0 * 2.0 ** k, -448.0 * 2.0 ** k, 1.0 * 2.0 ** k))
        assert s == sbyte                             # E = k: amax * 2^-E = 448 exactly, no saturation
        assert c[0] == 0x7E and c[1] == 0xFE and c[2] == 0x38      # 448, -448, 1.0 (exponent 7 = bias, mantissa 0)


def test_amax_just_above_a_power_of_two():
    c, s = _q(_block(1.0078125, 0.5))                # 1 + 2^-7: E = -8, 258 rounds to 256 (next code 288)
    assert s == 119 and c[0] == 0x78 and c[1] == 0x70
    c, s = _q(_block(451.5, 3.0))                    # just above 1.75 * 2^8: E = 1 (E = 0 would give 451.5 > 448)
    assert s == 128 and c[0] == 0x76 and c[1] == 0x3C           # 225.75 -> 224 (codes 224 / 240), 1.5
    c, s = _q(_block(448.0))                         # 1.75 * 2^8 itself stays at E = 0
    assert s == 127 and c[0] == 0x7E


def test_values_that_go_subnormal():
    c, s = _q(_block(448.0, 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -10, 0.75 * 2.0 ** -9, 7 * 2.0 ** -9, 2.0 ** -6, -5 * 2.0 ** -9))
    assert s == 127
    # 2^-9 = smallest subnormal; 1.5 x it ties -> even (2); 0.5 x it ties -> even (0); 0.75 x it -> 1; 7 x it = largest
    # subnormal; 2^-6 = smallest normal
    assert list(c[1:8]) == [0x01, 0x02, 0x00, 0x01, 0x07, 0x08, 0x85]


def test_ties_round_to_even():
    c, s = _q(_block(448.0, 1.0625, 1.1875, -1.0625, 240.0 + 8.0, 208.0 + 8.0))
    assert s == 127
    # 1 + 1/16 lies halfway between 1.0 (0x38) and 1.125 (0x39): even 0x38; 1 + 3/16 between 0x39 and 1.25 (0x3A): 0x3A;
    # 248 between 240 (0x77) and 256 (0x78): 0x78; 216 between 208 (0x75) and 224 (0x76): 0x76
    assert list(c[1:6]) == [0x38, 0x3A, 0xB8, 0x78, 0x76]


def test_tiny_amax_clamps_the_exponent():
    c, s = _q(_block(2.0 ** -135, -(2.0 ** -136), 2.0 ** -149))
    assert s == 0                                    # E would be -143: clamped to -127
    # 2^-135 * 2^127 = 2^-8 = two subnormal steps; -2^-9 -> 0x81; 2^-149 * 2^127 = 2^-22 -> 0
    assert c[0] == 0x02 and c[1] == 0x81 and c[2] & 0x7F == 0


def test_dequantize_round_trip_and_no_saturation():
    rng = np.random.RandomState(3)
    x = (rng.randn(500, 32) * np.exp2(rng.randint(-40, 40, size=(500, 1)))).astype(np.float32)
    c, s = mx.quantize_blocks(x)
    d = mx.dequantize_blocks(c, s)
    assert np.array_equal(d, mx.mx_round(x))
    amax = np.abs(x).max(axis=1)
    assert ((c & 0x7F) != 0x7F).all()                                     # no NaN code
    assert (np.abs(d).max(axis=1) <= amax * (1 + 2.0 ** -4)).all()        # the block maximum moves by at most half a step
    rel = np.abs(d - x) / amax[:, None]
    assert rel.max() <= 2.0 ** -5 * 448 / 224                             # half a step at 224 .. 448, relative to amax
