"""The float32 tower layer (csrc/net.hip: k_conv3x3_f32<BK, WAVES_PER_SIMD>, the implicit GEMM, and k_conv3x3_wino_f32<NW>, Winograd
F(2x2, 3x3)) on the test side: its definition in float64, the shapes tests/helpers/conv_f32_runner.py runs and why, the inputs it
runs them on, and what the launchers read from the environment.  NumPy only.

    layer(x, w_hwio, scale, shift, res, relu)   out = [relu]( conv3x3_same(x, w) * scale + shift [+ res] ), NHWC float64, the
                                                convolution as nine shifted [pixels, 128] @ [128, 128] products (no library's)
    constants()                                 CV_BM, WG_TB, and for each launcher the environment variable it reads once per process,
                                                its default, the value the launcher compares with and the kernel on either side
    CONFIGS                                     the two processes of tests/test_conv_f32_forms_gpu.py
    CASES                                       (n, H, W), each with what it reaches; tests/test_conv_f32_ref_cpu.py holds the table
                                                to its comments with CV_BM and WG_TB as the source has them
    inputs / integer_inputs / one_hot_weights   float32 arrays

What constants() is for: SNK_CONV_BK and SNK_WINO_WAVES select two of the four compiled kernels, and nothing a kernel computes says
which instance ran.  The CPU test asserts that the names, the defaults and the comparisons are the ones CONFIGS relies on, so a
renamed variable or a changed default fails there instead of letting the GPU test run the default kernels twice.  A rewritten
dispatch is not seen: whoever changes it changes the expressions below with it.
"""
import os
import re

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alphasnake-zero_amd", "csrc", "net.hip")
C = 128

# configuration -> the environment of its process (the variables not named are unset)
CONFIGS = {"default": {},                                              # k_conv3x3_f32<16, 3> and k_conv3x3_wino_f32<8>
           "bk32_nw4": {"SNK_CONV_BK": "32", "SNK_WINO_WAVES": "4"}}   # k_conv3x3_f32<32, 2> and k_conv3x3_wino_f32<4>
ENV_NAMES = ("SNK_CONV_BK", "SNK_WINO_WAVES", "SNK_CONV_ALGO")

# (n, H, W): pixels = n H W in blocks of CV_BM = 128 (direct), tiles = n ceil(H / 2) ceil(W / 2) in blocks of WG_TB = 32 (Winograd)
CASES = [(1, 1, 1),       # one pixel, one tile, every tap but the centre outside
         (3, 1, 5),       # H = 1
         (2, 5, 1),       # W = 1
         (3, 3, 2),       # W = 2: one tile column, none clipped in x
         (2, 4, 7),       # H even, W odd
         (2, 7, 4),       # H odd, W even
         (2, 8, 8),       # 128 pixels: exactly one direct block; 32 tiles: exactly one Winograd block; no clipped tile
         (3, 8, 16),      # 384 pixels, 96 tiles: exact multiples with several blocks, image borders inside blocks
         (1, 3, 43),      # 129 pixels: a second direct block with one live row
         (1, 127, 1),     # 127 pixels; 64 tiles
         (1, 2, 66),      # 33 tiles: a second Winograd block with one live tile
         (1, 2, 62),      # 31 tiles
         (3, 7, 9),       # 63 pixels, 20 tiles per image: every block spans images; the tails are 61 rows and 28 tiles
         (5, 21, 21), (3, 13, 13), (2, 37, 37)]      # the three canvases


def pixels(n, H, W):
    return n * H * W


def tiles(n, H, W):
    return n * ((H + 1) // 2) * ((W + 1) // 2)


def constants(path=SRC):
    """{CV_BM, WG_TB: int; BK, NW: {env, default, switch, kernel_if_equal, kernel_else}} read from the source: `switch` is the value
    the launcher compares its variable with, kernel_if_equal / kernel_else the template arguments it launches on either side"""
    with open(path) as f:
        text = f.read()
    out = {}
    for name in ("CV_BM", "WG_TB"):
        m = re.findall(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    m = re.findall(r'if \(variant < 0\) \{ const char \*v = getenv\("(\w+)"\); variant = v \? atoi\(v\) : (\d+); \}\s*'
                   r"if \(variant == (\d+)\) k_conv3x3_f32<(\d+), (\d+)><<<[^;]*;\s*else k_conv3x3_f32<(\d+), (\d+)><<<", text)
    assert len(m) == 1, m
    e, d, s, a0, a1, b0, b1 = m[0]
    out["BK"] = {"env": e, "default": int(d), "switch": int(s), "kernel_if_equal": (int(a0), int(a1)), "kernel_else": (int(b0), int(b1))}
    m = re.findall(r'if \(nw < 0\) \{ const char \*v = getenv\("(\w+)"\); nw = v \? atoi\(v\) : (\d+); \}\s*'
                   r"if \(nw == (\d+)\) k_conv3x3_wino_f32<(\d+)><<<[^;]*;\s*else k_conv3x3_wino_f32<(\d+)><<<", text)
    assert len(m) == 1, m
    e, d, s, a, b = m[0]
    out["NW"] = {"env": e, "default": int(d), "switch": int(s), "kernel_if_equal": (int(a),), "kernel_else": (int(b),)}
    return out


def kernels(config, c=None):
    """((BK, WAVES_PER_SIMD), (NW,)): the instances the two launchers start in a process with CONFIGS[config] as its environment"""
    c = c or constants()
    got = []
    for key in ("BK", "NW"):
        k = c[key]
        v = CONFIGS[config].get(k["env"])
        v = k["default"] if v is None else int(v)
        got.append(k["kernel_if_equal"] if v == k["switch"] else k["kernel_else"])
    return tuple(got)


def layer(x, w_hwio, scale, shift, res=None, relu=True):
    """x, res [n, H, W, 128], w_hwio [3, 3, 128 cin, 128 cout], scale, shift [128] -> float64 [n, H, W, 128]"""
    x = np.asarray(x, np.float64)
    w = np.asarray(w_hwio, np.float64)
    n, H, W, ci = x.shape
    co = w.shape[3]
    xp = np.zeros((n, H + 2, W + 2, ci))
    xp[:, 1:H + 1, 1:W + 1] = x
    out = np.zeros((n * H * W, co))
    for a in range(3):
        for b in range(3):
            out += np.ascontiguousarray(xp[:, a:a + H, b:b + W]).reshape(n * H * W, ci) @ w[a, b]
    out = out.reshape(n, H, W, co) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    if res is not None:
        out = out + np.asarray(res, np.float64)
    if relu:
        out = np.maximum(0.0, out)
    return out


def inputs(case, seed, mag=1.0):
    """(x, w, scale, shift, res) as tests/test_net_gpu.py::test_conv3x3_layer draws them: x = randn * mag, w = randn * 0.05,
    scale = rand + 0.5, shift = randn * 0.1 * mag, res = randn * mag"""
    n, H, W = case
    rng = np.random.RandomState(seed)
    x = rng.randn(n, H, W, C) * mag
    w = rng.randn(3, 3, C, C) * 0.05
    scale = rng.rand(C) + 0.5
    shift = rng.randn(C) * 0.1 * mag
    res = rng.randn(n, H, W, C) * mag
    return tuple(np.ascontiguousarray(t, np.float32) for t in (x, w, scale, shift, res))


def integer_inputs(case, seed):
    """x, res: integers in [-4, 4]; w in {-1, 0, 1}; scale in {0.5, 1, 2}; shift: an integer in [-3, 3].  Every intermediate of both
    forms is then a multiple of 1/4 below 2^22 in magnitude -- direct: sums of at most 1152 integers of magnitude <= 4; Winograd:
    U = G g G^T in quarters up to 2.25, V = B^T d B integers up to 16, their sums over 128 channels up to 4608, A^T M A up to nine of
    those; the epilogue halves at most -- so float32 is exact in any order of accumulation and the output is the float64 model's."""
    n, H, W = case
    rng = np.random.RandomState(seed)
    x = rng.randint(-4, 5, size=(n, H, W, C))
    w = rng.randint(-1, 2, size=(3, 3, C, C))
    scale = np.array([0.5, 1.0, 2.0])[rng.randint(0, 3, size=C)]
    shift = rng.randint(-3, 4, size=C)
    res = rng.randint(-4, 5, size=(n, H, W, C))
    return tuple(np.ascontiguousarray(t, np.float32) for t in (x, w, scale, shift, res))


def one_hot_weights(tap):
    """w[tap][c][c] = 1, everything else 0: the layer then returns its input shifted by the tap"""
    w = np.zeros((3, 3, C, C), np.float32)
    w[tap // 3, tap % 3, np.arange(C), np.arange(C)] = 1.0
    return w
