"""tests/conv_f32_ref.py checked without a GPU: the float64 model against torch's float64 convolution, the case table against its
comments, constants() against the present csrc/net.hip, and the claim tests/helpers/conv_f32_runner.py rests its bit-for-bit
assertions on: integer_inputs make F(2x2, 3x3) exact in float32."""
import numpy as np
import pytest

import conv_f32_ref as R


def _torch_layer(x, w, scale, shift, res, relu):
    import torch
    t = [torch.from_numpy(np.asarray(a, np.float64)) for a in (x, w, scale, shift, res)]
    ref = torch.nn.functional.conv2d(t[0].permute(0, 3, 1, 2), t[1].permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    ref = ref * t[2] + t[3]
    if res is not None:
        ref = ref + t[4]
    if relu:
        ref = ref.clamp_min(0)
    return ref.numpy()


@pytest.mark.parametrize("case", [(3, 7, 9), (2, 4, 7), (1, 1, 1)])
def test_layer_is_the_convolution(case):
    x, w, scale, shift, res = R.inputs(case, 11)
    for relu in (False, True):
        for r in (None, res):
            got = R.layer(x, w, scale, shift, r, relu)
            ref = _torch_layer(x, w, scale, shift, res if r is not None else None, relu)
            assert got.dtype == np.float64 and got.shape == ref.shape
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (case, relu, r is not None)


def test_constants_and_configurations():
    c = R.constants()
    assert (c["CV_BM"], c["WG_TB"]) == (128, 32)
    assert c["BK"] == {"env": "SNK_CONV_BK", "default": 16, "switch": 32, "kernel_if_equal": (32, 2), "kernel_else": (16, 3)}
    assert c["NW"] == {"env": "SNK_WINO_WAVES", "default": 8, "switch": 8, "kernel_if_equal": (8,), "kernel_else": (4,)}
    # the two processes of the GPU test launch four different kernels, and set nothing but what ENV_NAMES clears
    assert R.kernels("default", c) == ((16, 3), (8,))
    assert R.kernels("bk32_nw4", c) == ((32, 2), (4,))
    assert all(set(env) <= set(R.ENV_NAMES) for env in R.CONFIGS.values())


def test_case_table_reaches_what_it_says():
    c = R.constants()
    assert len(set(R.CASES)) == len(R.CASES) == 16
    px = {case: R.pixels(*case) for case in R.CASES}
    tl = {case: R.tiles(*case) for case in R.CASES}
    assert {0, 1, c["CV_BM"] - 1} <= {v % c["CV_BM"] for v in px.values()}
    assert {0, 1, c["WG_TB"] - 1} <= {v % c["WG_TB"] for v in tl.values()}
    assert {(H % 2, W % 2) for _, H, W in R.CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(H == 1 for _, H, W in R.CASES) and any(W == 1 for _, H, W in R.CASES) and any(W == 2 for _, H, W in R.CASES)
    # the comments of the table, one by one
    assert (px[(1, 1, 1)], tl[(1, 1, 1)]) == (1, 1)
    assert (px[(2, 8, 8)], tl[(2, 8, 8)]) == (c["CV_BM"], c["WG_TB"])
    assert (px[(3, 8, 16)], tl[(3, 8, 16)]) == (3 * c["CV_BM"], 3 * c["WG_TB"])
    assert px[(1, 3, 43)] == c["CV_BM"] + 1
    assert (px[(1, 127, 1)], tl[(1, 127, 1)]) == (c["CV_BM"] - 1, 2 * c["WG_TB"])
    assert tl[(1, 2, 66)] == c["WG_TB"] + 1 and tl[(1, 2, 62)] == c["WG_TB"] - 1
    assert (px[(3, 7, 9)], tl[(3, 7, 9)]) == (3 * 63, 3 * 20)
    assert 63 % c["CV_BM"] and c["CV_BM"] % 63 and 20 % c["WG_TB"] and c["WG_TB"] % 20      # no block boundary on an image boundary
    assert (px[(3, 7, 9)] % c["CV_BM"], tl[(3, 7, 9)] % c["WG_TB"]) == (61, 28)
    assert [s for s in R.CASES if s[1] == s[2] and s[1] in (21, 13, 37)] == [(5, 21, 21), (3, 13, 13), (2, 37, 37)]
    assert max(px.values()) == px[(2, 37, 37)]


def test_one_hot_weights_shift_the_input():
    x = R.inputs((2, 4, 7), 5)[0]
    one, zero = np.ones(R.C), np.zeros(R.C)
    for tap in range(9):
        w = R.one_hot_weights(tap)
        assert w.sum() == R.C and w[tap // 3, tap % 3].trace() == R.C
        dy, dx = tap // 3 - 1, tap % 3 - 1
        want = np.zeros(x.shape)
        want[:, max(0, -dy):4 - max(0, dy), max(0, -dx):7 - max(0, dx)] = x[:, max(0, dy):4 + min(0, dy), max(0, dx):7 + min(0, dx)]
        got = R.layer(x, w, one, zero, None, False)
        assert np.array_equal(got, want) and not np.signbit(got[got == 0]).any()


# F(2x2, 3x3) as csrc/net.hip states it: Y = A^T [ (G g G^T) . (B^T d B) ] A
G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]])
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float32)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float32)


def winograd_f32(x, w, scale, shift, res, relu):
    """the layer by F(2x2, 3x3) with every operation rounded to float32 (U = G g G^T rounded once from float64, as k_wino_weights
    does); the sums over the transforms' terms and over the input channels in NumPy's order"""
    f = np.float32
    n, H, W, C = x.shape
    TY, TX = (H + 1) // 2, (W + 1) // 2
    U = np.einsum("xa,abio,nb->xnio", G, w.astype(np.float64), G).astype(f)                 # [4][4][cin][cout]
    xp = np.zeros((n, 2 * TY + 2, 2 * TX + 2, C), f)
    xp[:, 1:H + 1, 1:W + 1] = x
    d = np.stack([np.stack([xp[:, i:i + 2 * TY:2, j:j + 2 * TX:2] for j in range(4)]) for i in range(4)])   # [4][4][n][TY][TX][C]
    assert d.dtype == f
    t = np.zeros_like(d)
    for i in range(4):                                                                      # B^T d
        for k in range(4):
            if BT[i, k]:
                t[i] = t[i] + BT[i, k] * d[k]
    V = np.zeros_like(d)
    for j in range(4):                                                                      # (B^T d) B
        for k in range(4):
            if BT[j, k]:
                V[:, j] = V[:, j] + t[:, k] * BT[j, k]
    assert V.dtype == f
    M = np.matmul(V.reshape(4, 4, n * TY * TX, C), U)                                       # float32 accumulation over cin
    assert M.dtype == f
    s = np.zeros((2, 4) + M.shape[2:], f)
    for a in range(2):                                                                      # A^T M
        for k in range(4):
            if AT[a, k]:
                s[a] = s[a] + AT[a, k] * M[k]
    Y = np.zeros((2, 2) + M.shape[2:], f)
    for b in range(2):                                                                      # (A^T M) A
        for k in range(4):
            if AT[b, k]:
                Y[:, b] = Y[:, b] + s[:, k] * AT[b, k]
    y = Y.reshape(2, 2, n, TY, TX, C).transpose(2, 3, 0, 4, 1, 5).reshape(n, 2 * TY, 2 * TX, C)[:, :H, :W]
    v = y * scale.astype(f) + shift.astype(f)
    if res is not None:
        v = v + res
    if relu:
        v = np.maximum(f(0), v)
    assert v.dtype == f
    return v


@pytest.mark.parametrize("case", [(3, 7, 9), (2, 8, 8)])
def test_integer_inputs_make_float32_winograd_exact(case):
    x, w, scale, shift, res = R.integer_inputs(case, 1000 * case[1] + case[2])
    assert set(np.unique(x)) == set(range(-4, 5)) and set(np.unique(w)) == {-1, 0, 1}
    assert set(np.unique(scale)) == {0.5, 1.0, 2.0} and set(np.unique(shift)) <= set(range(-3, 4))
    ref = R.layer(x, w, scale, shift, res, True)
    assert np.array_equal(ref, ref.astype(np.float32).astype(np.float64))                   # the model's values are float32 numbers
    assert not np.signbit(ref[ref == 0]).any()                                              # and its zeros are +0
    assert np.abs(ref).max() < 2.0 ** 22 and (ref > 0).any() and (ref == 0).any()
    got = winograd_f32(x, w, scale, shift, res, True)
    assert np.array_equal(got.view(np.int32), ref.astype(np.float32).view(np.int32))
    # the same emulation is NOT exact on random floats: the assertion above is about the inputs, not about the emulation
    x, w, scale, shift, res = R.inputs(case, 3)
    ref = R.layer(x, w, scale, shift, res, True)
    got = winograd_f32(x, w, scale, shift, res, True)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert 0 < err <= 2e-5, err
