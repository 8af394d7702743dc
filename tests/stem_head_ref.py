"""The first and last kernels of a Q-net evaluation (csrc/net.hip: the stem's entry points snk_stem_conv_*, the head's snk_head_f32 and
snk_head_dense_f32) as plain NumPy float64 functions, written from the comments of that file and sharing no code with it.
tests/test_stem_head_ref_cpu.py holds these functions against float64 torch and hand-written cases; tests/test_stem_forms_gpu.py
and tests/test_head_forms_gpu.py hold the kernels against these functions.

Layouts as the kernels have them: x [n][H][W][3], stem kernel [3][3][3][128] (kh, kw, cin, cout), activations [n][H][W][128],
Dense kernels (in, out), the obstacle mask one byte per (state, move)."""
import numpy as np

C = 128                              # tower channels
LDS_64K = 64 * 1024
X_SAT = 65504.0 / 1024.0             # the MFMA stem carries x * 2^10 as f16 hi + lo: inputs saturate at +-63.96875


def f64(a):
    return np.asarray(a, dtype=np.float64)


def stem(x, w, scale, shift, raw=False):
    """3x3 'same' cross-correlation 3 -> 128 as nine shifted adds over a zero-padded copy, then max(. * scale + shift, 0)
    (raw: the bare convolution, scale and shift unused)"""
    x, w = f64(x), f64(w)
    n, H, W, cin = x.shape
    assert w.shape == (3, 3, cin, C)
    xp = np.zeros((n, H + 2, W + 2, cin))
    xp[:, 1:H + 1, 1:W + 1] = x
    out = np.zeros((n, H, W, C))
    for dy in range(3):
        for dx in range(3):
            out += xp[:, dy:dy + H, dx:dx + W] @ w[dy, dx]
    if raw:
        return out
    return np.maximum(out * f64(scale) + f64(shift), 0.0)


def pack_bbox(y0, x0, y1, x1):
    """StemArgs::bbox: y0 | x0 << 8 | y1 << 16 | x1 << 24, rows y0..y1 and columns x0..x1 inclusive (x1 >= 128 sets bit 31)"""
    for v in (y0, x0, y1, x1):
        assert 0 <= int(v) <= 255
    return np.uint32(int(y0) | int(x0) << 8 | int(y1) << 16 | int(x1) << 24)


def rect_mask(bbox_u32, grow, H, W):
    """bool [n][H][W]: the pixels the sub-rectangle stems compute -- every image's box grown by `grow`, cut to the canvas"""
    bb = np.asarray(bbox_u32, dtype=np.uint32).reshape(-1).astype(np.int64)
    m = np.zeros((bb.size, H, W), dtype=bool)
    for i, b in enumerate(bb):
        y0, x0, y1, x1 = b & 255, (b >> 8) & 255, (b >> 16) & 255, (b >> 24) & 255
        r0, r1 = max(y0 - grow, 0), min(y1 + grow, H - 1)
        c0, c1 = max(x0 - grow, 0), min(x1 + grow, W - 1)
        m[i, r0:r1 + 1, c0:c1 + 1] = True
    return m


def stem_lds_bytes(H, W):
    """the padded float32 image a block of the one-image-per-block stems keeps in LDS"""
    return (H + 2) * (W + 2) * 3 * 4


def stem_group(n, H, W, group_max=4):
    """images a block of k_stem_conv_mfma takes per iteration (stem_mfma_launch)"""
    return max(1, min(group_max, LDS_64K // stem_lds_bytes(H, W), n))


def head_dense(h1, fc1_w, fc1_b, fc2_w, fc2_b, mask=None):
    """Flatten -> Dense(128) + ReLU -> Dense(3) + tanh -> obstacle overwrite; h1 [n][HW] (or [n][H][W])"""
    h1 = f64(h1)
    h1 = h1.reshape(h1.shape[0], -1)
    h2 = np.maximum(h1 @ f64(fc1_w) + f64(fc1_b), 0.0)
    q = np.tanh(h2 @ f64(fc2_w) + f64(fc2_b))
    if mask is not None:
        q[np.asarray(mask).reshape(q.shape) != 0] = -1.0
    return q


def head_pre_tanh(h1, fc1_w, fc1_b, fc2_w, fc2_b):
    """the argument of the tanh (the tests place it: some values in the linear part, some in the saturated part)"""
    h1 = f64(h1)
    h1 = h1.reshape(h1.shape[0], -1)
    return np.maximum(h1 @ f64(fc1_w) + f64(fc1_b), 0.0) @ f64(fc2_w) + f64(fc2_b)


def head(act, w1, s1, b1, fc1_w, fc1_b, fc2_w, fc2_b, mask=None):
    """1x1 convolution 128 -> 1 + folded batch norm (s1, b1) + ReLU, then head_dense.  act [n][H][W][128].  Returns (h1 [n][HW], q [n][3])"""
    act = f64(act)
    n = act.shape[0]
    h1 = np.maximum((act.reshape(n, -1, C) @ f64(w1).reshape(C)) * float(s1) + float(b1), 0.0)
    return h1, head_dense(h1, fc1_w, fc1_b, fc2_w, fc2_b, mask)


def head_dense_states_per_block(H, W):
    """k_head_dense<16 / 8 / 4>: the most states whose h1 and h2 rows fit 64 KB of LDS; 0 = refused"""
    per_state = (H * W + C) * 4
    for s in (16, 8, 4):
        if s * per_state <= LDS_64K:
            return s
    return 0


def row_index_f32(pix, wr):
    """the MFMA stem's row of pixel number `pix` in a rectangle `wr` wide, in the kernel's float32 arithmetic:
    yr = int((float(pix) + 0.5f) * (1.0f / float(wr)))"""
    inv = np.float32(1.0) / np.float32(wr)
    return ((np.asarray(pix).astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)
