"""NumPy restatement of the MX-FP8 quantization rule of the mxfp8 tower (csrc/conv_split.hip mx_scale_byte / mx_quant8 /
k_mxfp8_weights, include/snake_engine.h), and the Q-net with that tower's rounding points.

The rule:
  block  activations: the 32 input channels 32j .. 32j+31 of one pixel; weights: the same 32 input channels of one
         (output channel, tap)
  amax   the largest |v| of the block in float32
  E      the smallest integer with amax * 2^-E <= 448, clamped to [-127, 127]; amax == 0 gives E = -127; scale byte = E + 127
  code   OCP e4m3fn, round to nearest even of v * 2^-E, subnormals kept (nothing saturates by the choice of E)
"""
import numpy as np

E4M3_MAX = 448.0


def _e4m3_table():
    """the 127 non-negative finite e4m3fn values, index = code (0x00 .. 0x7E)"""
    c = np.arange(127)
    e, m = c >> 3, c & 7
    return np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))


E4M3_VALUES = _e4m3_table()


def scale_exponent(amax):
    """E of the rule for an array of block maxima (float32 or float64 values, >= 0)"""
    a = np.asarray(amax, np.float64)
    f, ex = np.frexp(a)                      # a = f 2^ex, 0.5 <= f < 1: m = 2 f, e = ex - 1; E = e - 8 if m <= 1.75 else e - 7
    E = np.where(f <= 0.875, ex - 9, ex - 8)
    E = np.where(a == 0, -127, E)
    return np.clip(E, -127, 127).astype(np.int64)


def e4m3_round(y):
    """round-to-nearest-even of float64 values |y| <= 448 onto the e4m3fn grid (subnormals kept)"""
    y = np.asarray(y, np.float64)
    a = np.abs(y)
    _, ex = np.frexp(np.where(a > 0, a, 1.0))
    quantum = np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)     # 3 mantissa bits; below 2^-6 the subnormal spacing 2^-9
    return np.copysign(np.round(a / quantum) * quantum, y)   # np.round: half to even (a / quantum is exact)


def e4m3_code(q):
    """codes of values already on the e4m3fn grid (sign bit 0x80)"""
    q = np.asarray(q, np.float64)
    idx = np.searchsorted(E4M3_VALUES, np.abs(q))
    assert np.array_equal(E4M3_VALUES[np.minimum(idx, 126)], np.abs(q)), "value off the e4m3 grid"
    return (idx | np.where(np.signbit(q), 0x80, 0)).astype(np.uint8)


def quantize_blocks(x):
    """x [..., 32] (float32 values) -> (codes uint8 [..., 32], scale bytes uint8 [...])"""
    x = np.asarray(x, np.float32).astype(np.float64)
    E = scale_exponent(np.abs(x).max(axis=-1))
    q = e4m3_round(np.ldexp(x, -E[..., None]))
    assert np.abs(q).max(initial=0.0) <= E4M3_MAX
    return e4m3_code(q), (E + 127).astype(np.uint8)


def dequantize_blocks(codes, sbytes):
    codes = np.asarray(codes, np.uint8)
    v = E4M3_VALUES[codes & 0x7F] * np.where(codes & 0x80, -1.0, 1.0)
    return np.ldexp(v, np.asarray(sbytes, np.int64)[..., None] - 127)


def mx_round(x, axis=-1):
    """the values the MFMA sees: x quantized in blocks of 32 consecutive entries along `axis` and dequantized (float64)"""
    x = np.moveaxis(np.asarray(x, np.float32), axis, -1)
    shp = x.shape
    b = x.reshape(shp[:-1] + (shp[-1] // 32, 32)).astype(np.float64)
    E = scale_exponent(np.abs(b).max(axis=-1))
    out = np.ldexp(e4m3_round(np.ldexp(b, -E[..., None])), E[..., None])
    return np.moveaxis(out.reshape(shp), -1, axis)


def same_codes(a, b):
    """code arrays equal, a zero of either sign counting as equal"""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    za, zb = (a & 0x7F) == 0, (b & 0x7F) == 0
    return bool(np.all((a == b) | (za & zb)))


def forward(weights, states):
    """AlphaNNet.v of the mxfp8 tower with its rounding points: oracle/net_ref.py's graph with bf16 activations in HBM (as
    bf16_act=True) and the tower convolutions' operands MX-quantized -- activations per pixel and 32-channel block, weights per
    (output channel, tap, 32 input channels) from their float32 values; products and sums in float32."""
    import torch
    import torch.nn.functional as F
    t = [torch.as_tensor(np.asarray(w, np.float32)) for w in weights]
    blocks = (len(t) - 14) // 10
    x = torch.as_tensor(np.ascontiguousarray(states, np.float32)).permute(0, 3, 1, 2)

    def conv(x, k):
        return F.conv2d(x, k.permute(3, 2, 0, 1), padding=k.shape[0] // 2)

    def conv_mx(x, k):
        xq = torch.as_tensor(mx_round(x.numpy(), axis=1).astype(np.float32))
        kq = torch.as_tensor(mx_round(k.numpy(), axis=2).astype(np.float32))
        return conv(xq, kq)

    def bn(x, g, b, m, v):
        return F.batch_norm(x, m, v, g, b, training=False, eps=1e-3)

    def r16(v):
        return v.to(torch.bfloat16).to(torch.float32)
    with torch.no_grad():
        h = r16(F.relu(bn(conv(x, t[0]), *t[1:5])))
        for blk in range(blocks):
            b0 = 5 + 10 * blk
            sc = h
            h = r16(F.relu(bn(conv_mx(h, t[b0]), *t[b0 + 1:b0 + 5])))
            h = F.relu(bn(conv_mx(h, t[b0 + 5]), *t[b0 + 6:b0 + 10]) + sc)
            if blk + 1 < blocks:
                h = r16(h)
        b0 = 5 + 10 * blocks
        h = F.relu(bn(conv(h, t[b0]), *t[b0 + 1:b0 + 5]))
        h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)
        h = F.relu(h @ t[b0 + 5] + t[b0 + 6])
        return torch.tanh(h @ t[b0 + 7] + t[b0 + 8]).numpy()
