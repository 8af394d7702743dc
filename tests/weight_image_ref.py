"""NumPy model of every weight image the tower convolutions read, written from the layout comments of csrc/conv_split.hip
(k_f16s_wscale, k_f16s_tail_from, k_f16s_weights, k_a16_weights, k_mxfp8_weights, the _batch forms, k_f16s_set_guard_word),
csrc/net.hip (k_transpose_w, k_wino_weights) and include/snake_engine.h -- byte for byte, in float32 where the kernels use it.

A kernel is the Keras HWIO array w [3][3][cin 128][cout 128] float32; tap = 3 kh + kw.

  weight scale   max |w| with fmaxf semantics (a NaN entry is ignored, an infinite one counts); k = 8 - ilogb(max) for
                 0 < max < 3e38, else 0; clamped to [K_MIN, K_MAX] = [-119, 100]: 256 <= max 2^k < 512 for every finite normal
                 maximum (ilogb <= 127 gives k >= -119, so the lower clamp is never reached; 2^-k = 2^119 is finite)
  tail           32 bytes at TAIL_OFFSET: float32 {2^-k, 2^k, x_scale, 1 / x_scale}, then int32 range flag 0, 4 bytes 0 and the
                 8-byte guard word address 0
  split image    f16 [chunk 8][tap 9][wn 4][half 2][lane 64][8]: lane = 32 h + l31, cout = 32 wn + l31, cin = 16 chunk + 8 h + j;
                 val = float32(w 2^k), hi = f16(val), lo = f16(float32(val - float32(hi))), both round to nearest even (NumPy's
                 float32 -> float16 cast), f16 subnormals kept.  flip: the source element is w[8 - tap][cout][cin]
  16-bit image   [chunk 4][tap 9][wn 4][k step 2][lane 64][8], cin = 32 chunk + 16 kstep + 8 h + j, in the FIRST half of the buffer.
                 f16: f16(w 2^k).  bf16: bf16(w 2^k) too -- k_a16_weights multiplies by tail[1] in both forms and the epilogue of
                 every form multiplies the sums by tail[0] (winv = tail[0] * tail[3], unconditional in hs_block).  The layer
                 tests of the bf16 tower model bf16(w) unscaled; the two agree only because the scale is a power of two and
                 nothing underflows: bf16(w 2^k) 2^-k == bf16(w) unless w 2^k or w is a float32 subnormal.
                 bf16 rounding: integer arithmetic on the float32 bits, round to nearest even, NaN kept NaN
  MX-FP8 image   e4m3fn codes [step 18 = 9 chunk64 + tap][wn 4][half p 2][lane 64][16]: lane (h, r) = 32 h + r holds cin
                 64 chunk + 32 p + 16 h + 0..15 of cout 32 wn + r; block = the 32 input channels of half p, quantized by the rule
                 of tests/mxfp8_ref.py; scale bytes at MX_SCALE_OFFSET shaped [step][wn][lane], lane (h, r): block h; the tail
                 is {1, 1, 1, 1, 0, 0, 0, 0}; the bytes between the scale bytes and the tail are not written
  transpose      float32 (tap, cout, cin)
  Winograd       float32 U[4 xi + nu][cin / 4][cout][cin % 4] = sum_ab G[xi][a] g[a][b] G[nu][b], summed in float64 in the
                 kernel's loop order (a outer, b inner, from 0.0) and rounded once to float32

NaN payloads are not part of the model: same_image() takes any NaN for any NaN; every other byte is exact, signs of zero
included (MX codes: a zero of either sign, mxfp8_ref.same_codes' rule).  MX blocks that hold a NaN or an infinity are outside
the rule (it is stated for finite values): mx_defined_mask() leaves their codes and scale byte out of a comparison.

`fault` arguments plant one known error each; tests/test_weight_image_ref_cpu.py asserts which cases of the table notice it.
"""
import functools

import numpy as np

import mxfp8_ref as mx

C = 128
N_W = 9 * C * C                               # 147456 kernel entries
TAIL_OFFSET = N_W * 4                         # SNK_CONV_F16S_TAIL_OFFSET
IMAGE_BYTES = TAIL_OFFSET + 32                # SNK_CONV_F16S_WEIGHT_BYTES
A16_BYTES = N_W * 2                           # the 16-bit images use the first half
MX_SCALE_OFFSET = N_W                         # one code byte per entry, then the scale bytes
MX_USED_BYTES = N_W + 18 * 4 * 64             # 152064
TRANSPOSE_BYTES = N_W * 4
WINO_BYTES = 16 * C * C * 4
K_MIN, K_MAX = -119, 100
FILL = 0xA5
G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)


# ---- scale -------------------------------------------------------------------------------------------------------------------
def abs_max(w):
    """fmaxf over |w| from 0: NaN entries are ignored, infinite ones count"""
    a = np.abs(np.asarray(w, np.float32).ravel())
    a = a[~np.isnan(a)]
    return np.float32(a.max()) if a.size else np.float32(0)


def weight_scale_k(w, fault=None, k_min=K_MIN):
    m = abs_max(w)
    k = 0
    if 0 < m < np.float32(3.0e38):
        f, ex = np.frexp(m)                   # m = f 2^ex, 0.5 <= f < 1 (subnormals too): ilogb = ex - 1
        k = 8 - (int(ex) - 1)
        if fault == "k_off_by_one" and f == 0.5:
            k += 1                            # 9 - ceil(log2 m): right except at an exact power of two
    return max(k_min, min(K_MAX, k))


def tail_bytes(k, x_scale=1.0, inv_x_scale=None):
    t = np.zeros(8, np.float32)
    t[0], t[1] = np.ldexp(np.float32(1), -k), np.ldexp(np.float32(1), k)
    t[2] = x_scale
    t[3] = np.float32(1) / np.float32(x_scale) if inv_x_scale is None else inv_x_scale
    return t.view(np.uint8).copy()


def _taps(w, flip=False, fault=None):
    """source array [tap][cin][cout] of an image's fragment order"""
    t = np.ascontiguousarray(np.asarray(w, np.float32)).reshape(9, C, C)
    if flip:
        t = t[::-1] if fault == "flip_no_swap" else t[::-1].transpose(0, 2, 1)
    return np.ascontiguousarray(t)


def _scaled(t, k):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return (t * np.ldexp(np.float32(1), k)).astype(np.float32)


# ---- roundings ---------------------------------------------------------------------------------------------------------------
def f16_rne(v):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(v, np.float32).astype(np.float16)


def _f16_neighbour(h, towards):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.nextafter(h, towards.astype(np.float16))


def f16_tie(v):
    """where the float32 value v lies exactly midway between two neighbouring f16 values (finite v only)"""
    v = np.asarray(v, np.float32)
    h = f16_rne(v)
    with np.errstate(over="ignore", invalid="ignore"):
        d = v.astype(np.float64) - h.astype(np.float64)
        nb = _f16_neighbour(h, np.where(d > 0, np.inf, -np.inf)).astype(np.float64)
        return np.isfinite(v) & np.isfinite(h.astype(np.float64)) & np.isfinite(nb) & (d != 0) & (2 * np.abs(d) == np.abs(nb - h.astype(np.float64)))


def f16_half_away(v):
    """the planted fault: ties go away from zero"""
    v = np.asarray(v, np.float32)
    h = f16_rne(v)
    with np.errstate(over="ignore", invalid="ignore"):
        nb = _f16_neighbour(h, np.where(v.astype(np.float64) > h.astype(np.float64), np.inf, -np.inf))
        return np.where(f16_tie(v) & (np.abs(nb) > np.abs(h)), nb, h)


def f16_truncate(v):
    """the planted fault: round towards zero"""
    v = np.asarray(v, np.float32)
    h = f16_rne(v)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(np.isfinite(v) & (np.abs(h.astype(np.float64)) > np.abs(v.astype(np.float64))),
                        _f16_neighbour(h, np.zeros(h.shape)), h)


def bf16_bits(v, fault=None):
    """float32 -> bf16 bit patterns (uint16), round to nearest even by integer arithmetic; NaN stays NaN (quiet bit set)"""
    u = np.ascontiguousarray(np.asarray(v, np.float32)).view(np.uint32).astype(np.uint64)
    if fault == "bf16_trunc":
        r = u >> 16
    else:
        r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


# ---- images ------------------------------------------------------------------------------------------------------------------
def split_parts(w, flip=False, k=None, fault=None):
    """(hi, lo) f16 arrays in [tap][cin][cout] order of the source array, and k"""
    if k is None:
        k = weight_scale_k(w, fault)
    val = _scaled(_taps(w, flip, fault), k)
    hi = f16_half_away(val) if fault == "hi_half_away" else f16_rne(val)
    with np.errstate(over="ignore", invalid="ignore"):
        if fault == "lo_f64":
            lo = (val.astype(np.float64) - hi.astype(np.float64)).astype(np.float16)
        else:
            r = (val - hi.astype(np.float32)).astype(np.float32)
            lo = f16_truncate(r) if fault == "lo_trunc" else f16_rne(r)
    return hi, lo, k


def _split_order(t, fault=None):
    """[tap][cin][cout] -> [chunk 8][tap 9][wn 4][h 2][l31 32][j 8]"""
    if fault == "hj_swap":                    # cin = 16 chunk + 2 j + h
        return t.reshape(9, 8, 8, 2, 4, 32).transpose(1, 0, 4, 3, 5, 2)
    return t.reshape(9, 8, 2, 8, 4, 32).transpose(1, 0, 4, 2, 5, 3)


def split_image(w, flip=False, x_scale=1.0, inv_x_scale=None, k=None, fault=None):
    """IMAGE_BYTES uint8: the split-f16 image (snk_conv3x3_prepare_weights_f16s, _f16s_train); k: a donor's scale"""
    hi, lo, k = split_parts(w, flip, k, fault)
    body = np.stack([_split_order(hi, fault), _split_order(lo, fault)], axis=3)
    return np.concatenate([np.ascontiguousarray(body).view(np.uint8).ravel(), tail_bytes(k, x_scale, inv_x_scale)])


def a16_image(w, bf, fault=None):
    """A16_BYTES + tail bytes: (body uint8 [A16_BYTES], tail uint8 [32]) of the f16 / bf16 activation towers' image"""
    k = weight_scale_k(w, fault)
    val = _scaled(_taps(w), k)
    v16 = bf16_bits(val, fault) if bf else f16_rne(val).view(np.uint16)
    body = v16.reshape(9, 4, 2, 2, 8, 4, 32).transpose(1, 0, 5, 2, 3, 6, 4)      # tap c ks h j wn l -> c tap wn ks h l j
    return np.ascontiguousarray(body).view(np.uint8).ravel(), tail_bytes(k)


def _mx_blocks(w):
    """[tap][chunk64 2][p 2][cout 128][32]"""
    return _taps(w).reshape(9, 2, 2, 32, C).transpose(0, 1, 2, 4, 3)


def mx_defined_blocks(w):
    """[tap][chunk][p][cout]: the block holds finite values only"""
    return np.isfinite(_mx_blocks(w)).all(axis=-1)


def mxfp8_image(w, fault=None):
    """(codes uint8 [N_W], scale bytes uint8 [4608], tail uint8 [32]); blocks with a NaN or an infinity are modelled as zeros"""
    x = np.where(mx_defined_blocks(w)[..., None], _mx_blocks(w), np.float32(0))
    codes, sb = mx.quantize_blocks(x)
    if fault == "mx_scale_wrong_p":           # codes against the other half's scale (saturating), scale bytes as they should be
        E = sb[:, :, ::-1].astype(np.int64) - 127
        q = np.clip(mx.e4m3_round(np.ldexp(x.astype(np.float64), -E[..., None])), -mx.E4M3_MAX, mx.E4M3_MAX)
        codes = mx.e4m3_code(q)
    codes = codes.reshape(9, 2, 2, 4, 32, 2, 16).transpose(1, 0, 3, 2, 5, 4, 6)   # tap c p wn r h i -> c tap wn p h r i
    sb = sb.reshape(9, 2, 2, 4, 32)                                               # tap c p wn r
    sb = sb.transpose(1, 0, 3, 4, 2) if fault == "mx_scale_lane_rh" else sb.transpose(1, 0, 3, 2, 4)
    tail = np.array([1, 1, 1, 1, 0, 0, 0, 0], np.float32).view(np.uint8)
    return np.ascontiguousarray(codes).ravel(), np.ascontiguousarray(sb).ravel(), tail.copy()


def mx_defined_mask(w):
    """(codes mask [N_W], scale mask [4608]) in image order: False where the block is outside the rule"""
    d = mx_defined_blocks(w)                                                      # tap c p co
    dc = np.broadcast_to(d[..., None], d.shape + (32,)).reshape(9, 2, 2, 4, 32, 2, 16).transpose(1, 0, 3, 2, 5, 4, 6)
    ds = d.reshape(9, 2, 2, 4, 32).transpose(1, 0, 3, 2, 4)
    return np.ascontiguousarray(dc).ravel(), np.ascontiguousarray(ds).ravel()


def transpose_image(w):
    return np.ascontiguousarray(_taps(w).transpose(0, 2, 1)).view(np.uint8).ravel()


def wino_image(w):
    g = np.asarray(w, np.float32).astype(np.float64)                              # [a][b][ci][co]
    U = np.empty((4, 4, C, C), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for xi in range(4):
            for nu in range(4):
                s = np.zeros((C, C), np.float64)
                for a in range(3):
                    for b in range(3):
                        s = s + G[xi][a] * g[a][b] * G[nu][b]
                U[xi, nu] = s.astype(np.float32)
    out = U.reshape(16, 32, 4, C).transpose(0, 1, 3, 2)                           # p, ci / 4, ci % 4, co -> p, ci / 4, co, ci % 4
    return np.ascontiguousarray(out).view(np.uint8).ravel()


# ---- whole buffers: what a prepare call writes, and the comparison -------------------------------------------------------------
KINDS = ("split", "a16", "mxfp8", "batch", "guard", "transpose", "wino")


def written_mask(kind, n_bytes):
    """bool [n_bytes]: the bytes a prepare call of that kind writes; everything else must stay as it was"""
    m = np.zeros(n_bytes, bool)
    if kind == "split":
        m[:IMAGE_BYTES] = True
    elif kind == "a16":
        m[:A16_BYTES] = True
        m[TAIL_OFFSET:IMAGE_BYTES] = True
    elif kind == "mxfp8":
        m[:MX_USED_BYTES] = True
        m[TAIL_OFFSET:IMAGE_BYTES] = True
    elif kind == "batch":                     # tail[2..3] belong to the producer of the convolution's input
        m[:TAIL_OFFSET + 8] = True
        m[TAIL_OFFSET + 16:IMAGE_BYTES] = True
    elif kind == "guard":
        m[TAIL_OFFSET + 24:IMAGE_BYTES] = True
    elif kind == "transpose":
        m[:TRANSPOSE_BYTES] = True
    elif kind == "wino":
        m[:WINO_BYTES] = True
    else:
        raise ValueError(kind)
    return m


def expected_buffer(kind, n_bytes, image, before=None):
    """the whole buffer after the call: the model's bytes where the mask says written, `before` (default: FILL) elsewhere.
    image: the model's bytes from offset 0 (a16 / mxfp8: a tuple of parts, placed at their offsets)"""
    out = np.full(n_bytes, FILL, np.uint8) if before is None else np.array(before, np.uint8)
    new = np.zeros(n_bytes, np.uint8)
    if kind == "a16":
        new[:A16_BYTES], new[TAIL_OFFSET:IMAGE_BYTES] = image
    elif kind == "mxfp8":
        new[:N_W], new[N_W:MX_USED_BYTES], new[TAIL_OFFSET:IMAGE_BYTES] = image
    else:
        new[:len(image)] = image
    m = written_mask(kind, n_bytes)
    out[m] = new[m]
    return out


def _same_float(got, want, utype, exp_mask, man_mask):
    g, w = got.view(utype), want.view(utype)
    nan = lambda u: ((u & exp_mask) == exp_mask) & ((u & man_mask) != 0)
    return (g == w) | (nan(g) & nan(w))


def same_image(kind, got, want, bf=False, defined=None):
    """bool [n_bytes] per byte: got equals want -- exactly, except that any NaN matches any NaN (f16 / bf16 / float32 by
    region), and for MX codes a zero of either sign matches a zero; defined = mx_defined_mask(w) leaves blocks outside the rule out"""
    got, want = np.asarray(got, np.uint8), np.asarray(want, np.uint8)
    ok = got == want
    if kind in ("split", "batch", "a16"):
        n = TAIL_OFFSET if kind != "a16" else A16_BYTES
        e, m = (0x7F80, 0x007F) if bf else (0x7C00, 0x03FF)
        ok[:n] = np.repeat(_same_float(got[:n], want[:n], np.uint16, e, m), 2)
    elif kind in ("transpose", "wino"):
        n = TRANSPOSE_BYTES if kind == "transpose" else WINO_BYTES
        ok[:n] = np.repeat(_same_float(got[:n], want[:n], np.uint32, 0x7F800000, 0x007FFFFF), 4)
    elif kind == "mxfp8":
        g, w = got[:N_W], want[:N_W]
        ok[:N_W] |= ((g & 0x7F) == 0) & ((w & 0x7F) == 0)
        if defined is not None:
            ok[:N_W] |= ~defined[0]
            ok[N_W:MX_USED_BYTES] |= ~defined[1]
    return ok


# ---- decoding (the tests of the model itself) ----------------------------------------------------------------------------------
def decode_tail(image):
    return np.asarray(image[TAIL_OFFSET:IMAGE_BYTES], np.uint8).view(np.float32).copy()


def decode_split(image):
    """(hi, lo) float64 [tap][cin][cout] of a split image's fragment order (scaled values), and the tail"""
    b = np.asarray(image[:TAIL_OFFSET], np.uint8).view(np.float16).reshape(8, 9, 4, 2, 2, 32, 8).astype(np.float64)
    back = lambda t: np.ascontiguousarray(t.transpose(1, 0, 3, 5, 2, 4)).reshape(9, C, C)
    return back(b[:, :, :, 0]), back(b[:, :, :, 1]), decode_tail(image)


def decode_a16(body, bf):
    u = np.asarray(body, np.uint8).view(np.uint16).reshape(4, 9, 4, 2, 2, 32, 8)
    u = np.ascontiguousarray(u.transpose(1, 0, 3, 4, 6, 2, 5)).reshape(9, C, C)   # c tap wn ks h l j -> tap c ks h j wn l
    if bf:
        return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return u.view(np.float16).astype(np.float64)


def decode_mxfp8(codes, sb):
    c = np.asarray(codes, np.uint8).reshape(2, 9, 4, 2, 2, 32, 16).transpose(1, 0, 3, 2, 5, 4, 6)   # -> tap c p wn r h i
    s = np.asarray(sb, np.uint8).reshape(2, 9, 4, 2, 32).transpose(1, 0, 3, 2, 4)                   # -> tap c p wn r
    v = mx.dequantize_blocks(np.ascontiguousarray(c).reshape(9, 2, 2, C, 32), np.ascontiguousarray(s).reshape(9, 2, 2, C))
    return np.ascontiguousarray(v.transpose(0, 1, 2, 4, 3)).reshape(9, C, C)


def decode_transpose(image):
    return np.asarray(image, np.uint8).view(np.float32).reshape(9, C, C).transpose(0, 2, 1).astype(np.float64)


def decode_wino(image):
    """least-squares inverse of U = G g G^T (float64), [tap][cin][cout]"""
    U = np.asarray(image, np.uint8).view(np.float32).reshape(4, 4, 32, C, 4).astype(np.float64)
    U = U.transpose(0, 1, 2, 4, 3).reshape(4, 4, C, C)
    P = np.linalg.pinv(G)
    return np.einsum("ax,xyio,by->abio", P, U, P).reshape(9, C, C)


# ---- the case table ------------------------------------------------------------------------------------------------------------
def _glorot(seed):
    return (np.random.RandomState(seed).randn(3, 3, C, C) * 0.05).astype(np.float32)


def _with_max(seed, m, at=None, negative=False):
    """random entries of magnitude <= 0.9 m and one entry of magnitude m (float32) at flat index `at` (default: drawn)"""
    rng = np.random.RandomState(seed)
    b = rng.randn(N_W)
    w = (b / np.abs(b).max() * (0.9 * float(m))).astype(np.float32)
    w[rng.randint(N_W) if at is None else at] = -np.float32(m) if negative else np.float32(m)
    assert abs_max(w) == np.float32(m)
    return w.reshape(3, 3, C, C)


def _ties(seed=77):
    """k = 0 (one entry -300, everything else below 300).  A third of the entries are plain uniform values: with
    val = hi + r, r = m 2^(e - 23) has up to 13 significant bits, so lo = f16(r) is a tie for every odd m of 12 bits -- about
    a quarter of them.  A third are scaled down by 2^-1 .. 2^-40: lo (and hi, further down) are f16 subnormals or zero, and
    entries below 2^-24 of the maximum vanish from hi.  The rest: f16 values plus exactly half an f16 ulp (hi ties, both
    parities, normal and subnormal), signed zeros, and the subnormal range's own ties (2^-25, 3 2^-25)."""
    rng = np.random.RandomState(seed)
    w = rng.uniform(-299.0, 299.0, N_W).astype(np.float32)
    third = N_W // 3
    w[third:2 * third] = np.ldexp(w[third:2 * third], -rng.randint(1, 41, third)).astype(np.float32)
    n_t = 4000
    bits = rng.randint(0x0001, 0x5BFF, n_t).astype(np.uint16)                    # f16 patterns 2^-24 .. below 256
    h = bits.view(np.float16)
    ulp = (np.nextafter(h, np.float16(np.inf)).astype(np.float64) - h.astype(np.float64))
    t = (h.astype(np.float64) + ulp / 2).astype(np.float32)
    assert np.array_equal(t.astype(np.float64), h.astype(np.float64) + ulp / 2)   # representable in float32
    w[2 * third:2 * third + n_t] = t * rng.choice([-1.0, 1.0], n_t).astype(np.float32)
    o = 2 * third + n_t
    w[o:o + 8] = [0.0, -0.0, 2.0 ** -25, -2.0 ** -25, 3 * 2.0 ** -25, -3 * 2.0 ** -25, 2.0 ** -30, -2.0 ** -40]
    w[o + 8:o + 64] = -0.0
    w = w[rng.permutation(N_W)]
    w[12345] = -300.0
    return w.reshape(3, 3, C, C)


def bf16_edge_blocks():
    """the hand-picked blocks of tests/test_mxfp8_gpu.py's _bf16_edge_blocks (bf16-exact values)"""
    rows = [[0.0], [448.0, -448.0, 1.0], [448.0 * 2.0 ** 5, 3.0], [448.0 * 2.0 ** -20, -1.0 * 2.0 ** -20],
            [1.0078125, 0.5], [451.5, 3.0], [448.0, 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -10, 0.75 * 2.0 ** -9, 7 * 2.0 ** -9, 2.0 ** -6],
            [448.0, 1.0625, 1.1875, -1.0625, 248.0, 216.0], [2.0 ** -130, -(2.0 ** -131), 2.0 ** -133]]
    out = np.zeros((len(rows), 32), np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def f32_edge_blocks():
    """blocks only float32 can express: a maximum one ulp above 448 2^E, exactly 1.75 2^e and one ulp above it, and values one
    ulp on either side of the midpoint of two neighbouring e4m3 codes (normal, top binade and subnormal; scale 1 and 2^-3)"""
    f = np.float32
    up = lambda v: np.nextafter(f(v), f(np.inf))
    dn = lambda v: np.nextafter(f(v), f(-np.inf))
    rows = []
    for E in (0, 5, -20):
        rows.append([up(448.0 * 2.0 ** E), -448.0 * 2.0 ** E, 2.0 ** E, 3 * 2.0 ** (E - 10)])
    for e in (0, 3, -7):
        rows.append([1.75 * 2.0 ** e, -1.0 * 2.0 ** e, 2.0 ** (e - 9)])
        rows.append([-up(1.75 * 2.0 ** e), 1.75 * 2.0 ** e, 2.0 ** (e - 9)])
    for s in (1.0, 0.125):
        mids = [1.0625, 248.0, 1.5 * 2.0 ** -9, 0.5 * 2.0 ** -9, 15.5 * 2.0 ** -9, 416.0]
        row = [448.0 * s]
        for m in mids:
            row += [up(m * s), dn(m * s), -up(m * s), -dn(m * s), m * s]
        rows.append(row)
    out = np.zeros((len(rows), 32), np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


# where the edge blocks go: first and last step (chunk64 0 tap 0, chunk64 1 tap 8), wn 0 and 3, both halves p
MX_PLANTS = [(tap, c64, p, wn) for (tap, c64) in ((0, 0), (8, 1)) for wn in (0, 3) for p in (0, 1)]


def plant_blocks(w, blocks):
    """block i -> input channels 64 c64 + 32 p .. + 31 of (tap, cout 32 wn + i), at every position of MX_PLANTS"""
    t = np.array(w, np.float32).reshape(9, C, C)
    assert len(blocks) <= 32
    for tap, c64, p, wn in MX_PLANTS:
        for i, blk in enumerate(blocks):
            t[tap, 64 * c64 + 32 * p:64 * c64 + 32 * p + 32, 32 * wn + i] = blk
    return t.reshape(3, 3, C, C)


def _nan_case():
    w = _glorot(31).reshape(-1)
    w[[0, 7, 4097, 70000, N_W - 1]] = np.nan
    return w.reshape(3, 3, C, C)


def _inf_case():
    w = _glorot(32).reshape(-1)
    w[54321] = np.inf
    return w.reshape(3, 3, C, C)


_BUILDERS = [("glorot", lambda: _glorot(1)), ("ties", _ties)]
for _i, _e in enumerate((-3, 0, 5)):
    _BUILDERS.append((f"pow2_{_e}", functools.partial(_with_max, 10 + _i, np.float32(2.0 ** _e))))
    _BUILDERS.append((f"below_pow2_{_e}", functools.partial(_with_max, 20 + _i, np.nextafter(np.float32(2.0 ** _e), np.float32(0)))))
_BUILDERS += [
    ("max_first", lambda: _with_max(40, np.float32(0.37), at=0)),
    ("max_last", lambda: _with_max(41, np.float32(0.37), at=N_W - 1)),
    ("max_negative", lambda: _with_max(42, np.float32(0.61), negative=True)),
    ("zero", lambda: np.zeros((3, 3, C, C), np.float32)),
    ("sub_2^-140", lambda: _with_max(43, np.float32(2.0 ** -140))),
    ("tiny_2^-110", lambda: _with_max(44, np.float32(2.0 ** -110))),
    ("big_2^110", lambda: _with_max(45, np.float32(2.0 ** 110))),
    ("big_2^117", lambda: _with_max(46, np.float32(2.0 ** 117))),
    ("nan", _nan_case),
    ("inf", _inf_case),
    ("mx_bf16_edges", lambda: plant_blocks(_glorot(50), bf16_edge_blocks())),
    ("mx_f32_edges", lambda: plant_blocks(_glorot(51), f32_edge_blocks())),
]
CASE_NAMES = [n for n, _ in _BUILDERS]


@functools.lru_cache(maxsize=None)
def case(name):
    """the named [3, 3, 128, 128] float32 kernel (read-only: shared by every test)"""
    w = np.ascontiguousarray(dict(_BUILDERS)[name](), np.float32)
    assert w.shape == (3, 3, C, C)
    w.setflags(write=False)
    return w
