"""The NumPy model of the weight images (tests/weight_image_ref.py) checked on its own, without a GPU: decoding its images
recovers the kernel, the flipped image is the forward image of the input gradient's kernel (and that kernel is the right one:
a float64 convolution with it equals autograd's input gradient), the integer bf16 rounding equals torch's, the `ties` kernel
holds the roundings it promises, and every planted fault of the model is noticed by the cases that should notice it.

Bounds.  val = float32(w 2^k), |val| < 512, hi = f16(val), r = val - hi (exact in float32: both are multiples of val's float32
ulp and |r| <= |val|), lo = f16(r).  For val in [2^e, 2^(e+1)): |r| <= 2^(e-11), and a normal lo keeps 11 bits of it, so
|hi + lo - val| <= 2^(e-23) <= 2^-23 |val|; an f16-subnormal lo is off by at most half its spacing, 2^-25.  The test asserts
|hi + lo - val| <= max(2^-22 |val|, 2^-25), and equality wherever val is a multiple of 2^-14 (then r is a multiple of 2^-14 of
at most 2^11 steps: an f16 number)."""
import numpy as np
import pytest

import mxfp8_ref as mx
import weight_image_ref as wi

FINITE = [n for n in wi.CASE_NAMES if n not in ("nan", "inf")]


def _scaled64(w, k):
    return np.ldexp(wi._taps(w).astype(np.float64), k)


@pytest.mark.parametrize("name", wi.CASE_NAMES)
def test_split_image_decodes_to_the_kernel(name):
    w = wi.case(name)
    img = wi.split_image(w, x_scale=0.125)
    assert img.dtype == np.uint8 and img.shape == (wi.IMAGE_BYTES,)
    hi, lo, tail = wi.decode_split(img)
    k = wi.weight_scale_k(w)
    assert tail.tolist() == [2.0 ** -k, 2.0 ** k, 0.125, 8.0, 0, 0, 0, 0]
    m = float(wi.abs_max(w))
    if 2.0 ** -92 <= m < 3e38:                                     # below 2^-92 the upper clamp k = 100 holds the scale back
        assert 256 <= m * 2.0 ** k < 512
    if name in ("nan", "inf"):
        bad = ~np.isfinite(wi._taps(w))
        assert np.isnan(hi[bad] + lo[bad]).all() and np.isfinite(hi[~bad] + lo[~bad]).all()
        return
    val = wi._scaled(wi._taps(w), k).astype(np.float64)            # the float32 product, as the kernel forms it
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    err = np.abs(hi + lo - val)
    assert (err <= np.maximum(2.0 ** -22 * np.abs(val), 2.0 ** -25)).all(), err.max()
    grid = np.ldexp(val, 14) == np.round(np.ldexp(val, 14))
    assert grid.any() and (err[grid] == 0).all()
    # and val itself is w 2^k exactly unless the product is a float32 subnormal
    exact = val == _scaled64(w, k)
    assert (exact | (np.abs(_scaled64(w, k)) < 2.0 ** -126)).all()


@pytest.mark.parametrize("name", FINITE)
def test_other_images_decode_to_the_kernel(name):
    w = wi.case(name)
    t = wi._taps(w)
    import torch
    k = wi.weight_scale_k(w)
    val = torch.as_tensor(wi._scaled(t, k))
    body, tail = wi.a16_image(w, bf=False)
    assert np.array_equal(wi.decode_a16(body, False), val.to(torch.float16).double().numpy())
    assert tail.view(np.float32).tolist() == [2.0 ** -k, 2.0 ** k, 1, 1, 0, 0, 0, 0]
    body, _ = wi.a16_image(w, bf=True)
    assert np.array_equal(wi.decode_a16(body, True), val.to(torch.bfloat16).double().numpy())
    codes, sb, tail = wi.mxfp8_image(w)
    assert codes.shape == (wi.N_W,) and sb.shape == (18 * 4 * 64,)
    assert np.array_equal(wi.decode_mxfp8(codes, sb), mx.mx_round(t, axis=1))
    assert tail.view(np.float32).tolist() == [1, 1, 1, 1, 0, 0, 0, 0]
    assert np.array_equal(wi.decode_transpose(wi.transpose_image(w)), t.astype(np.float64))
    got = wi.decode_wino(wi.wino_image(w))
    # U is rounded to float32 (2^-24 relative, 2^-150 absolute among subnormals); the inverse sums 16 entries of weight <= 4
    assert np.abs(got - t).max() <= 1e-6 * float(np.abs(t).max()) + 2.0 ** -144


def test_wino_image_against_a_matrix_product():
    w = wi.case("glorot")
    U = wi.wino_image(w).view(np.float32).reshape(4, 4, 32, wi.C, 4).transpose(0, 1, 2, 4, 3).reshape(4, 4, wi.C, wi.C)
    ref = np.einsum("xa,abio,yb->xyio", wi.G, w.astype(np.float64), wi.G)
    assert np.abs(U - ref).max() <= 2.0 ** -24 * np.abs(ref).max()
    assert np.array_equal(U[0, 0], w[0, 0]) and np.array_equal(U[3, 3], w[2, 2]) and np.array_equal(U[0, 3], w[0, 2])


def _flipped_kernel(w):
    """w'[tap][ci][co] = w[8 - tap][co][ci]"""
    return np.ascontiguousarray(w.reshape(9, wi.C, wi.C)[::-1].transpose(0, 2, 1)).reshape(3, 3, wi.C, wi.C)


@pytest.mark.parametrize("name", wi.CASE_NAMES)
def test_flip_image_is_the_forward_image_of_the_flipped_kernel(name):
    w = wi.case(name)
    a, b = wi.split_image(w, flip=True), wi.split_image(_flipped_kernel(w))
    assert wi.same_image("split", a, b).all()
    if name not in ("nan", "inf"):
        assert np.array_equal(a, b)


def test_flipped_kernel_convolves_to_the_input_gradient():
    import torch
    import torch.nn.functional as F
    w = wi.case("glorot")
    hi, lo, tail = wi.decode_split(wi.split_image(w))
    kf = torch.as_tensor((hi + lo) * float(tail[0])).reshape(3, 3, wi.C, wi.C)              # the forward image's kernel, HWIO
    hi, lo, tail = wi.decode_split(wi.split_image(w, flip=True))
    kb = torch.as_tensor((hi + lo) * float(tail[0])).reshape(3, 3, wi.C, wi.C)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, wi.C, 5, 6, dtype=torch.float64, generator=g, requires_grad=True)
    dy = torch.randn(2, wi.C, 5, 6, dtype=torch.float64, generator=g)
    y = F.conv2d(x, kf.permute(3, 2, 0, 1), padding=1)
    dx, = torch.autograd.grad(y, x, dy)
    got = F.conv2d(dy, kb.permute(3, 2, 0, 1), padding=1)
    assert (got - dx).abs().max() <= 1e-13 * dx.abs().max()
    assert (y - F.conv2d(x, torch.as_tensor(np.array(w)).double().permute(3, 2, 0, 1), padding=1)).abs().max() <= 2.0 ** -20 * y.abs().max()


@pytest.mark.parametrize("name", wi.CASE_NAMES)
def test_integer_bf16_rounding_equals_torch(name):
    import torch
    w = wi.case(name)
    for v in (w.reshape(-1), wi._scaled(wi._taps(w), wi.weight_scale_k(w)).reshape(-1)):
        got = wi.bf16_bits(v)
        want = torch.as_tensor(np.array(v)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        nan = np.isnan(v)
        assert np.array_equal(got[~nan], want[~nan])
        assert (((got[nan] & 0x7F80) == 0x7F80) & ((got[nan] & 0x7F) != 0)).all()
    # ties and the carry into the exponent, by hand
    v = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3FFF8000, 0x7F7FFFFF, 0x80008000, 0x00018000], np.uint32).view(np.float32)
    assert wi.bf16_bits(v).tolist() == [0x3F80, 0x3F82, 0x3F81, 0x4000, 0x7F80, 0x8000, 0x0002]


def test_ties_kernel_holds_what_it_promises():
    w = wi.case("ties")
    assert wi.weight_scale_k(w) == 0 and float(wi.abs_max(w)) == 300.0
    assert np.count_nonzero(np.abs(w) == 300.0) == 1 and (np.abs(w) < 512).all()
    val = wi._taps(w)
    hi, lo, _ = wi.split_parts(w)
    r = (val - hi.astype(np.float32)).astype(np.float32)
    assert np.array_equal(r.astype(np.float64), val.astype(np.float64) - hi.astype(np.float64))   # the difference is exact
    assert np.count_nonzero(wi.f16_tie(val)) >= 1000
    assert np.count_nonzero(wi.f16_tie(r)) >= 1000
    lo_small = np.abs(lo.astype(np.float64)) < 2.0 ** -14
    assert np.count_nonzero(lo_small) >= 1000
    assert np.count_nonzero(lo_small & (lo != 0)) >= 1000                                        # true subnormals, not only zeros
    hi_sub = (np.abs(hi.astype(np.float64)) < 2.0 ** -14) & (hi != 0)
    assert np.count_nonzero(hi_sub) >= 1000
    assert np.count_nonzero(np.signbit(val) & (val == 0)) >= 8                                    # -0.0
    assert np.count_nonzero((val != 0) & (np.abs(val) < 300.0 * 2.0 ** -24)) >= 100              # vanish from hi
    # both directions of round-to-even among the hi ties
    t = wi.f16_tie(val)
    up = np.abs(hi.astype(np.float64)) > np.abs(val.astype(np.float64))
    assert np.count_nonzero(t & up) >= 300 and np.count_nonzero(t & ~up) >= 300


def test_mx_edge_blocks_are_where_the_table_says():
    for name, blocks in (("mx_bf16_edges", wi.bf16_edge_blocks()), ("mx_f32_edges", wi.f32_edge_blocks())):
        w = wi.case(name)
        codes, sb, _ = wi.mxfp8_image(w)
        want_c, want_s = mx.quantize_blocks(blocks)
        codes = codes.reshape(18, 4, 2, 2, 32, 16)                 # step wn p h r i
        sb = sb.reshape(18, 4, 2, 32)                              # step wn h(block) r
        for tap, c64, p, wn in wi.MX_PLANTS:
            step = 9 * c64 + tap
            assert step in (0, 17)
            for i in range(len(blocks)):
                got = codes[step, wn, p, :, i, :].reshape(32)     # (h, 16): input channels 16 h + 0..15 of the half
                assert np.array_equal(got, want_c[i]), (name, tap, c64, p, wn, i)
                assert sb[step, wn, p, i] == want_s[i]
    # the float32-only edges do what they are there for
    b = wi.f32_edge_blocks()
    E = mx.scale_exponent(np.abs(b).max(axis=1))
    assert E[:3].tolist() == [1, 6, -19]                           # one ulp above 448 2^E: the next exponent
    assert E[3:9].tolist() == [-8, -7, -5, -4, -15, -14]           # 1.75 2^e: e - 8; one ulp above: e - 7
    c, _ = mx.quantize_blocks(b[9:10])
    v = mx.E4M3_VALUES[c[0] & 0x7F]
    assert v[1:6].tolist() == [1.125, 1.0, 1.125, 1.0, 1.0]        # above / below the midpoint 1.0625, and the tie to even


FAULT_IMAGES = {
    "lo_trunc": lambda w, f: wi.split_image(w, fault=f),
    "lo_f64": lambda w, f: wi.split_image(w, fault=f),
    "hi_half_away": lambda w, f: wi.split_image(w, fault=f),
    "k_off_by_one": lambda w, f: wi.split_image(w, fault=f),
    "hj_swap": lambda w, f: wi.split_image(w, fault=f),
    "flip_no_swap": lambda w, f: wi.split_image(w, flip=True, fault=f),
    "mx_scale_wrong_p": lambda w, f: np.concatenate(wi.mxfp8_image(w, fault=f)),
    "mx_scale_lane_rh": lambda w, f: np.concatenate(wi.mxfp8_image(w, fault=f)),
    "bf16_trunc": lambda w, f: np.concatenate(wi.a16_image(w, True, fault=f)),
}
_NOTICED = {}


def _noticed(fault):
    if fault not in _NOTICED:
        make = FAULT_IMAGES[fault]
        kind = "mxfp8" if fault.startswith("mx_") else "split"
        out = set()
        for name in wi.CASE_NAMES:
            a, b = make(wi.case(name), fault), make(wi.case(name), None)
            same = wi.same_image(kind, a, b).all() if kind == "split" and len(a) == wi.IMAGE_BYTES else np.array_equal(a, b)
            if not same:
                out.add(name)
        _NOTICED[fault] = out
    return _NOTICED[fault]


@pytest.mark.parametrize("fault", ["hj_swap", "flip_no_swap", "mx_scale_wrong_p", "mx_scale_lane_rh", "bf16_trunc", "lo_trunc"])
def test_layout_and_rounding_faults_are_noticed_by_every_nonzero_case(fault):
    """a wrong index map, a scale from the wrong block and a rounding towards zero change bytes of every kernel with random
    content; the all-zero kernel cannot see any of them.  The 2^-140 kernel is blind to three: its scaled values are at most
    2^-40 (the clamp k = 100), far below half the smallest f16 subnormal, so the split image is tiny hi and lo = 0 under either
    rounding; and all of its MX blocks clamp to E = -127 with every code zero, so the scale bytes are all alike"""
    blind = {"zero"}
    if fault in ("mx_scale_wrong_p", "mx_scale_lane_rh", "lo_trunc"):
        blind.add("sub_2^-140")
    assert _noticed(fault) == set(wi.CASE_NAMES) - blind


def test_half_away_rounding_is_noticed_where_a_tie_goes_down():
    """cases that hold a hi tie whose even neighbour is the smaller one -- `ties` by construction (thousands), random kernels
    by chance (a tie needs 13 zero bits: about 18 of 147456 entries)"""
    want = set()
    for name in wi.CASE_NAMES:
        w = wi.case(name)
        val = wi._scaled(wi._taps(w), wi.weight_scale_k(w))
        hi = wi.f16_rne(val)
        with np.errstate(invalid="ignore"):
            if (wi.f16_tie(val) & (np.abs(hi.astype(np.float64)) < np.abs(val.astype(np.float64)))).any():
                want.add(name)
    assert "ties" in want and _noticed("hi_half_away") == want


def test_k_off_by_one_is_noticed_at_exact_powers_of_two_only():
    """... whose k is not clamped: 2^-140 and 2^-110 clamp to 100 either way"""
    assert _noticed("k_off_by_one") == {"pow2_-3", "pow2_0", "pow2_5", "big_2^110", "big_2^117"}


def test_a_float64_difference_changes_nothing():
    """val - float(hi) is exact in float32 (see the module docstring), so `lo` from a float64 difference is the same number in
    every case: this variant is not a fault the bytes could show, and the model may use either"""
    assert _noticed("lo_f64") == set()


def test_written_masks():
    n = wi.IMAGE_BYTES + 64
    count = lambda kind, nb=n: int(wi.written_mask(kind, nb).sum())
    assert count("split") == wi.IMAGE_BYTES and count("a16") == wi.A16_BYTES + 32 and count("mxfp8") == 152064 + 32
    assert count("batch") == wi.IMAGE_BYTES - 8 and count("guard") == 8
    assert count("transpose", wi.TRANSPOSE_BYTES + 64) == wi.TRANSPOSE_BYTES and count("wino", wi.WINO_BYTES + 64) == wi.WINO_BYTES
    for kind in ("split", "a16", "mxfp8", "batch", "guard"):
        assert not wi.written_mask(kind, n)[wi.IMAGE_BYTES:].any()
    m = wi.written_mask("batch", n)
    assert not m[wi.TAIL_OFFSET + 8:wi.TAIL_OFFSET + 16].any() and m[wi.TAIL_OFFSET:wi.TAIL_OFFSET + 8].all()
    buf = wi.expected_buffer("a16", n, wi.a16_image(wi.case("glorot"), True))
    assert (buf[wi.A16_BYTES:wi.TAIL_OFFSET] == wi.FILL).all() and (buf[wi.IMAGE_BYTES:] == wi.FILL).all()
    assert buf[wi.TAIL_OFFSET:wi.IMAGE_BYTES].view(np.float32)[2] == 1.0


def test_scale_rule_edges():
    k = lambda name: wi.weight_scale_k(wi.case(name))
    assert [k(f"pow2_{e}") for e in (-3, 0, 5)] == [11, 8, 3]
    assert [k(f"below_pow2_{e}") for e in (-3, 0, 5)] == [12, 9, 4]
    assert k("zero") == 0 and k("inf") == 0 and k("ties") == 0
    assert k("sub_2^-140") == 100 and k("tiny_2^-110") == 100 and k("big_2^110") == -102 and k("big_2^117") == -109
    assert k("max_first") == k("max_last") == 10 and k("max_negative") == 9
    w = np.array(wi.case("glorot"))
    k0 = wi.weight_scale_k(w)
    w.reshape(-1)[5] = np.nan
    assert wi.weight_scale_k(w) == k0
    assert wi.weight_scale_k(np.full((3, 3, 128, 128), 3.2e38, np.float32)) == 0
    assert wi.weight_scale_k(np.full((3, 3, 128, 128), 2.9e38, np.float32)) == -119
