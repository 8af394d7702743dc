"""The sub-rectangle layers of the towers with 16-bit activations, one launch at a time, against tests/rect16_ref.py.

The three towers (SNK_CONV_ALGO=f16a / bf16 / mxfp8) share the 16-bit block frame of csrc/conv_split.hip; its sub-rectangle form
(snk_conv3x3_bn_{f16,bf16,mxfp8}_act16_rect on the descriptors of snk_conv_rect_plan_act16) has code of its own -- the a16 cut of
hs_rect_parts, the prologue that zeroes only the border slots of an LDS row, the buffer-descriptor epilogue with its own choice between
the shortcut and its background image, its own fill loop, the f16 tower's output range flag -- that the suite reached through whole-net
Q comparisons only, and there only with the 6- to 8-tile bodies.  Here every launch is one layer on hand-made bounding boxes
(rect16_ref.CASES_37 on a 37 x 37 canvas, CASES_9x13 on 9 x 13: every tile count 1 .. 8, part counts 1, 2, 3 and 6, shapes the LDS
rows or the staging items limit, rectangles on every canvas edge and on none, widths and heights of one pixel;
tests/test_rect16_ref_cpu.py asserts that coverage).

Set-up of a launch: planes are the background (0, 1, 0) with a foreign pixel at two corners of each box; x and the shortcut are random
16-bit tensors that hold NaN outside the box grown by grow_in / grow_res (what the producing layer did not write must not be read);
bg_in / bg_res / bg_out are random finite images; the output holds NaN and is followed by one image of NaN.

  plan      snk_conv_rect_plan_act16 against rect16_ref.plan: boxes, descriptors per tile-count bin, counts, nothing past the count
  layer     per kind, rectangle grow g with (grow_in, grow_res) = (g - 1, g - 2) as QNet sets them, and (3, 0, 0); with / without
            shortcut and bg_out.  On the rectangles: the bits of the kind's full-form entry on the composed input (each output is the
            same chain of MFMAs on the same operands); finite; and within the bound of test_act16_layer_in_the_batched_frame /
            test_random_layer_against_the_dequantized_operands of float64 on the same rounded operands (rect16_ref.layer):
            |out - want| <= ulp |want| + 2e-5 max|ref|, more than 0.99 bit-equal.  Outside them: the NaN pattern, or bg_out's bits.
  one-hot   a kernel that is 1 at one tap, exact integer data: the output is a shift of the composed input, bit for bit
  flag      the f16 tower's range flag stays 0 through all of that, and is raised (output 65504, no infinity) by a large scale
  refusals  NULL, in place, grow_in = 128, a canvas too large: < 0, named after the entry point called, nothing written

Measured on an MI355X, this module's own run (93 tests, 7.2 s; the float64 convolutions are made on the CPU, once per canvas, kind and
grow_in).  Over the 40 layer launches of a kind (20 cases x 2 canvases); the excess is max(|out - want| - bound), negative = inside
the bound everywhere (it is the bound at an output of 0 that both sides agree on); error / bound is the largest ratio, a one-ulp
difference at a value just above a power of two comes close to 1:

  kind    worst excess over the bound   largest error / bound   smallest bit-equal share
  f16a    -1.67e-04                     0.923                   0.99932
  bf16    -1.67e-04                     0.929                   0.99983
  mxfp8   -1.03e-04                     0.993                   0.99406

  time per test (call)                  f16a              bf16              mxfp8
  test_layer_on_the_rectangles          <= 0.70 s (first) <= 0.12 s         <= 0.19 s        (60 cases, 3.0 s in all)
  test_one_hot_tap_is_a_shift_...       <= 0.20 s         <= 0.10 s         <= 0.08 s        (27 cases, 2.2 s in all)
  test_plan_matches_the_model           0.29 s + 1.5 s for the first canvas's data and plan; every other test < 0.1 s

Every assertion holds: no wrong result was found in the kernels.
"""
import ctypes as C

import numpy as np
import pytest

import mxfp8_ref as mx
import rect16_ref as rr

pytestmark = pytest.mark.gpu

KINDS = ["f16a", "bf16", "mxfp8"]
# (rectangle grow, grow_in, grow_res): the production relation (tower layer i: i + 2, i + 1, i) and one setting off it
SETTINGS = [(g, max(g - 1, 0), max(g - 2, 0)) for g in rr.GROW] + [(3, 0, 0)]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    from snake_engine._lib import lib, check
    return torch, lib(), check


def _st():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _kind(torch, L, kind):
    """(16-bit type, its name, ulp, full-form entry, sub-rectangle entry, prepare_weights)"""
    if kind == "f16a":
        return (torch.float16, "f16", 2.0 ** -10, L.snk_conv3x3_bn_f16_act16, L.snk_conv3x3_bn_f16_act16_rect,
                L.snk_conv3x3_prepare_weights_f16_act16)
    if kind == "bf16":
        return (torch.bfloat16, "bf16", 2.0 ** -7, L.snk_conv3x3_bn_bf16_act16, L.snk_conv3x3_bn_bf16_act16_rect,
                L.snk_conv3x3_prepare_weights_bf16)
    return (torch.bfloat16, "bf16", 2.0 ** -7, L.snk_conv3x3_bn_mxfp8_act16, L.snk_conv3x3_bn_mxfp8_act16_rect,
            L.snk_conv3x3_prepare_weights_mxfp8)


def _weights(env, kind, w):
    """the kind's weight image of the float32 HWIO kernel w (a device tensor)"""
    torch, L, check = env
    from snake_engine.net import F16S_WEIGHT_BYTES
    wS = torch.zeros(F16S_WEIGHT_BYTES, dtype=torch.uint8, device="cuda")
    check(_kind(torch, L, kind)[5](w.data_ptr(), wS.data_ptr(), _st()))
    return wS


def _flag(wS):
    """the range flag: the fifth 32-bit word of the weight image's tail"""
    return int(wS[-32:].cpu().numpy().view(np.int32)[4])


def _bits(t):
    import torch
    return t.view(torch.int16)


_DATA = {}


def _canvas(env, H, W):
    """everything of a canvas that does not depend on the kind -- made once, read-only afterwards"""
    torch, L, check = env
    if (H, W) in _DATA:
        return _DATA[H, W]
    boxes = dict((c[:2], c[2]) for c in rr.CANVASES)[H, W]
    n = len(boxes)
    g = torch.Generator(device="cuda").manual_seed(100 * H + W)
    planes = torch.tensor([0.0, 1.0, 0.0]).repeat(n, H, W, 1)
    for i, (y0, x0, y1, x1) in enumerate(boxes):
        planes[i, y0, x0] = torch.tensor([0.3, 0.2, 0.1])
        planes[i, y1, x1] = torch.tensor([0.0, 0.0, 1.0])
    d = dict(boxes=boxes, n=n, planes=planes.cuda().contiguous(), ref={}, full={})
    for name in ("x", "r"):
        d[name] = torch.randn(n, H, W, 128, device="cuda", generator=g)
    for name in ("bg_in", "bg_res", "bg_out"):
        d[name] = torch.randn(H, W, 128, device="cuda", generator=g)
    d["w"] = (torch.randn(3, 3, 128, 128, device="cuda", generator=g) * 0.05).contiguous()
    d["sc"] = torch.rand(128, device="cuda", generator=g) + 0.5
    d["sh"] = torch.randn(128, device="cuda", generator=g) * 0.1
    d["inside"] = {k: torch.as_tensor(rr.inside(boxes, k, H, W)).cuda() for k in range(0, 4)}
    # the plan of the four rectangle grows, made by the library
    mb = int(L.snk_conv_rect_max_blocks_act16(n, H, W))
    assert mb > 0
    desc = torch.full((len(rr.GROW), mb, 4), -1, dtype=torch.int32, device="cuda")
    counts = torch.zeros((len(rr.GROW), 2), dtype=torch.int32, device="cuda")
    bbox = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    check(L.snk_conv_rect_plan_act16(_p(d["planes"]), 0.0, 1.0, 0.0, n, H, W, len(rr.GROW), (C.c_int * len(rr.GROW))(*rr.GROW),
                                     _p(bbox), _p(desc), _p(counts), _st()))
    torch.cuda.synchronize()
    d.update(mb=mb, desc=desc, counts=counts, bbox=bbox)
    _DATA[H, W] = d
    return d


def _tensors(env, H, W, t16name):
    """the 16-bit tensors of a canvas: x / r with NaN outside the box grown by k (x_k, r_k), the background images"""
    torch = env[0]
    d = _canvas(env, H, W)
    key = "t_" + t16name
    if key not in d:
        dt = torch.float16 if t16name == "f16" else torch.bfloat16
        nan = torch.full((), float("nan"), dtype=dt, device="cuda")
        t = {name: d[name].to(dt).contiguous() for name in ("x", "r", "bg_in", "bg_res", "bg_out")}
        for k, m in d["inside"].items():
            t["x", k] = torch.where(m[..., None], t["x"], nan).contiguous()
            t["r", k] = torch.where(m[..., None], t["r"], nan).contiguous()
        t["r64"], t["bg_res64"] = t["r"].double().cpu().numpy(), t["bg_res"].double().cpu().numpy()      # the reference's host copies
        t["sc64"], t["sh64"] = d["sc"].double().cpu().numpy(), d["sh"].double().cpu().numpy()
        d[key] = t
    return d[key]


def _rounded_weights(torch, kind, w):
    """float64 NumPy: the kernel as the kind's prepare_weights rounds it"""
    if kind == "f16a":
        ws = 2.0 ** (8 - int(torch.floor(torch.log2(w.abs().max())).item()))     # the kernel's weight scale: max|w| -> [256, 512)
        return ((w * ws).to(torch.float16).double() / ws).cpu().numpy()
    if kind == "bf16":
        return w.to(torch.bfloat16).double().cpu().numpy()
    return mx.mx_round(w.cpu().numpy(), axis=2)


def _ref_conv(env, H, W, kind, grow_in):
    """float64 convolution of the composed, rounded operands -- once per (canvas, kind, grow_in), shared and never modified"""
    torch = env[0]
    d = _canvas(env, H, W)
    if (kind, grow_in) not in d["ref"]:
        t = _tensors(env, H, W, _kind(torch, env[1], kind)[1])
        xc = rr.compose(t["x"].double().cpu().numpy(), t["bg_in"].double().cpu().numpy(), d["boxes"], grow_in, H, W)
        if kind == "mxfp8":
            xc = mx.mx_round(xc, axis=3)
        if ("w", kind) not in d["ref"]:
            d["ref"]["w", kind] = _rounded_weights(torch, kind, d["w"])
        d["ref"][kind, grow_in] = rr.conv3x3(xc, d["ref"]["w", kind])
    return d["ref"][kind, grow_in]


def _launch(env, kind, H, W, g, grow_in, grow_res, res, fill, wS, sc, sh, x=None, bg_in=None):
    """one sub-rectangle launch on the plan's descriptors of rectangle grow g; returns the output (n + 1 images, NaN before)"""
    torch, L, check = env
    d = _canvas(env, H, W)
    dt, name, _, _, rect, _ = _kind(torch, L, kind)
    t = _tensors(env, H, W, name)
    out = torch.full((d["n"] + 1, H, W, 128), float("nan"), dtype=dt, device="cuda")
    li = rr.GROW.index(g)
    check(rect(_p(t["x", grow_in] if x is None else x), _p(wS), _p(sc), _p(sh), _p(t["r", grow_res]) if res else None, _p(out),
               _p(d["desc"][li]), _p(d["counts"][li]), _p(t["bg_in"] if bg_in is None else bg_in), grow_in,
               _p(t["bg_res"]) if res else None, grow_res, _p(t["bg_out"]) if fill else None, d["n"], H, W, _st()))
    return out


def _outside_is_untouched(torch, d, out, on, fill_image):
    """the image behind the batch and (fill_image None) every pixel outside the rectangles still hold the NaN pattern they were
    filled with; with a fill image the pixels outside hold its bits"""
    n = d["n"]
    nanbits = _bits(torch.full((1,), float("nan"), dtype=out.dtype, device="cuda"))[0]
    assert (_bits(out[n]) == nanbits).all(), "something was written behind the last image"
    off = ~on
    if fill_image is None:
        assert (_bits(out[:n])[off] == nanbits).all(), "a pixel outside the rectangle was written"
    else:
        want = _bits(fill_image).expand(n, -1, -1, -1)
        assert torch.equal(_bits(out[:n])[off], want[off]), "outside the rectangle the canvas does not hold bg_out's bits"


# ---- the plan ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [c[:2] for c in rr.CANVASES])
def test_plan_matches_the_model(env, H, W):
    torch, L, check = env
    d = _canvas(env, H, W)
    boxes, n, mb = d["boxes"], d["n"], d["mb"]
    assert mb == rr.max_blocks(n, H, W)
    assert int(L.snk_conv_rect_max_blocks_act16(0, H, W)) == 0
    if (H, W) == (37, 37):
        assert mb != int(L.snk_conv_rect_max_blocks(n, H, W)), "the 16-bit frame cuts a 37 x 37 canvas differently"
    bb = d["bbox"].cpu().numpy().view(np.uint32)
    assert [int(b) for b in bb] == [rr.box_word(b) for b in boxes]
    dh, ch = d["desc"].cpu().numpy().view(np.uint32), d["counts"].cpu().numpy()
    for li, lp in enumerate(rr.plan(boxes, rr.GROW, H, W)):
        assert (int(ch[li, 0]), int(ch[li, 1])) == (lp.count, lp.tiles), (li, ch[li], lp.count, lp.tiles)
        assert lp.count <= mb and (dh[li, lp.count:] == 0xFFFFFFFF).all(), "something was written past the count"
        o = 0
        for tm, want in lp.bins:                                   # largest first; inside a bin the order is the atomics'
            got = sorted(tuple(int(v) for v in row) for row in dh[li, o:o + len(want)])
            assert got == want, (li, tm, [a for a in got if a not in want][:3], [a for a in want if a not in got][:3])
            o += len(want)
        assert o == lp.count


# ---- one layer --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("g,grow_in,grow_res", SETTINGS)
@pytest.mark.parametrize("kind", KINDS)
def test_layer_on_the_rectangles(env, kind, g, grow_in, grow_res, res, fill):
    torch, L, check = env
    for H, W, _ in rr.CANVASES:
        d = _canvas(env, H, W)
        n, boxes = d["n"], d["boxes"]
        dt, name, ulp, full, _, _ = _kind(torch, L, kind)
        t = _tensors(env, H, W, name)
        if ("wS", kind) not in d:
            d["wS", kind] = _weights(env, kind, d["w"])
        wS = d["wS", kind]
        out = _launch(env, kind, H, W, g, grow_in, grow_res, res, fill, wS, d["sc"], d["sh"])
        on = d["inside"][g]
        _outside_is_untouched(torch, d, out, on, t["bg_out"] if fill else None)
        got = out[:n]
        assert torch.isfinite(got[on]).all(), "a NaN pixel (outside the producer's rectangle) was read"
        # the full-form entry on the composed input: once per (kind, grow_in, shortcut's grow)
        fkey = (kind, grow_in, grow_res if res else None)
        if fkey not in d["full"]:
            xc = torch.where(d["inside"][grow_in][..., None], t["x"], t["bg_in"]).contiguous()
            rc = torch.where(d["inside"][grow_res][..., None], t["r"], t["bg_res"]).contiguous() if res else None
            fo = torch.full((n + 1, H, W, 128), float("nan"), dtype=dt, device="cuda")
            check(full(_p(xc), _p(wS), _p(d["sc"]), _p(d["sh"]), _p(rc), _p(fo), 1, n, H, W, 1, _st()))
            assert torch.isnan(fo[n]).all() and torch.isfinite(fo[:n]).all()
            d["full"][fkey] = fo[:n]
        fo = d["full"][fkey]
        diff = (_bits(got) != _bits(fo)) & on[..., None]
        assert not diff.any(), (f"{int(diff.sum())} values differ from the full form, first at (image, y, x, channel) "
                                f"{torch.nonzero(diff)[0].tolist()}")
        # float64 of the same rounded operands
        ref = rr.layer(None, None, boxes, grow_in, None, t["sc64"], t["sh64"], t["r64"] if res else None,
                       t["bg_res64"] if res else None, grow_res, conv=_ref_conv(env, H, W, kind, grow_in))
        ref = torch.as_tensor(ref).cuda()[on]
        want = ref.to(dt)
        scale = ref.abs().max().item()
        err, bound = (got[on].double() - want.double()).abs(), ulp * want.double().abs() + 2e-5 * scale
        over, used = (err - bound).max().item(), (err / bound).max().item()
        same = (_bits(got[on]) == _bits(want)).float().mean().item()
        print(f"FIGURE {kind} {H}x{W} g={g} in={grow_in} res={grow_res if res else None} fill={int(fill)}: bit-equal {same:.5f}, "
              f"worst excess over the bound {over:.3g}, largest error / bound {used:.3f}, max|ref| {scale:.3g}")
        assert over <= 0, over
        assert same > 0.99, same
        if kind == "f16a":
            assert _flag(wS) == 0, "the f16 tower's range flag was raised by an ordinary layer"


# ---- one-hot taps -----------------------------------------------------------------------------------------------------------

def _exact(torch, g, *lead):
    """integers |v| <= 15 times 2^-2 .. 2^2 per 32-channel block: exact in f16, bf16 and MX-FP8 (float32 device tensor)"""
    v = torch.randint(-15, 16, lead + (128,), device="cuda", generator=g).float()
    e = torch.randint(-2, 3, lead + (4,), device="cuda", generator=g).float()
    return v * torch.exp2(e).repeat_interleave(32, dim=-1)


@pytest.mark.parametrize("tap", range(9))
@pytest.mark.parametrize("kind", KINDS)
def test_one_hot_tap_is_a_shift_of_the_composed_input(env, kind, tap):
    torch, L, check = env
    dt, name = _kind(torch, L, kind)[:2]
    w = torch.zeros(3, 3, 128, 128, device="cuda")
    w[tap // 3, tap % 3] = torch.eye(128, device="cuda")
    wS = _weights(env, kind, w)
    one, zero = torch.ones(128, device="cuda"), torch.zeros(128, device="cuda")
    nan = torch.full((), float("nan"), dtype=dt, device="cuda")
    for H, W, boxes in rr.CANVASES:
        d = _canvas(env, H, W)
        n = d["n"]
        if "hot" not in d:
            gen = torch.Generator(device="cuda").manual_seed(7 * H + W)
            x, bg = _exact(torch, gen, n, H, W), _exact(torch, gen, H, W)
            d["hot"] = (x, bg, x.double().cpu().numpy(), bg.double().cpu().numpy())
        x, bg, xh, bgh = d["hot"]
        assert torch.equal(x.to(dt).float(), x) and torch.equal(bg.to(dt).float(), bg)
        for g, grow_in, _ in SETTINGS:
            xin = torch.where(d["inside"][grow_in][..., None], x.to(dt), nan).contiguous()
            out = _launch(env, kind, H, W, g, grow_in, 0, False, False, wS, one, zero, x=xin, bg_in=bg.to(dt).contiguous())
            on = d["inside"][g]
            _outside_is_untouched(torch, d, out, on, None)
            e = rr.one_hot_expected(xh, bgh, boxes, grow_in, tap)
            want = torch.as_tensor(e + 0.0).cuda().to(dt)                     # (+ 0.0: no negative zero)
            assert torch.equal(want.double().cpu(), torch.as_tensor(e)), "the expected values are not exact in the 16-bit type"
            diff = (_bits(out[:n]) != _bits(want)) & on[..., None]
            if diff.any():
                i, y, xx, c = torch.nonzero(diff)[0].tolist()
                print(f"{kind} tap {tap} {H}x{W} g={g} grow_in={grow_in}: {int(diff.sum())} values differ, first at image {i} "
                      f"(box {boxes[i]}) y {y} x {xx} channel {c}: got {out[i, y, xx, c].item()} want {want[i, y, xx, c].item()}")
            assert not diff.any()
        if kind == "f16a":
            assert _flag(wS) == 0


# ---- the f16 tower's range flag -----------------------------------------------------------------------------------------------

def test_f16_range_flag_is_raised_by_a_saturated_rectangle(env):
    """a scale that pushes the rectangles' outputs past 65504: they are written as 65504, none as infinity, and the flag word is set"""
    torch, L, check = env
    H = W = 37
    d = _canvas(env, H, W)
    wS = _weights(env, "f16a", d["w"])
    assert _flag(wS) == 0
    big = (d["sc"] * 1e6).contiguous()
    out = _launch(env, "f16a", H, W, 2, 1, 0, False, False, wS, big, d["sh"])
    on = d["inside"][2]
    _outside_is_untouched(torch, d, out, on, None)
    got = out[:d["n"]][on]
    assert torch.isfinite(got).all() and got.max().item() == 65504.0 and got.min().item() == 0.0
    conv = torch.as_tensor(_ref_conv(env, H, W, "f16a", 1)).cuda()[on]
    far = (conv * big.double() + d["sh"].double()) > 2 * 65504.0
    assert far.any() and (got[far] == 65504.0).all()
    assert _flag(wS) != 0, "outputs were saturated and the range flag stayed 0"


# ---- refusals -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_refusals_name_the_entry_point_and_write_nothing(env, kind):
    torch, L, check = env
    H, W = 9, 13
    d = _canvas(env, H, W)
    n = d["n"]
    dt, name, _, _, rect, _ = _kind(torch, L, kind)
    t = _tensors(env, H, W, name)
    if ("wS", kind) not in d:
        d["wS", kind] = _weights(env, kind, d["w"])
    fname = {"f16a": b"snk_conv3x3_bn_f16_act16_rect", "bf16": b"snk_conv3x3_bn_bf16_act16_rect",
             "mxfp8": b"snk_conv3x3_bn_mxfp8_act16_rect"}[kind]
    out = torch.full((n + 1, H, W, 128), float("nan"), dtype=dt, device="cuda")
    x = t["x", 1].clone()
    x_before = _bits(x).clone()
    a = dict(x=_p(x), wS=_p(d["wS", kind]), sc=_p(d["sc"]), sh=_p(d["sh"]), res=_p(t["r", 0]), out=_p(out), desc=_p(d["desc"][2]),
             count=_p(d["counts"][2]), bg_in=_p(t["bg_in"]), grow_in=1, bg_res=_p(t["bg_res"]), grow_res=0, bg_out=_p(t["bg_out"]),
             n=n, H=H, W=W)

    def call(**kw):
        b = dict(a, **kw)
        return rect(b["x"], b["wS"], b["sc"], b["sh"], b["res"], b["out"], b["desc"], b["count"], b["bg_in"], b["grow_in"], b["bg_res"],
                    b["grow_res"], b["bg_out"], b["n"], b["H"], b["W"], _st())
    bad = [dict(x=None), dict(wS=None), dict(sc=None), dict(sh=None), dict(out=None), dict(desc=None), dict(count=None),
           dict(out=a["x"]), dict(grow_in=128), dict(grow_res=128), dict(grow_in=-1), dict(H=2), dict(W=81), dict(H=81, W=81), dict(n=-1)]
    for kw in bad:
        assert call(**kw) < 0, kw
        assert fname + b":" in L.snk_last_error(), (kw, L.snk_last_error())
    # no images: the f16 and bf16 entries return at once, the mxfp8 entry refuses (its full-form entry does too)
    if kind == "mxfp8":
        assert call(n=0) < 0 and fname in L.snk_last_error()
    else:
        assert call(n=0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.equal(_bits(x), x_before), "a refused call wrote something"
    assert call() == 0                                              # and the same arguments, unspoiled, are a launch
    torch.cuda.synchronize()
    assert torch.isfinite(out[:n][d["inside"][2]]).all() and torch.isnan(out[n]).all()
