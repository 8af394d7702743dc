"""The child process of tests/test_stem_forms_gpu.py: every launch form of the inference stem (csrc/net.hip) against the float64
model tests/stem_head_ref.py.  SNK_STEM, SNK_STEM_GRID and SNK_STEM_GROUP are read once per process, so each configuration is one
run of this program: `stem_forms_runner.py default | group1 | group2_grid3`, the environment set by the caller.

Every output buffer holds NaN before the launch and has one image of slack behind it that must still be all NaN afterwards.  A
line `fig <entry> <case> <figure> <bound>` is printed before each assertion, `max <entry> ...` at the end.  Tolerances:
  float32 output  max |out - ref| <= 3e-6 max |ref|                       (tests/test_net_gpu.py::test_stem_shapes_and_forms)
  f16 output      |out - ref| <= 2^-10 |ref| + 1e-5 per element           (the same test)
  bf16 output     |out - ref| <= 2^-8 |ref| + 3e-6 max |ref| per element  (bf16 keeps 8 significant bits: rounding the float32 value
                  to nearest moves it by at most half an ulp <= 2^-8 of it, and that value is within the float32 bound of the
                  reference; truncation instead of rounding would reach 2^-7)
The figure of a 16-bit output is the largest |out - ref| / bound over the elements (<= 1 passes; measured 0.50 for f16, whose
rounding is within 2^-11, and 0.99 for bf16, whose first term is the rounding's own bound)."""
import os
import sys

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO = os.path.dirname(TESTS)
for _p in (TESTS, REPO, os.path.join(REPO, "alphasnake-zero_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np
import torch

import stem_head_ref as R

CONFIGS = {"default": {}, "group1": {"SNK_STEM_GROUP": "1"}, "group2_grid3": {"SNK_STEM_GROUP": "2", "SNK_STEM_GRID": "3"}}
NAN = float("nan")
C = R.C

# (n, H, W): what each reaches in the default configuration (G = images per block iteration of k_stem_conv_mfma)
FULL = [(7, 35, 35),        # gap 3: G = 3, groups 3 + 3 + 1
        (5, 38, 38),        # gap 3: G = 3 at its upper edge, ragged 3 + 2
        (3, 45, 45),        # G = 2, ragged 2 + 1
        (2, 55, 55),        # gap 3: G = 1 from LDS pressure
        (1, 71, 71),        # gap 3: G = 1, 63 948 B of 65 536
        (2, 1, 300),        # single-row images
        (3, 1, 1),          # one pixel, one tile
        (2, 4, 8),          # exactly 32 pixels: one full tile, no clamped rows
        (2, 3, 11)]         # 33 pixels: a second tile with one live row
PERSIST = {"default": (2051, 5, 7),       # gap 4: 513 groups of 4 on 512 blocks, block 0 runs a second iteration with ng = 3
           "group1": (515, 5, 7),         # gap 4: 515 groups of 1 on 512 blocks
           "group2_grid3": (13, 5, 7)}    # gap 4: _f32 on 3 blocks, 7 groups of 2: three iterations, the last group of 1 image
FALLBACK = [(1, 72, 72),    # gap 5: 65 712 B of padded image -> k_stem_conv; 5184 pixels = 20 full blocks + 64
            (2, 3, 1200)]   # gap 5: blocks whose 256 pixels cross an image boundary
FULL_ENTRIES = ("snk_stem_conv_bn_relu_f32", "snk_stem_conv_bn_relu_f16out",
                "snk_stem_conv_bn_relu_bf16out",                                 # gap 2: the bf16 / MX-FP8 towers' stem
                "snk_stem_conv_f32")
RECT_ENTRIES = ("snk_stem_conv_bn_relu_f32_rect", "snk_stem_conv_bn_relu_f16out_rect", "snk_stem_conv_bn_relu_bf16out_rect")   # gap 1
DTYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

BOXES_21 = [(5, 5, 15, 15),          # the 11 x 11 window at (5, 5)
            (0, 0, 0, 0), (20, 20, 20, 20), (0, 20, 0, 20), (10, 0, 10, 0),      # one-pixel boxes: three corners and an edge
            (0, 0, 20, 20),          # the whole canvas
            (3, 2, 6, 9),            # 6 x 10 = 60 pixels at grow 1
            (4, 4, 9, 9)]            # 8 x 8 = 64 pixels at grow 1: an exact multiple of the 32-pixel tile
# (name, H, W, boxes (y0, x0, y1, x1) one per image, grow, configurations)
RECT = [("21x21g1", 21, 21, BOXES_21, 1, ("default", "group1")),
        ("21x21g3", 21, 21, BOXES_21, 3, ("default", "group1")),
        ("21x21g127", 21, 21, BOXES_21, 127, ("default", "group1")),            # cut to the canvas: every box becomes the whole image
        ("4x200", 4, 200, [(1, 150, 2, 199),                                     # x1 >= 128: bit 31 of the packed box
                           (0, 0, 3, 0), (0, 127, 0, 128)], 1, ("default", "group1")),
        ("37x37", 37, 37, [(10 + i, 5, 20, 30 - i) for i in range(7)], 1, ("default", "group1")),   # G = 3, unequal tile counts in a group
        ("2051x5x7", 5, 7, [(i % 5, i % 7, i % 5, i % 7) for i in range(2051)], 1, ("default",))]   # the second persistent iteration

FIG = {}


def kind_of(entry):
    return "bf16" if "bf16out" in entry else "f16" if "f16out" in entry else "f32"


def inputs(n, H, W, seed):
    """x = rand * 6 - 1 (the range observations live in), w = randn * 0.2, scale = rand + 0.5, shift = randn * 0.1"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, H, W, 3, generator=g) * 6 - 1
    w = torch.randn(3, 3, 3, C, generator=g) * 0.2
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    return x, w, scale, shift


def nan_out(n, H, W, kind):
    return torch.full((n + 1, H, W, C), NAN, dtype=DTYPE[kind], device="cuda")


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def launch(L, entry, d, out, n, H, W, bbox=None, grow=None):
    """d: device copies of (x, w, scale, shift).  Raises EngineError with the library's message where the call is refused."""
    from snake_engine._lib import check
    st = torch.cuda.current_stream().cuda_stream
    fn = getattr(L, entry)
    if entry == "snk_stem_conv_f32":
        check(fn(d[0].data_ptr(), d[1].data_ptr(), out.data_ptr(), n, H, W, st))
    elif entry.endswith("_rect"):
        check(fn(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out.data_ptr(),
                 bbox.data_ptr() if bbox is not None else None, grow, n, H, W, st))
    else:
        check(fn(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out.data_ptr(), n, H, W, st))
    torch.cuda.synchronize()


def hold(entry, case, got, ref, ref_max, where=None):
    """got, ref: float64 arrays of one shape; where: bool over the leading [n][H][W] axes (the elements compared) or None = all"""
    kind = kind_of(entry)
    if where is not None:
        got, ref = got[where], ref[where]
    assert np.isfinite(got).all(), (entry, case, "not finite")
    err = np.abs(got - ref)
    if kind == "f32":
        fig, bound = float(err.max()) / ref_max, 3e-6
    else:
        tol = 2.0 ** -10 * np.abs(ref) + 1e-5 if kind == "f16" else 2.0 ** -8 * np.abs(ref) + 3e-6 * ref_max
        fig, bound = float((err / tol).max()), 1.0
    print(f"fig {entry} {case} {fig:.3e} {bound:.0e}", flush=True)
    FIG[entry] = max(FIG.get(entry, 0.0), fig)
    assert fig <= bound, (entry, case, fig, bound)


def untouched(out):
    return bool(torch.isnan(out).all())


def refused(L, entry, d, out, n, H, W, bbox=None, grow=None):
    from snake_engine._lib import EngineError
    try:
        launch(L, entry, d, out, n, H, W, bbox, grow)
    except EngineError:
        assert untouched(out), (entry, n, H, W, "refused, but the buffer was written")
        return
    raise AssertionError((entry, n, H, W, grow, "was not refused"))


def full_case(L, shape, entries, keep=None):
    n, H, W = shape
    case = f"{n}x{H}x{W}"
    x, w, scale, shift = inputs(n, H, W, 1000 * H + W + n)
    d = [t.cuda() for t in (x, w, scale, shift)]
    ref = {False: R.stem(x.numpy(), w.numpy(), scale.numpy(), shift.numpy())}
    if "snk_stem_conv_f32" in entries:
        ref[True] = R.stem(x.numpy(), w.numpy(), None, None, raw=True)
    for entry in entries:
        raw = entry == "snk_stem_conv_f32"
        out = nan_out(n, H, W, kind_of(entry))
        launch(L, entry, d, out, n, H, W)
        assert untouched(out[n]), (entry, case, "the slack behind the output was written")
        hold(entry, case, out[:n].cpu().double().numpy(), ref[raw], float(np.abs(ref[raw]).max()))
        if keep is not None and not raw:
            keep[kind_of(entry)] = out
    return d, ref[False]


def rect_case(L, name, H, W, boxes, grow):
    """outside the grown box the buffer still holds NaN; inside, the float64 reference within the tolerance and the same dtype's
    full-canvas entry bit for bit"""
    n = len(boxes)
    full = {}
    d, ref = full_case(L, (n, H, W), FULL_ENTRIES[:3], keep=full)
    ref_max = float(np.abs(ref).max())
    packed = np.array([R.pack_bbox(*b) for b in boxes], dtype=np.uint32)
    inside = R.rect_mask(packed, grow, H, W)
    if name == "21x21g1":
        assert int(inside[6].sum()) == 60 and int(inside[7].sum()) == 64 and int(inside[1].sum()) == 4 and inside[5].all()
    if name == "21x21g127":
        assert inside.all()
    if name == "4x200":
        assert int(packed[0]) >> 31 == 1 and int(inside[0].sum()) == 4 * 51 and int(inside[2].sum()) == 2 * 4
    bbox = torch.from_numpy(packed.view(np.int32).copy()).cuda()       # as the caller holds them: one int32 per image
    m = torch.from_numpy(inside).cuda()
    for entry in RECT_ENTRIES:
        kind = kind_of(entry)
        out = nan_out(n, H, W, kind)
        launch(L, entry, d, out, n, H, W, bbox, grow)
        assert untouched(out[n]), (entry, name, "the slack behind the output was written")
        assert untouched(out[:n][~m]), (entry, name, "a pixel outside the grown box was written")
        hold(entry, name + f"/grow{grow}", out[:n].cpu().double().numpy(), ref, ref_max, where=inside)
        assert torch.equal(bits(out[:n])[m], bits(full[kind][:n])[m]), (entry, name, "differs from the full-canvas entry inside the box")
    return d, bbox


def rect_refusals(L):
    """what the host code rejects before any launch: grow 0, grow 128, no boxes"""
    n, H, W = 2, 21, 21
    d = [t.cuda() for t in inputs(n, H, W, 99)]
    bbox = torch.from_numpy(np.array([R.pack_bbox(5, 5, 15, 15)] * n, dtype=np.uint32).view(np.int32).copy()).cuda()
    for entry in RECT_ENTRIES:
        out = nan_out(n, H, W, kind_of(entry))
        refused(L, entry, d, out, n, H, W, bbox, 0)
        refused(L, entry, d, out, n, H, W, bbox, 128)
        refused(L, entry, d, out, n, H, W, None, 1)


def fallback_cases(L):
    for shape in FALLBACK:
        n, H, W = shape
        assert R.stem_lds_bytes(H, W) > R.LDS_64K
        d, _ = full_case(L, shape, FULL_ENTRIES[:1])                   # k_stem_conv
        for entry in FULL_ENTRIES[1:]:                                 # the MFMA-only entries refuse before any launch
            refused(L, entry, d, nan_out(n, H, W, kind_of(entry)), n, H, W)


def exact_properties(L):
    """gap 6: the MFMA form's scaling logic, on (3, 9, 9)"""
    n, H, W = 3, 9, 9
    x, w, scale, shift = inputs(n, H, W, 909)

    def raw(x_, w_):
        out = nan_out(n, H, W, "f32")
        launch(L, "snk_stem_conv_f32", [x_.cuda(), w_.cuda(), None, None], out, n, H, W)
        assert untouched(out[n])
        return out[:n]
    base = raw(x, w)
    assert bool(torch.isfinite(base).all()) and float(base.abs().max()) > 1.0
    # the weight scale is the power of two that brings max |w| to [256, 512): the split operands and every product of w 2^k are
    # those of w up to the exponent
    for k in (-20, -3, 1, 9, 20):
        got = raw(x, w * 2.0 ** k)
        assert torch.equal(bits(got), bits(base * 2.0 ** k)), ("weights x 2^k", k, int((bits(got) != bits(base * 2.0 ** k)).sum()))
    zero = raw(x, torch.zeros_like(w))                                 # max |w| = 0: scale 1, nothing divides by it
    assert bool((zero == 0).all()) and bool(torch.isfinite(zero).all())
    # inputs saturate at +-65504 / 1024 instead of becoming inf in the f16 split
    big, sat = x.clone(), x.clone()
    idx = torch.arange(0, x.numel(), 7)
    sign = torch.where(torch.arange(idx.numel()) % 2 == 0, 1.0, -1.0)
    big.view(-1)[idx] = 100.0 * sign
    sat.view(-1)[idx] = R.X_SAT * sign
    got_big, got_sat = raw(big, w), raw(sat, w)
    assert bool(torch.isfinite(got_big).all()) and torch.equal(bits(got_big), bits(got_sat))
    assert not torch.equal(bits(got_big), bits(base))
    # the f16 output saturates upwards instead of becoming inf
    out = nan_out(n, H, W, "f16")
    launch(L, "snk_stem_conv_bn_relu_f16out", [x.cuda(), w.cuda(), torch.full((C,), 1e6).cuda(), shift.cuda()], out, n, H, W)
    assert untouched(out[n]) and bool(torch.isfinite(out[:n]).all()) and float(out[:n].max()) == 65504.0
    assert bool((out[:n] == 0).any())


def main():
    config = sys.argv[1]
    want = CONFIGS[config]
    for k in ("SNK_STEM", "SNK_STEM_GRID", "SNK_STEM_GROUP"):
        assert os.environ.get(k) == want.get(k), (k, os.environ.get(k))
    from snake_engine._lib import lib
    L = lib()
    group_max = int(want.get("SNK_STEM_GROUP", 4))
    if config == "default":
        assert [R.stem_group(*s, group_max) for s in FULL[:5]] == [3, 3, 2, 1, 1]
    for shape in FULL:
        full_case(L, shape, FULL_ENTRIES)
    full_case(L, PERSIST[config], FULL_ENTRIES[:1] if config == "group2_grid3" else FULL_ENTRIES)
    for name, H, W, boxes, grow, configs in RECT:
        if config in configs:
            rect_case(L, name, H, W, boxes, grow)
    if config == "default":
        rect_refusals(L)
        fallback_cases(L)
        exact_properties(L)
    for entry in sorted(FIG):
        print(f"max {entry} {FIG[entry]:.3e} (bound {'3e-06 of max |ref|' if kind_of(entry) == 'f32' else '1 = the per-element tolerance'})")
    print(f"stem forms {config}: ok")


if __name__ == "__main__":
    main()
