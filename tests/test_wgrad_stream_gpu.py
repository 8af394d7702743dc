"""The weight gradient of the tower convolution (csrc/train_wgrad.hip) with SEVERAL images per image group, against its definition
in float64 (tests/wgrad_ref.py::dw_ref; alpha_nnet.py:58-59 under Keras fit).

The form the training step runs, k_wgrad2_f16s, cuts the batch into 128 image groups and reads a group as ONE slot stream: image i,
row y, column x at slot (i (H + 1) + y) (W + 1) + x, the zero column behind a row and the zero row behind an image as the taps'
padding, windows of 16 NK slots whatever the image boundaries.  Below 129 images a group holds one image at most, and nothing of
that is exercised: the division by H + 1, the zero row that is the padding of two images, a window that starts in one image and ends
in the next, a shorter last group, and the deferred batch norm's rule that padding BETWEEN two images stays zero.  The cases of
wgrad_ref.CASES put 2 .. 5 images into a group (the product: 16) in every kernel body the launcher reaches at default settings --
six window bodies and the slab form k_wgrad_f16s, which tests/test_wgrad_ref_cpu.py holds against the launcher's dispatch -- on
square and on narrow rectangular images (H != W: the row pitch W + 1 and the image pitch H + 1 are different numbers).

Every launch finds NaN in the partials and in dw (a group without images must write its zeros), and its operands inside larger
allocations with NaN in front of and behind them (a read outside the tensors shows in the result).

Not covered: SNK_WGRAD_NK, a development knob.  The launch line only it reaches, (4, 4, 21), stays untested, and so do the NK = 4
bodies at the widths that take NK = 5 by default."""
import os
import subprocess
import sys

import pytest

import wgrad_ref

pytestmark = pytest.mark.gpu

_ID = lambda c: f"{c[0]}x{c[1]}x{c[2]}"


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def run():
    from helpers import wgrad_runner
    return wgrad_runner


def rel(a, b):
    return float((a.detach().double() - b.detach().double()).abs().max() / (b.detach().double().abs().max() + 1e-300))


_EXACT = {}


def _exact(run, L, n, h, w):
    """the integer operands of a case and their float64 gradient: once, shared, left unchanged"""
    if (n, h, w) not in _EXACT:
        _EXACT[(n, h, w)] = run.exact_case(L, n, h, w)
    return _EXACT[(n, h, w)]


@pytest.mark.parametrize("case", wgrad_ref.CASES, ids=_ID)
def test_integer_operands_give_the_gradient_bit_for_bit(torch_gpu, run, case):
    """x and dy hold integers in -3 .. 3 and their scales are 2^10: every v 2^10 is an exact f16 (the lo halves are zero), every
    product and every float32 partial sum an integer multiple of 2^20 below 2^44, the fold runs in float64 and the last scale is a
    power of two -- so dw EQUALS the float64 gradient, in the split entry and in the single-pass f16 entry, with no tolerance.  A
    kernel that took a neighbour image's edge row as halo, or lost a slot at a window's or a group's end, differs by integers."""
    torch = torch_gpu
    from snake_engine._lib import lib, EngineError
    n, h, w, body, pattern = case
    L = lib()
    assert L.snk_train_deferred_bn_supported(h, w) == (0 if body == "slab" else 1)        # the library's own word on which form runs
    c = _exact(run, L, n, h, w)
    dw = run.launch(L, "snk_conv3x3_wgrad_f16s", c["x"], c["dy"], c["tx"], c["tdy"], n, h, w)
    differ = int((dw.double() != c["ref"]).sum())
    print(f"wgrad exact {n} x {h} x {w}: body {body}, groups {pattern}, largest entry {float(c['ref'].abs().max()):.0f}, split entry differs in {differ}")
    assert float(c["ref"].abs().max()) > 0
    assert torch.equal(dw.double(), c["ref"]), differ
    if body == "slab":
        with pytest.raises(EngineError, match="has no single-pass f16 variant"):
            run.launch(L, "snk_conv3x3_wgrad_f16", c["x"], c["dy"], c["tx"], c["tdy"], n, h, w)
    else:
        dw16 = run.launch(L, "snk_conv3x3_wgrad_f16", c["x"], c["dy"], c["tx"], c["tdy"], n, h, w)
        assert torch.equal(dw16.double(), c["ref"]), int((dw16.double() != c["ref"]).sum())


@pytest.mark.parametrize("case", wgrad_ref.CASES, ids=_ID)
def test_deferred_batch_norm_keeps_the_padding_between_two_images_zero(torch_gpu, run, case):
    """the deferred entries read y_below and take every value as relu(y * scale + shift).  y_below holds integers in -3 .. 3, the
    scales are 1, -1 or 2 and the shifts 0, 1 or 2 (three of four channels positive): the activation is an exact integer, and a
    padding slot -- the zero column behind a row, the zero row between two images of a group -- that went through the transform would
    enter as its channel's shift.  dw EQUALS the float64 gradient of the written activation, bit for bit, in both deferred entries;
    the slab form refuses the deferred input with its message."""
    torch = torch_gpu
    from snake_engine._lib import lib, EngineError
    n, h, w, body, pattern = case
    L = lib()
    c = _exact(run, L, n, h, w)
    scale, shift = run.channel_transform()
    assert int((shift > 0).sum()) == 96 and int((scale < 0).sum()) > 0
    if body == "slab":
        with pytest.raises(EngineError, match="run the slab form, which has no deferred input"):
            run.launch(L, "snk_conv3x3_wgrad_f16s_deferred", c["x"], c["dy"], c["tx"], c["tdy"], n, h, w, scale, shift)
        return
    act = torch.relu(c["x"] * scale + shift)                  # what snk_bn_train_apply would have written
    ta = run.tail_of(L, act)                                 # the range of the written activation's maximum
    amax = float(act.max())
    assert amax == 8.0 and float(ta[2]) == 256.0 and float(ta[3]) == 2.0 ** -8
    ref = wgrad_ref.dw_ref(act, c["dy"])
    assert float(wgrad_ref.dw_ref(act, c["dy"].abs()).max()) < 2.0 ** 24       # the precondition: exact float32 partial sums
    assert not torch.equal(ref, c["ref"])
    for entry in ("snk_conv3x3_wgrad_f16s_deferred", "snk_conv3x3_wgrad_f16_deferred"):
        dw = run.launch(L, entry, c["x"], c["dy"], ta, c["tdy"], n, h, w, scale, shift)
        differ = int((dw.double() != ref).sum())
        print(f"wgrad exact {n} x {h} x {w}: body {body}, {entry} differs in {differ}")
        assert torch.equal(dw.double(), ref), (entry, differ)


def _rounded(torch, v, s):
    """the single-pass rule: f16(v * s), round to nearest even, as a float64 value of v's magnitude (tests/test_train_f16_gpu.py)"""
    return (v * s).to(torch.float16).double() / float(s)


# (case, xmag, gmag): the operand magnitudes of test_tower_convolution_three_passes_match_float64, both ends of the scale range
_FLOAT_CASES = [(wgrad_ref.CASES[0], 1.0, 1.0), (wgrad_ref.CASES[2], 1.0, 1e-4), (wgrad_ref.CASES[3], 30.0, 1e-6), (wgrad_ref.CASES[9], 1e-3, 50.0)]


@pytest.mark.parametrize("case,xmag,gmag", _FLOAT_CASES, ids=[_ID(c[0]) for c in _FLOAT_CASES])
def test_random_floats_match_float64_with_the_lo_planes(torch_gpu, run, case, xmag, gmag):
    """randn * xmag against a gradient with a rand ** 6 spread of magnitudes, as real gradients have: the lo planes carry weight.  The
    split entry against float64 on the unrounded operands, the single-pass f16 entry against float64 on the operands rounded by its
    rule; the bound is the kernel's own, 3e-6 of the largest entry (tests/test_train_ops_gpu.py, measured there at n <= 64).  The
    float32 error of the same nine products is printed beside it as a yardstick.  Measured on one MI355X (split entry / float32
    products / f16 entry on its rounded operands): 129 x 21 x 21 3.9e-7 / 5.8e-6 / 1.9e-7, 130 x 37 x 37 7.0e-7 / 6.6e-6 / 3.6e-7,
    385 x 4 x 13 2.3e-7 / 2.8e-6 / 1.1e-7, 35 x 3 x 47 (slab form) 1.8e-7 / 2.2e-6 / refused."""
    torch = torch_gpu
    from snake_engine._lib import lib, EngineError
    n, h, w, body, pattern = case
    assert (n, h, w) in ((129, 21, 21), (130, 37, 37), (385, 4, 13), (35, 3, 47))
    L = lib()
    g = torch.Generator(device="cuda").manual_seed(n)
    x = torch.randn(n, h, w, 128, device="cuda", generator=g) * xmag
    dy = torch.randn(n, h, w, 128, device="cuda", generator=g) * gmag
    dy = dy * (torch.rand(n, h, w, 1, device="cuda", generator=g) ** 6)
    x, dy = run.guarded(x), run.guarded(dy)
    tx, tdy = run.tail_of(L, x), run.tail_of(L, dy)
    ref = wgrad_ref.dw_ref(x, dy)
    e32 = rel(wgrad_ref.dw_ref(x, dy, torch.float32), ref)
    dw = run.launch(L, "snk_conv3x3_wgrad_f16s", x, dy, tx, tdy, n, h, w)
    e = rel(dw, ref)
    print(f"wgrad floats {n} x {h} x {w}: body {body}, groups {pattern}, split entry rel {e:.3g} (float32 products {e32:.3g})")
    assert e < 3e-6, (e, e32)
    if body == "slab":
        with pytest.raises(EngineError, match="has no single-pass f16 variant"):
            run.launch(L, "snk_conv3x3_wgrad_f16", x, dy, tx, tdy, n, h, w)
        return
    ref16 = wgrad_ref.dw_ref(_rounded(torch, x, float(tx[2])), _rounded(torch, dy, float(tdy[2])))
    dw16 = run.launch(L, "snk_conv3x3_wgrad_f16", x, dy, tx, tdy, n, h, w)
    e16, apart = rel(dw16, ref16), rel(dw16, ref)
    print(f"wgrad floats {n} x {h} x {w}: f16 entry rel {e16:.3g} on the rounded operands, {apart:.3g} on the unrounded")
    assert e16 < 3e-6, e16


def test_slab_form_behind_the_switch_with_three_images_per_group(torch_gpu):
    """SNK_WGRAD=slabs: k_wgrad_f16s as the A/B partner on the two canvases the window form took over (21 x 21; 37 x 37 in slabs of
    five image rows), 33 images in 16 groups of three.  The switch is read once per process, so tests/helpers/wgrad_runner.py runs as
    a child: the exact-integer check of the split entry for both shapes, and snk_train_deferred_bn_supported == 0."""
    from conftest import REPO
    helper = os.path.join(REPO, "tests", "helpers", "wgrad_runner.py")
    r = subprocess.run([sys.executable, helper], env=dict(os.environ, SNK_WGRAD="slabs"), capture_output=True, text=True, timeout=240)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    for n, h, w, pattern in wgrad_ref.SLAB_SWITCH:
        assert f"ok {n} x {h} x {w} slab form" in r.stdout
    assert f"wgrad slabs: {len(wgrad_ref.SLAB_SWITCH)} cases exact" in r.stdout
