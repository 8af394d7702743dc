"""The tower convolution's batched block frames against float64.

Every tower layer goes through conv_f16s_launch (csrc/conv_split.hip), which cuts an image (conv_f16s_plan) into blocks of up to 8 M tiles and runs
k_conv3x3_f16s<NI, MODE, ...>; a batch of at most 40 images is re-cut into one-tile blocks, and that is where every other layer-level
comparison of the suite lands (tests/test_conv_tiles_cpu.py asserts it).  Here the batch is n = 41 -- the smallest one above the
re-cut, and 41 = 5 x 8 + 1 leaves one image behind the XCD groups of 8 -- at the shapes whose plans tests/test_conv_tiles_cpu.py
pins:

  H x 21, H in {1, 3, 4, 6, 7, 9, 10, 12}   one block of NI = 1 .. 8 tiles, the last tile ragged
  21 x 21                                   two blocks of 7 tiles (the body self-play runs)
  37 x 37, float32 frame                    NI = 5: seven blocks of 5 tiles, two of 4 (ntile < NI), the last tile 25 of 32 rows
  37 x 37, 16-bit frame                     NI = 8: one block of 8 tiles, five of 7 (the kernel's NI - 1 body)

The reference is torch.nn.functional.conv2d in float64 on the GPU, then scale / shift, shortcut and ReLU in float64; for the
reduced-precision entry points it is built from the same rounded operands (the recipes of test_f16_reduced_precision_layer_and_net,
test_f16_activation_tower_layer_and_net and test_bf16_conv_layer_and_net in tests/test_net_gpu.py, with their bounds).  One float64
convolution per (shape, operand rounding) is shared by the epilogue variants and never modified.  In every case the input and the
shortcut are followed by one image of NaN, the output by one image of NaN that must stay NaN, and the real outputs must be finite.

Frame independence (the last test): in hs_block every M tile has its own accumulator acc[i], and an output's chain is
chunk 0 .. 7 -> tap 0 .. 8 -> (hi hi, hi lo, lo hi) MFMAs whatever NI is (HS_TAP: `acc[i]` takes tile i's products of tap s and
nothing else; NI only interleaves the tiles' instructions); staging, the LDS pixel and the epilogue's per-row arithmetic do not
depend on the block's tile range either.  So an image convolved alone (n = 1: one-tile blocks) must give the bits of its slice of
the batched launch, and the assertion is kept."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

N = 41
SWEEP = [(1, 21), (3, 21), (4, 21), (6, 21), (7, 21), (9, 21), (10, 21), (12, 21)]      # NI = 1 .. 8
BOARDS = [(21, 21), (37, 37)]
SHAPES = SWEEP + BOARDS
XS = 256.0                                # activation scale of the float32-tensor forms: |x| up to ~6, 6 * 256 << 65504
S1, B1 = 0.7, 0.05                        # the head's 1x1 stage: batch-norm scale / shift (one channel)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    from snake_engine._lib import lib, check
    return torch, lib(), check


def _st():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _conv64(torch, x, w):
    """float64 'same' 3 x 3 convolution of channels-last x [n, H, W, 128] with an HWIO kernel"""
    return torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1).contiguous()


_DATA = {}


def _guarded(torch, t):
    """t followed by one image of NaN"""
    return torch.cat([t, torch.full_like(t[:1], float("nan"))]).contiguous()


def _data(env, H, W):
    """inputs of a shape -- made once, read-only afterwards: float32 / f16 / bf16 input and shortcut (each followed by an image of
    NaN), kernel, scale, shift, the weight images, the head's 1x1 kernel"""
    torch, L, check = env
    if (H, W) in _DATA:
        return _DATA[H, W]
    from snake_engine.net import F16S_WEIGHT_BYTES
    g = torch.Generator(device="cuda").manual_seed(1000 * H + W)
    x = torch.randn(N, H, W, 128, device="cuda", generator=g)
    r = torch.randn(N, H, W, 128, device="cuda", generator=g)
    w = (torch.randn(3, 3, 128, 128, device="cuda", generator=g) * 0.05).contiguous()
    sc = torch.rand(128, device="cuda", generator=g) + 0.5
    sh = torch.randn(128, device="cuda", generator=g) * 0.1
    w1 = torch.randn(128, device="cuda", generator=g) * 0.1
    d = dict(w=w, sc=sc, sh=sh, w1=w1, conv={})
    for name, dt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
        d["x_" + name], d["r_" + name] = _guarded(torch, x.to(dt)), _guarded(torch, r.to(dt))
    ws = 2.0 ** (8 - int(torch.floor(torch.log2(w.abs().max())).item()))      # the kernel's weight scale: max|w| -> [256, 512)
    d["w_f16"] = (w * ws).to(torch.float16).double() / ws
    d["w_bf16"] = w.to(torch.bfloat16).double()
    for name, prep in (("f16s", lambda a, b: L.snk_conv3x3_prepare_weights_f16s(a, b, C.c_float(XS), _st())),
                       ("f16a", lambda a, b: L.snk_conv3x3_prepare_weights_f16_act16(a, b, _st())),
                       ("bf16", lambda a, b: L.snk_conv3x3_prepare_weights_bf16(a, b, _st()))):
        d["wS_" + name] = torch.empty(F16S_WEIGHT_BYTES, dtype=torch.uint8, device="cuda")
        check(prep(w.data_ptr(), d["wS_" + name].data_ptr()))
    _DATA[H, W] = d
    return d


def _conv_of(env, H, W, kind):
    """the float64 convolution (no scale / shift) of the operands as entry point `kind` rounds them -- once per (shape, kind)"""
    torch = env[0]
    d = _data(env, H, W)
    if kind not in d["conv"]:
        if kind == "f16s":                # float32-accurate: the operands as they are
            xv, wv = d["x_f32"][:N].double(), d["w"].double()
        elif kind == "f16":               # single pass, float32 tensors: f16(x * 256) / 256, f16(w * ws) / ws
            xv, wv = (d["x_f32"][:N] * XS).to(torch.float16).double() / XS, d["w_f16"]
        elif kind == "f16a":              # f16 activations in HBM (exact), f16(w * ws) / ws
            xv, wv = d["x_f16"][:N].double(), d["w_f16"]
        else:                             # bf16 activations in HBM (exact), bf16(w)
            xv, wv = d["x_bf16"][:N].double(), d["w_bf16"]
        d["conv"][kind] = _conv64(torch, xv, wv)
    return d["conv"][kind]


def _ref(env, H, W, kind, relu, res):
    """float64 layer output: conv * scale + shift (+ shortcut, as the entry point reads it) (ReLU)"""
    d = _data(env, H, W)
    ref = _conv_of(env, H, W, kind) * d["sc"].double() + d["sh"].double()
    if res:
        ref = ref + d[{"f16s": "r_f32", "f16": "r_f32", "f16a": "r_f16", "bf16": "r_bf16"}[kind]][:N].double()
    return ref.clamp_min(0) if relu else ref


def _out(torch, H, W, dtype=None):
    return torch.full((N + 1, H, W, 128), float("nan"), dtype=dtype or torch.float32, device="cuda")


def _guards(torch, out):
    assert torch.isnan(out[N]).all(), "something was written behind the last image"
    assert torch.isfinite(out[:N]).all()


def _p(t):
    return None if t is None else t.data_ptr()


# ---- snk_conv3x3_bn_f16s: the float32-accurate layer, MODE 1 / 2 / 0 / 0 --------------------------------------------------------

@pytest.mark.parametrize("relu,res", [(1, 0), (1, 1), (0, 1), (0, 0)])
@pytest.mark.parametrize("H,W", SHAPES)
def test_f16s_layer_in_the_batched_frame(env, H, W, relu, res):
    """bound: that of test_f16s_rectangular_and_edge_shapes -- an output's accumulation chain does not depend on the tile count"""
    torch, L, check = env
    d = _data(env, H, W)
    ref = _ref(env, H, W, "f16s", relu, res)
    out = _out(torch, H, W)
    check(L.snk_conv3x3_bn_f16s(_p(d["x_f32"]), _p(d["wS_f16s"]), _p(d["sc"]), _p(d["sh"]), _p(d["r_f32"]) if res else None,
                                _p(out), N, H, W, relu, _st()))
    _guards(torch, out)
    err, scale = (out[:N].double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"f16s {H}x{W} relu={relu} res={res}: err {err:.3g} scale {scale:.3g}")
    assert err <= 5e-6 * max(1.0, scale), (err, scale)


# ---- snk_conv3x3_bn_f16s_head: MODE 3 (no layer output) and the generic epilogue with the head (output kept) -----------------------

@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("hw", [21, 37])
def test_f16s_fused_head_in_the_batched_frame(env, hw, keep):
    """h1 against float64 END TO END (the float64 layer output, not the kernel's), bound of test_f16s_fused_head_equals_layer_plus_head"""
    torch, L, check = env
    d = _data(env, hw, hw)
    h1_ref = ((_ref(env, hw, hw, "f16s", 1, 1).reshape(N, hw * hw, 128) @ d["w1"].double()) * S1 + B1).clamp_min(0)
    h1 = torch.full((N + 1, hw * hw), float("nan"), device="cuda")
    act = _out(torch, hw, hw) if keep else None
    check(L.snk_conv3x3_bn_f16s_head(_p(d["x_f32"]), _p(d["wS_f16s"]), _p(d["sc"]), _p(d["sh"]), _p(d["r_f32"]), _p(act), _p(d["w1"]),
                                     C.c_float(S1), C.c_float(B1), _p(h1), N, hw, hw, _st()))
    _guards(torch, h1)
    if keep:
        plain = _out(torch, hw, hw)
        check(L.snk_conv3x3_bn_f16s(_p(d["x_f32"]), _p(d["wS_f16s"]), _p(d["sc"]), _p(d["sh"]), _p(d["r_f32"]), _p(plain), N, hw, hw, 1, _st()))
        _guards(torch, act)
        assert torch.equal(act[:N], plain[:N]), "the kept layer output differs from the plain MODE 2 launch"
    err, scale = (h1[:N].double() - h1_ref).abs().max().item(), h1_ref.abs().max().item()
    print(f"f16s head {hw}x{hw} keep={keep}: err {err:.3g} scale {scale:.3g}")
    assert err <= 2e-6 * max(1.0, scale), (err, scale)


# ---- snk_conv3x3_bn_f16: single pass, float32 tensors (the generic epilogue of k_conv3x3_f16s<NI, 0, false>) ----------------------

@pytest.mark.parametrize("H,W,relu,res", [(h, w, 1, 1) for h, w in SHAPES] + [(h, w, 0, 0) for h, w in BOARDS])
def test_f16_single_pass_layer_in_the_batched_frame(env, H, W, relu, res):
    torch, L, check = env
    d = _data(env, H, W)
    ref = _ref(env, H, W, "f16", relu, res)
    out = _out(torch, H, W)
    check(L.snk_conv3x3_bn_f16(_p(d["x_f32"]), _p(d["wS_f16s"]), _p(d["sc"]), _p(d["sh"]), _p(d["r_f32"]) if res else None,
                               _p(out), N, H, W, relu, _st()))
    _guards(torch, out)
    err, scale = (out[:N].double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"f16 {H}x{W} relu={relu} res={res}: err {err:.3g} scale {scale:.3g}")
    assert err <= 2e-5 * scale, (err, scale)


# ---- snk_conv3x3_bn_f16_act16 / snk_conv3x3_bn_bf16_act16: 16-bit activations in HBM --------------------------------------------

_ACT16 = ([(h, w, 0, 1, 1) for h, w in SWEEP] +
          [(h, w, o16, relu, res) for h, w in BOARDS for o16 in (0, 1) for relu, res in ((1, 1), (0, 0))])


@pytest.mark.parametrize("H,W,out16,relu,res", _ACT16)
@pytest.mark.parametrize("kind", ["f16a", "bf16"])
def test_act16_layer_in_the_batched_frame(env, kind, H, W, out16, relu, res):
    """bounds of test_bf16_conv_layer_and_net / test_f16_activation_tower_layer_and_net: float32 output to float32 rounding; a
    16-bit output is that result rounded once -- within one ulp (2^-7 bf16, 2^-10 f16) of the rounded reference, > 99 % bit-equal"""
    torch, L, check = env
    d = _data(env, H, W)
    t16, ulp, name = (torch.float16, 2.0 ** -10, "f16") if kind == "f16a" else (torch.bfloat16, 2.0 ** -7, "bf16")
    fn = L.snk_conv3x3_bn_f16_act16 if kind == "f16a" else L.snk_conv3x3_bn_bf16_act16
    ref = _ref(env, H, W, kind, relu, res)
    scale = ref.abs().max().item()
    out = _out(torch, H, W, t16 if out16 else None)
    check(fn(_p(d["x_" + name]), _p(d["wS_" + kind]), _p(d["sc"]), _p(d["sh"]), _p(d["r_" + name]) if res else None, _p(out), out16,
             N, H, W, relu, _st()))
    _guards(torch, out)
    if not out16:
        err = (out[:N].double() - ref).abs().max().item()
        print(f"{kind} {H}x{W} f32 out relu={relu} res={res}: err {err:.3g} scale {scale:.3g}")
        assert err <= 2e-5 * scale, (err, scale)
        return
    want = ref.to(t16)
    err = (out[:N].double() - want.double()).abs()
    same = (out[:N] == want).float().mean().item()
    over = (err - (ulp * want.double().abs() + 2e-5 * scale)).max().item()
    print(f"{kind} {H}x{W} 16-bit out relu={relu} res={res}: bit-equal {same:.5f}, worst excess over the bound {over:.3g}")
    assert over <= 0, over
    assert same > 0.99, same


# ---- snk_conv3x3_bn_f16_act16_head / snk_conv3x3_bn_bf16_act16_head: MODE 3 of the 16-bit frame -----------------------------------

@pytest.mark.parametrize("hw", [21, 37])
@pytest.mark.parametrize("kind", ["f16a", "bf16"])
def test_act16_fused_head_in_the_batched_frame(env, kind, hw):
    """The MODE 3 epilogue takes the head's dot product from the float32 values `v` after shortcut and ReLU (hs_block, `has_head`):
    the activation is NOT rounded to 16 bits before the 1x1 stage, so neither is the reference's.  No tolerance for this entry point
    exists in the project; the kernel must be no further from float64 than four times a float32 PyTorch evaluation of the same
    rounded operands (the pattern that closes test_tower_convolution_three_passes_match_float64).

    Measured on an MI355X, absolute errors (err_kernel, err_torch_f32), max|h1_ref| = 3.16 at 21 x 21 and 5.42 at 37 x 37:
      f16 activations   21 x 21 (8.54e-07, 2.54e-06)   37 x 37 (1.48e-06, 3.06e-06)
      bf16 activations  21 x 21 (7.32e-07, 9.76e-07)   37 x 37 (1.34e-06, 1.98e-06)"""
    torch, L, check = env
    d = _data(env, hw, hw)
    name = "f16" if kind == "f16a" else "bf16"
    fn = L.snk_conv3x3_bn_f16_act16_head if kind == "f16a" else L.snk_conv3x3_bn_bf16_act16_head
    h1_ref = ((_ref(env, hw, hw, kind, 1, 1).reshape(N, hw * hw, 128) @ d["w1"].double()) * S1 + B1).clamp_min(0)
    x32, r32, w32 = d["x_" + name][:N].float(), d["r_" + name][:N].float(), d["w_" + name].float()     # exact: 16-bit values in float32
    a32 = torch.nn.functional.conv2d(x32.permute(0, 3, 1, 2), w32.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    a32 = (a32 * d["sc"] + d["sh"] + r32).clamp_min(0)
    h1_32 = ((a32.reshape(N, hw * hw, 128) @ d["w1"]) * S1 + B1).clamp_min(0)
    h1 = torch.full((N + 1, hw * hw), float("nan"), device="cuda")
    check(fn(_p(d["x_" + name]), _p(d["wS_" + kind]), _p(d["sc"]), _p(d["sh"]), _p(d["r_" + name]), _p(d["w1"]), C.c_float(S1),
             C.c_float(B1), _p(h1), N, hw, hw, _st()))
    _guards(torch, h1)
    err_k = (h1[:N].double() - h1_ref).abs().max().item()
    err_t = (h1_32.double() - h1_ref).abs().max().item()
    scale = h1_ref.abs().max().item()
    print(f"{kind} head {hw}x{hw}: err_kernel {err_k:.3g} err_torch_f32 {err_t:.3g} scale {scale:.3g}")
    assert err_k <= 4 * err_t + 1e-7 * scale, f"err_kernel {err_k:.3g} err_torch_f32 {err_t:.3g} max|h1_ref| {scale:.3g}"


# ---- frame independence -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [21, 37])
def test_an_image_alone_gives_the_bits_of_its_slice_of_the_batch(env, hw):
    """f16s MODE 2: image i of the batch (7-tile / 5- and 4-tile blocks; i = 0, 7: ends of an XCD group, 8: the next group, 40: the
    ungrouped tail) against the same image launched with n = 1 (one-tile blocks) -- see the module docstring for why bits"""
    torch, L, check = env
    d = _data(env, hw, hw)
    out = _out(torch, hw, hw)
    check(L.snk_conv3x3_bn_f16s(_p(d["x_f32"]), _p(d["wS_f16s"]), _p(d["sc"]), _p(d["sh"]), _p(d["r_f32"]), _p(out), N, hw, hw, 1, _st()))
    _guards(torch, out)
    for i in (0, 7, 8, 40):
        xi, ri = d["x_f32"][i:i + 1].contiguous(), d["r_f32"][i:i + 1].contiguous()
        one = torch.full((2, hw, hw, 128), float("nan"), device="cuda")
        check(L.snk_conv3x3_bn_f16s(_p(xi), _p(d["wS_f16s"]), _p(d["sc"]), _p(d["sh"]), _p(ri), _p(one), 1, hw, hw, 1, _st()))
        assert torch.isnan(one[1]).all() and torch.isfinite(one[0]).all()
        assert torch.equal(one[0], out[i]), f"image {i}: {(one[0] != out[i]).sum().item()} values differ"
