"""Every weight image the tower convolutions read, byte for byte against the NumPy model (tests/weight_image_ref.py): the ten
prepare kernels behind snk_conv3x3_prepare_weights{,_winograd,_f16s,_f16_act16,_bf16,_mxfp8,_f16s_train,_f16s_train_batch} and
snk_conv3x3_f16s_set_guard_word.  Every image is a buffer of SNK_CONV_F16S_WEIGHT_BYTES + 64 bytes pre-filled with 0xA5 (the
transpose and Winograd buffers: their size + 64) and the WHOLE buffer is compared: the model's bytes where a call writes, the
fill everywhere else -- the upper half of a 16-bit image, the gap of the MX-FP8 image, tail[2..3] in the batch form, the 64
bytes behind the tail.  Exact, signs of zero included; only a NaN's payload is free, an MX code zero may have either sign, and MX
blocks that hold a NaN or an infinity are outside the quantization rule.  No convolution runs here: a few prepare launches a test."""
import ctypes

import numpy as np
import pytest

import weight_image_ref as wi

pytestmark = pytest.mark.gpu

N = wi.IMAGE_BYTES + 64
SENTINEL = (5.0, 0.2)                         # tail[2..3] of the training forms: what the input's producer left there


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    from snake_engine import net
    from snake_engine._lib import lib, check, EngineError
    assert net.F16S_WEIGHT_BYTES == wi.IMAGE_BYTES and net.F16S_TAIL_OFFSET == wi.TAIL_OFFSET
    return torch, lib(), check, EngineError


def _st():
    import torch
    return torch.cuda.current_stream().cuda_stream


_DEV = {}


def _dev(name):
    """the case's kernel on the device (uploaded once)"""
    import torch
    if name not in _DEV:
        _DEV[name] = torch.as_tensor(np.array(wi.case(name))).cuda()
    return _DEV[name]


def _fresh(n=N, tail23=None):
    import torch
    b = torch.full((n,), wi.FILL, dtype=torch.uint8, device="cuda")
    if tail23 is not None:
        b[wi.TAIL_OFFSET + 8:wi.TAIL_OFFSET + 16].view(torch.float32).copy_(torch.tensor(tail23))
    return b


def _in_tail(scale, inv):
    import torch
    return torch.tensor([7.0, -3.0, scale, inv], device="cuda")


def _compare(what, kind, buf, want, **kw):
    got = buf.cpu().numpy()
    assert got.shape == want.shape
    ok = wi.same_image(kind, got, want, **kw)
    if not ok.all():
        bad = np.flatnonzero(~ok)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[:8].tolist()}: got {got[bad[:8]].tolist()}, "
                             f"want {want[bad[:8]].tolist()}")
    return got


_MODEL = {}


def _split_model(name, flip):
    """the model's split image with the training forms' tail (shared by the tests, never changed)"""
    if (name, flip) not in _MODEL:
        img = wi.split_image(wi.case(name), flip=flip, x_scale=SENTINEL[0], inv_x_scale=SENTINEL[1])
        img.setflags(write=False)
        _MODEL[name, flip] = img
    return _MODEL[name, flip]


_SINGLE = {}


def _single_entry(env, name, flip):
    """what snk_conv3x3_prepare_weights_f16s_train leaves for that case (IMAGE_BYTES bytes), with the sentinel as its input scale"""
    torch, L, check, _ = env
    if (name, flip) not in _SINGLE:
        buf = _fresh()
        check(L.snk_conv3x3_prepare_weights_f16s_train(_dev(name).data_ptr(), buf.data_ptr(), _in_tail(*SENTINEL).data_ptr(),
                                                       int(flip), None, _st()))
        got = buf.cpu().numpy()
        got.setflags(write=False)
        _SINGLE[name, flip] = got
    return _SINGLE[name, flip]


def _wino_report(got, want):
    g, w = got[:wi.WINO_BYTES].view(np.float32), want[:wi.WINO_BYTES].view(np.float32)
    fin = np.isfinite(g) & np.isfinite(w)
    key = lambda a: np.where(a.view(np.int32) < 0, np.int64(-2 ** 31) - a.view(np.int32).astype(np.int64), a.view(np.int32).astype(np.int64))
    d = np.abs(key(g[fin]) - key(w[fin]))
    return int(np.count_nonzero(d)), int(d.max(initial=0))


@pytest.mark.parametrize("name", wi.CASE_NAMES)
def test_single_layer_entries(env, name):
    torch, L, check, _ = env
    w, wd = wi.case(name), _dev(name)
    for xs in (256.0, 0.125):
        buf = _fresh()
        check(L.snk_conv3x3_prepare_weights_f16s(wd.data_ptr(), buf.data_ptr(), xs, _st()))
        _compare(f"f16s x_scale {xs}", "split", buf, wi.expected_buffer("split", N, wi.split_image(w, x_scale=xs)))
    for bf, fn in ((False, L.snk_conv3x3_prepare_weights_f16_act16), (True, L.snk_conv3x3_prepare_weights_bf16)):
        buf = _fresh()
        check(fn(wd.data_ptr(), buf.data_ptr(), _st()))
        _compare("bf16" if bf else "f16_act16", "a16", buf, wi.expected_buffer("a16", N, wi.a16_image(w, bf)), bf=bf)
    buf = _fresh()
    check(L.snk_conv3x3_prepare_weights_mxfp8(wd.data_ptr(), buf.data_ptr(), _st()))
    _compare("mxfp8", "mxfp8", buf, wi.expected_buffer("mxfp8", N, wi.mxfp8_image(w)), defined=wi.mx_defined_mask(w))
    buf = _fresh(wi.TRANSPOSE_BYTES + 64)
    check(L.snk_conv3x3_prepare_weights(wd.data_ptr(), buf.data_ptr(), _st()))
    _compare("transpose", "transpose", buf, wi.expected_buffer("transpose", wi.TRANSPOSE_BYTES + 64, wi.transpose_image(w)))
    # Winograd: bit equality -- G's entries are 0, 1 and +-1/2, so every product is exact and the model adds them in the
    # kernel's order; on a failure the count and the largest distance in float32 ulps are reported (more than 1 cannot be two
    # float64 summation orders rounded once)
    buf = _fresh(wi.WINO_BYTES + 64)
    check(L.snk_conv3x3_prepare_weights_winograd(wd.data_ptr(), buf.data_ptr(), _st()))
    want = wi.expected_buffer("wino", wi.WINO_BYTES + 64, wi.wino_image(w))
    try:
        _compare("winograd", "wino", buf, want)
    except AssertionError as e:
        raise AssertionError(f"{e}; (entries that differ, largest ulp distance) = {_wino_report(buf.cpu().numpy(), want)}")
    # the training form: the input scale comes from d_in_tail on the device
    for flip in (False, True):
        got = _single_entry(env, name, flip)
        want = wi.expected_buffer("split", N, _split_model(name, flip))
        ok = wi.same_image("split", got, want)
        assert ok.all(), (flip, np.flatnonzero(~ok)[:8], got[~ok][:8], want[~ok][:8])
    # ... with a donor image of the same kernel: the same bytes, tail[2..3] from d_in_tail (not from the donor)
    donor = _fresh()
    check(L.snk_conv3x3_prepare_weights_f16s_train(wd.data_ptr(), donor.data_ptr(), _in_tail(4.0, 0.25).data_ptr(), 0, None, _st()))
    for flip in (False, True):
        buf = _fresh()
        check(L.snk_conv3x3_prepare_weights_f16s_train(wd.data_ptr(), buf.data_ptr(), _in_tail(*SENTINEL).data_ptr(), int(flip),
                                                       donor.data_ptr(), _st()))
        _compare(f"train with donor, flip {flip}", "split", buf, wi.expected_buffer("split", N, _split_model(name, flip)))
    # ... and with a donor made from another kernel: the image carries the donor's scale
    other = "pow2_5" if name != "pow2_5" else "glorot"
    k_other = wi.weight_scale_k(wi.case(other))
    check(L.snk_conv3x3_prepare_weights_f16s_train(_dev(other).data_ptr(), donor.data_ptr(), _in_tail(4.0, 0.25).data_ptr(), 0, None, _st()))
    buf = _fresh()
    check(L.snk_conv3x3_prepare_weights_f16s_train(wd.data_ptr(), buf.data_ptr(), _in_tail(*SENTINEL).data_ptr(), 1, donor.data_ptr(), _st()))
    want = wi.split_image(w, flip=True, x_scale=SENTINEL[0], inv_x_scale=SENTINEL[1], k=k_other)
    _compare("train with another kernel's donor", "split", buf, wi.expected_buffer("split", N, want))


def _ptrs(items):
    return (ctypes.c_void_p * len(items))(*[None if t is None else t.data_ptr() for t in items])


@pytest.mark.parametrize("bwd", ["none", "all", "first_and_middle_null"])
@pytest.mark.parametrize("n_layers", [1, 3, 40])
def test_batch_entry(env, n_layers, bwd):
    """snk_conv3x3_prepare_weights_f16s_train_batch (k_f16s_wscale_batch, k_f16s_weights_batch), the path an optimizer step
    takes: every image equals the one-layer entry's and the model's, tail[2..3] keep what was there, tail[4..7] are zero.
    first_and_middle_null: the pattern of snake_engine/train_step.py (no input gradient below the first layer)."""
    torch, L, check, _ = env
    off = {1: 15, 3: 13, 40: 0}[n_layers]     # 1: big_2^117; 3: tiny_2^-110, big_2^110, big_2^117; 40: the whole table twice
    names = [wi.CASE_NAMES[(off + i) % len(wi.CASE_NAMES)] for i in range(n_layers)]
    fwd = [_fresh(tail23=SENTINEL) for _ in names]
    if bwd == "none":
        back = [None] * n_layers
    else:
        null = {0, n_layers // 2} if bwd == "first_and_middle_null" else set()
        back = [None if i in null else _fresh(tail23=SENTINEL) for i in range(n_layers)]
    before = _fresh(tail23=SENTINEL).cpu().numpy()
    check(L.snk_conv3x3_prepare_weights_f16s_train_batch(_ptrs([_dev(n) for n in names]), _ptrs(fwd),
                                                         None if bwd == "none" else _ptrs(back), n_layers, _st()))
    for i, name in enumerate(names):
        for flip, buf in ((False, fwd[i]), (True, back[i])):
            if buf is None:
                continue
            want = wi.expected_buffer("batch", N, _split_model(name, flip), before=before)
            got = _compare(f"layer {i} ({name}), flip {flip}", "batch", buf, want)
            tail = got[wi.TAIL_OFFSET:wi.IMAGE_BYTES].view(np.float32)
            assert tuple(tail[2:4]) == tuple(np.float32(SENTINEL)) and not got[wi.TAIL_OFFSET + 16:wi.IMAGE_BYTES].any()
            single = _single_entry(env, name, flip)                 # the sentinel is its input scale: all of it must agree
            assert wi.same_image("split", got, single).all(), (i, name, flip)


def test_refusals(env):
    torch, L, check, EngineError = env
    names = wi.CASE_NAMES[:3]
    w, f = [_dev(n) for n in names], [_fresh() for _ in names]
    for n in (0, 41, -1):
        with pytest.raises(EngineError, match=r"train_batch: 1 \.\. 40 layers per call"):
            check(L.snk_conv3x3_prepare_weights_f16s_train_batch(_ptrs(w * 14), _ptrs(f * 14), None, n, _st()))
    with pytest.raises(EngineError, match=r"train_batch: NULL kernel or image \(layer 1\)"):
        check(L.snk_conv3x3_prepare_weights_f16s_train_batch(_ptrs([w[0], None, w[2]]), _ptrs(f), None, 3, _st()))
    with pytest.raises(EngineError, match=r"train_batch: NULL kernel or image \(layer 1\)"):
        check(L.snk_conv3x3_prepare_weights_f16s_train_batch(_ptrs(w), _ptrs([f[0], None, f[2]]), _ptrs(f), 3, _st()))
    with pytest.raises(EngineError, match="train_batch"):
        check(L.snk_conv3x3_prepare_weights_f16s_train_batch(None, _ptrs(f), None, 3, _st()))
    for xs in (3.0, 0.3, 0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(EngineError, match="prepare_weights_f16s: x_scale .* is not a power of two"):
            check(L.snk_conv3x3_prepare_weights_f16s(w[0].data_ptr(), f[0].data_ptr(), xs, _st()))
    with pytest.raises(EngineError, match="prepare_weights_f16s_train: bad argument"):
        check(L.snk_conv3x3_prepare_weights_f16s_train(w[0].data_ptr(), f[0].data_ptr(), _in_tail(1.0, 1.0).data_ptr(), 0, f[0].data_ptr(), _st()))
    with pytest.raises(EngineError, match="prepare_weights_f16s_train: bad argument"):
        check(L.snk_conv3x3_prepare_weights_f16s_train(w[0].data_ptr(), f[0].data_ptr(), None, 0, None, _st()))
    torch.cuda.synchronize()
    for b in f:                                # a refused call launches nothing
        assert bool((b == wi.FILL).all())


@pytest.mark.parametrize("entry", ["f16s", "mxfp8"])
def test_guard_word(env, entry):
    torch, L, check, _ = env
    w = _dev("glorot")

    def prepare(buf):
        if entry == "f16s":
            check(L.snk_conv3x3_prepare_weights_f16s(w.data_ptr(), buf.data_ptr(), 2.0, _st()))
        else:
            check(L.snk_conv3x3_prepare_weights_mxfp8(w.data_ptr(), buf.data_ptr(), _st()))
    buf = _fresh()
    prepare(buf)
    before = buf.cpu().numpy()
    assert not before[wi.TAIL_OFFSET + 16:wi.IMAGE_BYTES].any()
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    check(L.snk_conv3x3_f16s_set_guard_word(buf.data_ptr(), word.data_ptr(), _st()))
    addr = np.frombuffer(int(word.data_ptr()).to_bytes(8, "little"), np.uint8)
    _compare("guard word set", "guard", buf, wi.expected_buffer("guard", N, np.concatenate([np.zeros(wi.TAIL_OFFSET + 24, np.uint8), addr]),
                                                                 before=before))
    check(L.snk_conv3x3_f16s_set_guard_word(buf.data_ptr(), None, _st()))          # NULL unregisters
    _compare("guard word unset", "guard", buf, before)
    check(L.snk_conv3x3_f16s_set_guard_word(buf.data_ptr(), word.data_ptr(), _st()))
    prepare(buf)                                                                    # a later prepare call clears it
    _compare("prepare after the guard word", "guard", buf, before)
    assert int(word.item()) == 0


def _f16s_and_batch(env, name):
    """(tail float32[8], body f16) of the case from the one-layer entry and from the batch entry"""
    torch, L, check, _ = env
    out = []
    a, b = _fresh(), _fresh(tail23=SENTINEL)
    check(L.snk_conv3x3_prepare_weights_f16s(_dev(name).data_ptr(), a.data_ptr(), 1.0, _st()))
    check(L.snk_conv3x3_prepare_weights_f16s_train_batch(_ptrs([_dev(name)]), _ptrs([b]), None, 1, _st()))
    for buf in (a, b):
        g = buf.cpu().numpy()
        out.append((g[wi.TAIL_OFFSET:wi.IMAGE_BYTES].view(np.float32), g[:wi.TAIL_OFFSET].view(np.float16)))
    return out


def test_non_finite_entries_and_extreme_maxima(env):
    """NaN entries do not move k and come out as f16 NaN (hi and lo); an infinite entry gives k = 0; maxima of 2^-140 and 2^-110
    give k = 100 and a finite image; f16-subnormal hi and lo parts are kept, not flushed (the model keeps them: v_cvt_f16_f32
    follows the wave's f16 denormal mode, which the compiler leaves on, and the float32 subtraction before it is exact)"""
    w = np.array(wi.case("nan"))
    nan = np.isnan(w)
    k = wi.weight_scale_k(np.where(nan, np.float32(0), w))
    for tail, body in _f16s_and_batch(env, "nan"):
        assert tail[0] == 2.0 ** -k and tail[1] == 2.0 ** k
        assert np.count_nonzero(np.isnan(body)) == 2 * np.count_nonzero(nan) and not np.isinf(body).any()
    for tail, body in _f16s_and_batch(env, "inf"):
        assert tail[0] == 1.0 and tail[1] == 1.0
        assert np.count_nonzero(~np.isfinite(body)) == 2                 # hi = inf, lo = inf - inf
    for name in ("sub_2^-140", "tiny_2^-110"):
        for tail, body in _f16s_and_batch(env, name):
            assert tail[1] == 2.0 ** 100 and tail[0] == 2.0 ** -100 and np.isfinite(body).all()
    hi, lo, _ = wi.split_parts(wi.case("ties"))
    sub = lambda a: int(np.count_nonzero((a != 0) & (np.abs(a.astype(np.float64)) < 2.0 ** -14)))
    want = sub(hi) + sub(lo)
    assert sub(hi) >= 1000 and sub(lo) >= 1000
    for tail, body in _f16s_and_batch(env, "ties"):
        print(f"f16-subnormal parts of `ties`: device {sub(body)}, model {want}")
        assert sub(body) == want


def test_scale_clamp_leaves_large_kernels_finite(env):
    """the lower clamp of k, in k_f16s_wscale and k_f16s_wscale_batch: at max |w| = 2^110 and 2^117 the image is finite and
    256 <= max 2^k < 512.  With the clamp at -100 that it replaces, 2^110 gave max 2^k = 1024 and 2^117 gave 2^17: f16
    infinities for the largest weights."""
    for name, m in (("big_2^110", 2.0 ** 110), ("big_2^117", 2.0 ** 117)):
        for tail, body in _f16s_and_batch(env, name):
            assert np.isfinite(body).all(), (name, int(np.count_nonzero(~np.isfinite(body))))
            assert 256 <= m * float(tail[1]) < 512 and float(tail[0]) * float(tail[1]) == 1.0 and np.isfinite(tail[:2]).all()
            assert float(np.abs(body.astype(np.float64)).max()) == m * float(tail[1])
