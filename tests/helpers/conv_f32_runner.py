"""The child process of tests/test_conv_f32_forms_gpu.py: the two float32 forms of the 3x3 tower layer (csrc/net.hip) in every launch
form against the float64 model tests/conv_f32_ref.py.  SNK_CONV_BK and SNK_WINO_WAVES are read once per process, so each
configuration is one run of this program, `conv_f32_runner.py default | bk32_nw4`, the environment set by the caller:

    default     snk_conv3x3_bn_f32 launches k_conv3x3_f32<16, 3>, snk_conv3x3_bn_f32_winograd launches k_conv3x3_wino_f32<8>
    bk32_nw4    SNK_CONV_BK=32 and SNK_WINO_WAVES=4: k_conv3x3_f32<32, 2> and k_conv3x3_wino_f32<4>

Every output buffer holds NaN before the launch and has one image of slack behind it that must still be all NaN afterwards.  For
both entries ("direct": snk_conv3x3_prepare_weights + snk_conv3x3_bn_f32, "winograd": the _winograd pair):

  random layer     every case of CASES with ReLU and residual, four of them in all four combinations:
                   max |out - ref| <= 2e-5 max |ref|   (tests/test_net_gpu.py::test_conv3x3_layer's bound for these kernels)
  no range limit   the same bound with the inputs scaled by 3e4 and by 1e-6, every output finite
  exact integers   every case of CASES on integer_inputs: the int32 bit patterns of the float64 model's values
  one-hot taps     w = one_hot_weights(tap), scale 1, shift 0, no residual, no ReLU, random x.  direct: the shifted input bit for bit,
                   +0 where the tap leaves the image.  winograd: |out - shifted x| <= 4e-7 max |x| per element -- its transforms add
                   and subtract neighbours, so it is not exact on random floats: four float32 roundings (half an ulp, 2^-23 max |x|
                   each) of values up to 4 max |x|
  padding          an image of NaN between two others leaves their outputs bit for bit what they are without it: what lies
                   outside an image is selected away, not multiplied by zero
  one image alone  gives the bits of its slice of the batch
  whole net        QNet under SNK_CONV_ALGO=winograd and =direct on the golden 11x11x4 states, batch norm randomised: |dQ| <= 1e-5
                   against oracle/net_ref.py in one chunk and in chunks of 53, the two bit for bit the same
  refusals         (default configuration) a NULL argument and out == x raise EngineError, n_images = 0 returns 0: buffer untouched
The batch limits (M < 2^31, n H W 128 < 2^32) are not approached: reaching them takes 16 GB, and a refusal probe of them over small
buffers would launch out of bounds if the guard ever regressed.

A line `fig <entry> <case> <figure> <bound>` is printed before each assertion, `max <entry> <group> ...` at the end, then
`digest <entry> <sha256 of the random (5, 21, 21) output>` and `conv f32 forms <config>: ok`.  Measured on an MI355X:

  default     max direct layer 1.788e-06     max direct range 1.586e-06     max direct net 1.781e-06
              max winograd layer 5.069e-07   max winograd range 5.199e-07   max winograd net 1.550e-06   max winograd onehot 1.760e-07
  bk32_nw4    max direct layer 1.385e-06     max direct range 1.580e-06     max direct net 1.699e-06
              max winograd layer 5.069e-07   max winograd range 5.199e-07   max winograd net 1.550e-06   max winograd onehot 1.760e-07
(layer, range: of max |ref|, bound 2e-05; net: |dQ|, bound 1e-05; onehot: of max |x|, bound 4e-07.)  The exact-integer, one-hot
direct, NaN-image and image-alone comparisons hold bit for bit in both configurations.  The Winograd figures, and its digest, are
the same in both: NW does not change the order of any sum.  The one-hot figure is also what a NumPy float32 restatement of the
transforms gives (tests/test_conv_f32_ref_cpu.py::winograd_f32), rounding for rounding."""
import hashlib
import os
import sys

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO = os.path.dirname(TESTS)
for _p in (TESTS, REPO, os.path.join(REPO, "alphasnake-zero_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np
import torch

import conv_f32_ref as R

NAN = float("nan")
C = R.C
ENTRIES = {"direct": ("snk_conv3x3_prepare_weights", "snk_conv3x3_bn_f32", 9 * C * C),
           "winograd": ("snk_conv3x3_prepare_weights_winograd", "snk_conv3x3_bn_f32_winograd", 16 * C * C)}
ALL_FOUR = [(3, 7, 9), (2, 8, 8), (1, 2, 66), (5, 21, 21)]      # run with and without ReLU, with and without residual
RANGE = [(3, 7, 9), (5, 21, 21)]
MAGS = (3e4, 1e-6)
ONE_HOT = [(3, 7, 9), (2, 4, 7)]
TOL_LAYER = 2e-5
TOL_ONE_HOT = 4e-7
TOL_Q = 1e-5
FIG = {}
DIGEST = {}


def seed_of(case):
    n, H, W = case
    return 1000 * H + W + n


def name_of(case):
    return "%dx%dx%d" % case


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def prepare(L, entry, w):
    from snake_engine._lib import check
    image = torch.empty(ENTRIES[entry][2], dtype=torch.float32, device="cuda")
    check(getattr(L, ENTRIES[entry][0])(w.data_ptr(), image.data_ptr(), st()))
    return image


def launch(L, entry, image, x, scale, shift, res, out, n, H, W, relu):
    """the raw call: raises EngineError with the library's message where it is refused"""
    from snake_engine._lib import check
    check(getattr(L, ENTRIES[entry][1])(x.data_ptr() if x is not None else None, image.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                        res.data_ptr() if res is not None else None, out.data_ptr(), n, H, W, int(relu), st()))
    torch.cuda.synchronize()


def conv(L, entry, image, x, scale, shift, res, relu):
    """device tensors in, the [n, H, W, 128] output out; asserts that the image of slack behind it still holds NaN"""
    n, H, W, _ = x.shape
    out = torch.full((n + 1, H, W, C), NAN, dtype=torch.float32, device="cuda")
    launch(L, entry, image, x, scale, shift, res, out, n, H, W, relu)
    assert bool(torch.isnan(out[n]).all()), (entry, (n, H, W), "the slack behind the output was written")
    return out[:n]


def hold(entry, group, label, fig, bound):
    print(f"fig {entry} {label} {fig:.3e} {bound:.0e}", flush=True)
    FIG[(entry, group)] = max(FIG.get((entry, group), 0.0), fig)
    assert fig <= bound, (entry, label, fig, bound)


def random_layer(L, case, combos, mag=1.0, group="layer"):
    x, w, scale, shift, res = R.inputs(case, seed_of(case), mag)
    d = [dev(t) for t in (x, w, scale, shift, res)]
    for relu, with_res in combos:
        ref = R.layer(x, w, scale, shift, res if with_res else None, relu)
        ref_max = float(np.abs(ref).max())
        for entry in ENTRIES:
            out = conv(L, entry, prepare(L, entry, d[1]), d[0], d[2], d[3], d[4] if with_res else None, relu)
            got = out.cpu().double().numpy()
            assert np.isfinite(got).all(), (entry, case, mag, "not finite")
            label = name_of(case) + f"/relu{int(relu)}res{int(with_res)}" + ("" if mag == 1.0 else f"/mag{mag:g}")
            hold(entry, group, label, float(np.abs(got - ref).max()) / ref_max, TOL_LAYER)
            if case == (5, 21, 21) and relu and with_res and mag == 1.0:
                DIGEST[entry] = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()


def same_bits(entry, label, got, want):
    """got: device float32; want: a NumPy float32 array of the same shape"""
    a = bits(got).cpu().numpy()
    b = np.ascontiguousarray(want, np.float32).view(np.int32)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        i = tuple(int(v) for v in bad[0])
        print(f"differ {entry} {label}: first at (image, y, x, channel) = {i}: got {got[i].item()!r}, expected {float(want[i])!r}; "
              f"{len(bad)} of {a.size} elements differ", flush=True)
        raise AssertionError((entry, label, "bit patterns differ", i, len(bad)))


def integer_layer(L, case):
    x, w, scale, shift, res = R.integer_inputs(case, seed_of(case))
    ref = R.layer(x, w, scale, shift, res, True)
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref)
    d = [dev(t) for t in (x, w, scale, shift, res)]
    for entry in ENTRIES:
        out = conv(L, entry, prepare(L, entry, d[1]), d[0], d[2], d[3], d[4], True)
        same_bits(entry, "integers " + name_of(case), out, ref32)


def one_hot(L, case):
    n, H, W = case
    x = R.inputs(case, seed_of(case) + 7)[0]
    x_max = float(np.abs(x).max())
    xd, one, zero = dev(x), dev(np.ones(C)), dev(np.zeros(C))
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        want = np.zeros_like(x)
        want[:, max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)] = x[:, max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)]
        wd = dev(R.one_hot_weights(tap))
        label = f"onehot {name_of(case)}/tap{tap}"
        out = conv(L, "direct", prepare(L, "direct", wd), xd, one, zero, None, False)
        same_bits("direct", label, out, want)
        out = conv(L, "winograd", prepare(L, "winograd", wd), xd, one, zero, None, False)
        got = out.cpu().double().numpy()
        assert np.isfinite(got).all()
        hold("winograd", "onehot", label.replace(" ", "/"), float(np.abs(got - want).max()) / x_max, TOL_ONE_HOT)


def nan_image(L):
    case = (3, 7, 9)
    x, w, scale, shift, res = R.inputs(case, seed_of(case))
    bad = x.copy()
    bad[1] = NAN
    d = [dev(t) for t in (x, w, scale, shift, res)]
    for entry in ENTRIES:
        image = prepare(L, entry, d[1])
        clean = conv(L, entry, image, d[0], d[2], d[3], d[4], True)
        got = conv(L, entry, image, dev(bad), d[2], d[3], d[4], True)
        assert bool(torch.isfinite(clean).all())
        for i in (0, 2):
            assert torch.equal(bits(got[i]), bits(clean[i])), (entry, "a NaN image changed image", i, int((bits(got[i]) != bits(clean[i])).sum()))


def image_alone(L, case):
    n = case[0]
    x, w, scale, shift, res = R.inputs(case, seed_of(case))
    d = [dev(t) for t in (x, w, scale, shift, res)]
    for entry in ENTRIES:
        image = prepare(L, entry, d[1])
        batch = conv(L, entry, image, d[0], d[2], d[3], d[4], True)
        for i in range(n):
            alone = conv(L, entry, image, d[0][i:i + 1], d[2], d[3], d[4][i:i + 1], True)
            assert torch.equal(bits(alone[0]), bits(batch[i])), (entry, case, "image alone differs from its slice", i)


def randomised_bn(ws, seed):
    """as tests/test_net_gpu.py::_randomised_bn: gamma, beta, mean, var of every batch norm redrawn"""
    rng = np.random.RandomState(seed)
    out = [w.copy() for w in ws]
    k = 0
    while k < len(out):
        if out[k].ndim == 4:
            n = out[k].shape[3]
            out[k + 1] = (1.0 + 0.2 * rng.randn(n)).astype(np.float32)
            out[k + 2] = (0.1 * rng.randn(n)).astype(np.float32)
            out[k + 3] = (0.05 * rng.randn(n)).astype(np.float32)
            out[k + 4] = (0.5 + rng.rand(n)).astype(np.float32)
            k += 5
        else:
            k += 1
    return out


def whole_net():
    from oracle import net_ref
    from snake_engine import net
    s = np.load(os.path.join(TESTS, "golden", "states_11x11x4.npz"), allow_pickle=False)
    states = s["raw"][:96]
    ws = randomised_bn(net.glorot_uniform_weights((21, 21, 3), blocks=4, seed=0), 3)
    ref = net_ref.forward(ws, states)
    planes = torch.as_tensor(states, device="cuda")
    mask = torch.as_tensor(s["mask"][s["raw_index"][:96]], device="cuda")
    for algo in ("winograd", "direct"):
        os.environ["SNK_CONV_ALGO"] = algo
        try:
            got = []
            for max_chunk in (4096, 53):                 # one chunk; 53 + 43
                qn = net.QNet(ws, (21, 21, 3), max_chunk=max_chunk)
                assert qn.conv_algo == algo
                q = qn.forward(planes, mask).cpu().numpy()
                assert np.isfinite(q).all()
                hold(algo, "net", f"net/chunk{max_chunk}", float(np.abs(q - ref).max()), TOL_Q)
                assert (q[ref == -1.0] == -1.0).all()
                got.append(q)
            assert np.array_equal(got[0].view(np.int32), got[1].view(np.int32)), (algo, "the two chunkings differ")
        finally:
            del os.environ["SNK_CONV_ALGO"]


def refusals(L):
    from snake_engine._lib import EngineError
    case = (2, 4, 7)
    n, H, W = case
    x, w, scale, shift, res = [dev(t) for t in R.inputs(case, 99)]
    for entry in ENTRIES:
        image = prepare(L, entry, w)
        out = torch.full((n + 1, H, W, C), NAN, dtype=torch.float32, device="cuda")
        for what, x_ in (("NULL x", None), ("out == x", out)):
            try:
                launch(L, entry, image, x_, scale, shift, res, out, n, H, W, True)
            except EngineError:
                assert bool(torch.isnan(out).all()), (entry, what, "refused, but the buffer was written")
            else:
                raise AssertionError((entry, what, "was not refused"))
        launch(L, entry, image, x, scale, shift, res, out, 0, H, W, True)        # n_images = 0: returns 0, launches nothing
        assert bool(torch.isnan(out).all()), (entry, "n_images = 0 wrote the buffer")


def main():
    config = sys.argv[1]
    want = R.CONFIGS[config]
    for k in R.ENV_NAMES:
        assert os.environ.get(k) == want.get(k), (k, os.environ.get(k))
    from snake_engine._lib import lib
    L = lib()
    every = [(True, True), (True, False), (False, True), (False, False)]
    for case in R.CASES:
        random_layer(L, case, every if case in ALL_FOUR else every[:1])
    for case in RANGE:
        for mag in MAGS:
            random_layer(L, case, every[:1], mag, "range")
    for case in R.CASES:
        integer_layer(L, case)
    for case in ONE_HOT:
        one_hot(L, case)
    nan_image(L)
    for case in RANGE:
        image_alone(L, case)
    whole_net()
    if config == "default":
        refusals(L)
    bound = {"layer": f"{TOL_LAYER:.0e} of max |ref|", "range": f"{TOL_LAYER:.0e} of max |ref|", "onehot": f"{TOL_ONE_HOT:.0e} of max |x|",
             "net": f"|dQ| {TOL_Q:.0e}"}
    for entry, group in sorted(FIG):
        print(f"max {entry} {group} {FIG[(entry, group)]:.3e} (bound {bound[group]})")
    for entry in ENTRIES:
        print(f"digest {entry} {DIGEST[entry]}")
    print(f"conv f32 forms {config}: ok")


if __name__ == "__main__":
    main()
