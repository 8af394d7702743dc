"""The training head's entry points (csrc/train_net.hip: snk_head_conv1x1_sums, snk_head_dense_train_fwd,
snk_head_dense_train_bwd, snk_head_conv1x1_bwd and _bwd_stats) as plain NumPy float64 functions, written from the comments of
that file and sharing no code with it.  tests/test_train_head_ref_cpu.py holds these functions against float64 autograd of the
same graph; tests/test_train_head_gpu.py holds the kernels against these functions.

Every function returns a dict.  Next to each dot product `x` stands `S_x`: the float64 sum of the ABSOLUTE values of its terms
and addends, which is what a float32 evaluation's error is proportional to (bound() below).

A later stage can be given the value an earlier stage really produced (`z_in`, `d1_in`, `q_in`, `dpre1_in`, `g_in`, `da_in`):
the GPU test passes the kernel's own, already checked, intermediate there, so that each stage is held to the bound of ITS
dot product and no error of the stage before has to be allowed for.  Without them the functions are the whole chain.

Layouts as the kernels have them: a [rows][128] with rows = (state, pixel); z, h, g [n][HW]; W1 [HW][128]; W2 [128][3];
the ReLU bits of the last tower layer as one byte per quad of channels, bit k of byte q = channel 4 q + k (k_bn_apply).
"""
import numpy as np

C = 128                      # tower channels
STATES_PER_BLOCK = 16        # k_head_dense_train_fwd / _bwd
ROW_BLOCKS, ROWS_PER_SWEEP = 2048, 8     # tn_grid: min(2048, ceil(rows / 8)) blocks, 8 rows per block and sweep
LDS_LIMIT = 150 * 1024       # the forward's dynamic LDS: 16 (HW + 128) floats
U = 2.0 ** -24               # unit round-off of float32

# (n, H, W).  Every canvas once with n no multiple of 16 and once with n >= 17 (two blocks, the second short); n = 1 (the first
# half of k_head_dw1 runs over no state) on odd HW; (17, 37, 37) = 23 273 rows: more than one sweep of the 2048 x 8 row grid.
#   3x5: HW = 15, odd, one group of 8 then the scalar tail     1x5: only the scalar tail         4x6: 24, even, a multiple of 8
#   13x13: 169, odd, % 8 = 1, below 256                        21x13: 273, rectangular, just above 256
#   21x21: 441, the 11x11 board                                37x37: 1369, 95 KB of LDS, six pixel passes in the backward
CASES = [(1, 3, 5), (17, 3, 5), (2, 1, 5), (33, 1, 5), (15, 4, 6), (16, 4, 6), (17, 4, 6), (1, 13, 13), (33, 13, 13),
         (15, 21, 13), (17, 21, 13), (2, 21, 21), (33, 21, 21), (2, 37, 37), (17, 37, 37)]


def f64(x):
    return np.asarray(x, dtype=np.float64)


def bound(K, S):
    """|float32 evaluation - exact| of a K-term dot product in any order, with or without FMA, plus up to 8 further roundings"""
    return (K + 8) * U * f64(S)


def row_blocks(rows):
    return min(ROW_BLOCKS, max(1, (rows + ROWS_PER_SWEEP - 1) // ROWS_PER_SWEEP))


def row_block_of(rows):
    """block that handles each row of a row-strided kernel (k_head1x1, k_head_expand): row r belongs to block (r / 8) mod grid"""
    return (np.arange(rows) // ROWS_PER_SWEEP) % row_blocks(rows)


def rows_per_block(rows):
    return int(np.bincount(row_block_of(rows)).max())


def unpack_quad_bits(mask_bytes):
    """[rows][32] bytes -> [rows][128] bool: channel 4 q + k is bit k of byte q"""
    m = np.asarray(mask_bytes, dtype=np.uint8).reshape(-1, C // 4)
    return np.stack([(m >> k) & 1 for k in range(4)], axis=2).reshape(-1, C).astype(bool)


def pack_quad_bits(bits):
    b = np.asarray(bits, dtype=bool).reshape(-1, C // 4, 4).astype(np.uint8)
    return (b[:, :, 0] | (b[:, :, 1] << 1) | (b[:, :, 2] << 2) | (b[:, :, 3] << 3)).astype(np.uint8)


def conv1x1_sums(a, w1x1, center, z_in=None):
    """z[r] = sum_c a[r][c] w1x1[c]; sums = {sum (z - center), sum (z - center)^2}  (center None = 0)"""
    a, w = f64(a).reshape(-1, C), f64(w1x1).reshape(C)
    t = a * w
    z, S_z = t.sum(1), np.abs(t).sum(1)
    e = (z if z_in is None else f64(z_in).reshape(-1)) - (0.0 if center is None else float(center))
    return dict(z=z, S_z=S_z, sums=np.array([e.sum(), (e * e).sum()]), S_sums=np.array([np.abs(e).sum(), (e * e).sum()]),
                e=e)


def dense_fwd(z, scale, shift, W1, b1, W2, b2, target, err_scale=1.0, d1_in=None, q_in=None):
    """h = relu(z scale + shift) [n][HW]; d1 = relu(h W1 + b1) [n][128]; q = tanh(d1 W2 + b2) [n][3];
    sq_err = err_scale sum (q - target)^2.  pre_h, pre1, arg: the three pre-activations"""
    z, W1, b1, W2, b2 = f64(z), f64(W1), f64(b1), f64(W2), f64(b2)
    scale, shift = float(scale), float(shift)
    pre_h = z * scale + shift
    S_h = np.abs(z * scale) + abs(shift)
    h = np.maximum(pre_h, 0.0)
    # a float32 h can be non-zero where pre_h is above minus its bound; there its error is proportional to S_h, not to h
    live = pre_h > -bound(1, S_h)
    pre1 = h @ W1 + b1
    S_pre1 = np.where(live, S_h, 0.0) @ np.abs(W1) + np.abs(b1)
    d1 = np.maximum(pre1, 0.0)
    d1u = d1 if d1_in is None else f64(d1_in)
    arg = d1u @ W2 + b2
    S_arg = np.abs(d1u) @ np.abs(W2) + np.abs(b2)
    q = np.tanh(arg)
    out = dict(pre_h=pre_h, S_h=S_h, h=h, pre1=pre1, S_pre1=S_pre1, d1=d1, arg=arg, S_arg=S_arg, q=q)
    if target is not None:
        e = ((q if q_in is None else f64(q_in)) - f64(target)) ** 2
        out["sq_err"] = e.sum() * err_scale
        out["S_sq_err"] = e.sum() * abs(err_scale)
    return out


def dense_bwd(q, target, d1, h, h_mask, d1_mask, z, mean, inv, W1, W2, norm, dpre1_in=None, g_in=None):
    """dq = 2 (q - target) norm; dpre2 = dq (1 - q^2); dW2 = d1^T dpre2; db2 = sum_s dpre2;
    dpre1 = (dpre2 W2^T) where d1_mask > 0; db1 = sum_s dpre1; dW1 = h^T dpre1 [HW][128];
    g = (dpre1 W1^T) where h_mask > 0; gsums = {sum g, sum g zhat}, zhat = (z - mean) inv.
    h_mask / d1_mask None: the signs of h / d1.  small = dW2 [128][3], db2 [3], db1 [128] in one row of 515"""
    q, target, d1, h, z, W1, W2 = f64(q), f64(target), f64(d1), f64(h), f64(z), f64(W1), f64(W2)
    h_mask = h if h_mask is None else f64(h_mask)
    d1_mask = d1 if d1_mask is None else f64(d1_mask)
    norm = float(norm)
    dp2 = 2.0 * (q - target) * norm * (1.0 - q * q)
    S_dp2 = 2.0 * np.abs(q - target) * abs(norm) * (1.0 + q * q)          # 1 - q^2 rounds relative to 1 + q^2
    dW2, S_dW2 = d1.T @ dp2, np.abs(d1).T @ S_dp2
    db2, S_db2 = dp2.sum(0), S_dp2.sum(0)
    on1 = d1_mask > 0.0
    dpre1 = np.where(on1, dp2 @ W2.T, 0.0)
    S_dpre1 = np.where(on1, S_dp2 @ np.abs(W2).T, 0.0)
    dp = dpre1 if dpre1_in is None else f64(dpre1_in)
    db1, S_db1 = dp.sum(0), np.abs(dp).sum(0)
    dW1, S_dW1 = h.T @ dp, np.abs(h).T @ np.abs(dp)
    onh = h_mask > 0.0
    g = np.where(onh, dp @ W1.T, 0.0)
    S_g = np.where(onh, np.abs(dp) @ np.abs(W1).T, 0.0)
    gg = g if g_in is None else f64(g_in)
    zhat = (z - float(mean)) * float(inv)
    return dict(dp2=dp2, S_dp2=S_dp2, dpre1=dpre1, S_dpre1=S_dpre1, g=g, S_g=S_g, dW1=dW1, S_dW1=S_dW1,
                small=np.concatenate([dW2.reshape(-1), db2, db1]), S_small=np.concatenate([S_dW2.reshape(-1), S_db2, S_db1]),
                gsums=np.array([gg.sum(), (gg * zhat).sum()]), S_gsums=np.array([np.abs(gg).sum(), np.abs(gg * zhat).sum()]),
                g_terms=np.stack([gg, gg * zhat]))


def conv1x1_bwd(g, z, mean, inv, abc, a_last, w1x1, y_last=None, mask_last=None, mean_last=None, inv_last=None, da_in=None):
    """dz[r] = A (g[r] - B - zhat[r] C), abc = (A, B, C); da[r][c] = dz[r] w1x1[c]; dw1x1[c] = sum_r a_last[r][c] dz[r];
    with the last layer's y, mask bytes, mean and 1/sigma: sums [2][128] = {sum g', sum g' (y - mean) inv}, g' = da where the bit is set"""
    g, z, a_last, w = f64(g).reshape(-1), f64(z).reshape(-1), f64(a_last).reshape(-1, C), f64(w1x1).reshape(C)
    A, B, Cc = (float(v) for v in abc)
    zhat = (z - float(mean)) * float(inv)
    dz = A * (g - B - zhat * Cc)
    S_dz = abs(A) * (np.abs(g) + abs(B) + np.abs(zhat * Cc))
    da, S_da = dz[:, None] * w, S_dz[:, None] * np.abs(w)
    dw_terms, S_dw_terms = a_last * dz[:, None], np.abs(a_last) * S_dz[:, None]
    out = dict(dz=dz, S_dz=S_dz, da=da, S_da=S_da, dw1x1=dw_terms.sum(0), S_dw1x1=S_dw_terms.sum(0), S_dw_terms=S_dw_terms)
    if mask_last is not None:
        gp = np.where(unpack_quad_bits(mask_last), da if da_in is None else f64(da_in).reshape(-1, C), 0.0)
        xhat = (f64(y_last).reshape(-1, C) - f64(mean_last)) * f64(inv_last)
        out["stat_terms"] = np.stack([gp, gp * xhat])                        # [2][rows][128]
        out["sums"] = out["stat_terms"].sum(1)
        out["S_sums"] = np.abs(out["stat_terms"]).sum(1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# operands.  "int": every product and every partial sum is an exact float32 (test_train_head_ref_cpu.py proves the 2^24
# headroom case by case), so a float32 evaluation in ANY order equals the float64 one.  "float": O(1) pre-activations.
# ---------------------------------------------------------------------------------------------------------------------
def _ints(rs, lo, hi, shape):
    return rs.randint(lo, hi + 1, size=shape).astype(np.float64)


def operands(case, kind):
    """one dict of float64 / uint8 arrays per (case, kind), the same on every call"""
    n, H, W = case
    HW, rows = H * W, n * H * W
    rs = np.random.RandomState(1000 * n + 10 * HW + (kind == "int"))
    o = {}
    if kind == "int":
        o["a"] = _ints(rs, 0, 3, (rows, C))
        o["w1x1"] = _ints(rs, -1, 1, C)
        o["center"] = 3.0
        # forward: z in -3..2, scale 1, shift 1 -> h in 0..3; W1 in -1..1; W2 a power of two times -1..1 keeps tanh's argument O(1)
        o["z"] = _ints(rs, -3, 2, (n, HW))
        o["scale"], o["shift"] = 1.0, 1.0
        o["W1"], o["b1"] = _ints(rs, -1, 1, (HW, C)), _ints(rs, -2, 2, C)
        o["W2"], o["b2"] = _ints(rs, -1, 1, (C, 3)) / 64.0, _ints(rs, -1, 1, 3) / 4.0
        o["target"] = _ints(rs, -1, 1, (n, 3))
        o["err_scale"] = 0.25
        # backward: q a multiple of 1/4 (it is an input there), W2 whole numbers
        o["q"] = _ints(rs, -3, 3, (n, 3)) / 4.0
        o["h"], o["d1"] = np.maximum(_ints(rs, -3, 3, (n, HW)), 0.0), np.maximum(_ints(rs, -3, 3, (n, C)), 0.0)
        o["h_mask"], o["d1_mask"] = _ints(rs, -1, 1, (n, HW)), _ints(rs, -1, 1, (n, C))
        o["W2b"] = _ints(rs, -1, 1, (C, 3))
        o["mean"], o["inv"], o["norm"] = 1.0, 0.5, 2.0 ** -7
        # expansion: dz = 2 (g - 1 - (z - 1) / 2 * 2): even whole numbers
        o["g"] = _ints(rs, -3, 3, rows)
        o["zr"] = _ints(rs, -3, 3, rows)
        o["abc"] = np.array([2.0, 1.0, 2.0])
        o["y_last"] = _ints(rs, -3, 3, (rows, C))
        o["mean_last"], o["inv_last"] = _ints(rs, -1, 1, C), 2.0 ** _ints(rs, -1, 1, C)
    else:
        o["a"] = np.maximum(rs.randn(rows, C), 0.0)
        o["w1x1"] = rs.randn(C) * 0.1
        o["center"] = 0.37
        o["z"] = rs.randn(n, HW)
        o["scale"], o["shift"] = 1.3, 0.2
        o["W1"], o["b1"] = rs.randn(HW, C) / np.sqrt(HW), rs.randn(C) * 0.1
        o["W2"], o["b2"] = rs.randn(C, 3) * 0.15, rs.randn(3) * 0.1
        o["target"] = np.tanh(rs.randn(n, 3))
        o["err_scale"] = 1.0 / (3 * n)
        o["q"] = np.tanh(rs.randn(n, 3))
        o["h"], o["d1"] = np.maximum(rs.randn(n, HW), 0.0), np.maximum(rs.randn(n, C), 0.0)
        o["h_mask"], o["d1_mask"] = rs.randn(n, HW), rs.randn(n, C)
        o["W2b"] = o["W2"]
        o["mean"], o["inv"], o["norm"] = 0.1, 1.7, 1.0 / (3 * n)
        o["g"] = rs.randn(rows) * 1e-2
        o["zr"] = rs.randn(rows)
        o["abc"] = np.array([0.9, 0.01, 0.02])
        o["y_last"] = rs.randn(rows, C)
        o["mean_last"], o["inv_last"] = rs.randn(C) * 0.1, rs.rand(C) + 0.5
    o["a_last"] = o["a"]
    o["mask_last"] = rs.randint(0, 16, size=(rows, C // 4)).astype(np.uint8)
    # what the kernels will be given: float32 values (exactly representable for "int"), held here as float64
    for k, v in o.items():
        if isinstance(v, np.ndarray) and v.dtype == np.float64:
            o[k] = v.astype(np.float32).astype(np.float64)
        elif isinstance(v, float) and k not in ("norm", "err_scale"):        # (the two doubles of the C interface)
            o[k] = float(np.float32(v))
    return o


def state_block_of(n, per_state):
    """block of each element of an [n][per_state] tensor in the 16-states-per-block kernels"""
    return np.repeat(np.arange(n) // STATES_PER_BLOCK, per_state)


def _per_block(terms, block):
    """largest sum of |terms| over the elements of one block (terms [elements][...], block [elements])"""
    t = np.abs(f64(terms)).reshape(len(block), -1)
    acc = np.zeros((int(block.max()) + 1, t.shape[1]))
    np.add.at(acc, block, t)
    return float(acc.max())


def int_headroom(case):
    """{quantity: (largest sum of |terms| that one float32 accumulation of the kernels can meet, in units of the quantity's
    quantum; whether every reference value is a whole number of quanta)} for the "int" operands.  Below 2^24 every partial
    sum of whole numbers of quanta is an exact float32 whatever the order; the folds over blocks are float64."""
    n, H, W = case
    HW, rows = H * W, n * H * W
    o = operands(case, "int")
    out = {}

    def put(name, S_max, value, quantum):
        v = f64(value) / quantum
        out[name] = (float(S_max) / quantum, bool(np.all(v == np.round(v))))

    rb = row_block_of(rows)
    c = conv1x1_sums(o["a"], o["w1x1"], o["center"])
    put("z", c["S_z"].max(), c["z"], 1.0)
    put("sums", _per_block(np.stack([c["e"], c["e"] ** 2], axis=1), rb), c["sums"], 1.0)
    f = dense_fwd(o["z"], o["scale"], o["shift"], o["W1"], o["b1"], o["W2"], o["b2"], o["target"], o["err_scale"])
    put("h", f["S_h"].max(), f["h"], 1.0)
    put("d1", f["S_pre1"].max(), f["d1"], 1.0)
    qb = o["norm"] / 32.0                       # q - t: quarters, 1 - q^2: sixteenths, times 2
    b = dense_bwd(o["q"], o["target"], o["d1"], o["h"], o["h_mask"], o["d1_mask"], o["z"], o["mean"], o["inv"], o["W1"], o["W2b"],
                  o["norm"])
    put("dp2", b["S_dp2"].max(), b["dp2"], qb)
    put("dpre1", b["S_dpre1"].max(), b["dpre1"], qb)
    put("g", b["S_g"].max(), b["g"], qb)
    put("dW1", b["S_dW1"].max(), b["dW1"], qb)
    put("small", b["S_small"].max(), b["small"], qb)            # (over ALL states: more than any one block of 16 meets)
    put("gsums", _per_block(b["g_terms"].reshape(2, -1).T, state_block_of(n, HW)), b["gsums"], qb * o["inv"])
    e = conv1x1_bwd(o["g"], o["zr"], o["mean"], o["inv"], o["abc"], o["a_last"], o["w1x1"], o["y_last"], o["mask_last"],
                    o["mean_last"], o["inv_last"])
    put("da", e["S_da"].max(), e["da"], 1.0)
    put("dw1x1", _per_block(e["S_dw_terms"], rb), e["dw1x1"], 1.0)
    put("stat_sums", _per_block(e["stat_terms"].transpose(1, 0, 2), rb), e["sums"], 0.5)
    return out
