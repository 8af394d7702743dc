"""snk_engine_observe_mirror (run with -m gpu on an MI355X): the observe kernel's second output form, which writes flagged rows
flipped on the W axis -- numpy.flip(states, axis=2) of the trainer's augmentation (trainer.py:93-97) in the launch that encodes
the rows.  The expected bytes are the unmirrored launch's (snk_engine_observe_rows on the same index, itself pinned to the
reference's bytes by tests/test_engine_gpu.py) with the flagged rows flipped, so every comparison is bit for bit."""
import numpy as np
import pytest

from conftest import load_golden, golden_state

pytestmark = pytest.mark.gpu

# 5x5x2, 9x9x3: the generic <0,0> body; 7x7x2, 11x11x4: the compile-time bodies; 16x16x6: 256 cells, the first board whose rings
# have 16-bit entries; 19x19x8: the largest
CFGS = ["5x5x2", "9x9x3", "7x7x2", "11x11x4", "16x16x6", "19x19x8"]
N_STATES = 24


@pytest.fixture(scope="module")
def se():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import snake_engine
    return snake_engine


def _boards(se, cfg, n_states=N_STATES):
    """an engine holding n_states golden states spread over the trajectories + one state with a dead snake; the (slot, snake)
    pairs of every live snake of the former, then one pair naming the dead snake; the last_move of each live pair"""
    from snake_engine.engine import state_from_compact
    z = load_golden(f"tic_{cfg}.npz")
    s = load_golden(f"states_{cfg}.npz")
    H, W, S, hd = int(z["H"]), int(z["W"]), int(z["S"]), int(z["health_dec"])
    uniq = np.unique(s["state_index"])
    chosen = uniq[np.linspace(0, len(uniq) - 1, n_states).astype(int)]
    assert len(set(chosen.tolist())) == n_states >= 16
    slot_of = {int(v): k for k, v in enumerate(chosen)}
    keep = np.isin(s["state_index"], chosen)
    pairs = [[slot_of[int(si)], int(sn)] for si, sn in zip(s["state_index"][keep], s["snake_id"][keep])]
    dirs = [int(z["st_dir"][si][sn]) & 3 for si, sn in zip(s["state_index"][keep], s["snake_id"][keep])]
    assert set(dirs) == {0, 1, 2, 3}, "the chosen states carry all four rotations"
    for si in chosen:                                     # every live snake of the chosen states is observed
        assert int(z["st_alive"][si].sum()) == sum(1 for p in pairs if p[0] == slot_of[int(si)])
    dead_state = next(i for i in range(len(z["st_alive"])) if z["st_alive"][i].sum() < S)
    dead_snake = int(np.flatnonzero(z["st_alive"][dead_state] == 0)[0])
    eng = se.Engine(n_states + 1, H, W, S, hd, 0.15)
    eng.import_states([state_from_compact(H, W, S, golden_state(z, i)) for i in list(chosen) + [dead_state]])
    pairs.append([n_states, dead_snake])
    return eng, np.array(pairs, np.int32), np.array(dirs)


def _alloc(eng, m, layout):
    import torch
    from snake_engine.engine import NHWC_F32, NCHW_BF16
    shape = (m,) + (eng.obs_shape if layout == NHWC_F32 else (3,) + eng.obs_shape[:2])
    # (filled with a pattern no observation holds, so that a byte the kernel leaves unwritten shows)
    return eng.new(shape, torch.bfloat16 if layout == NCHW_BF16 else torch.float32, 7.0)


def _bits(t):
    import torch
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _w_axis(layout):
    from snake_engine.engine import NHWC_F32
    return 2 if layout == NHWC_F32 else 3


def _plain(eng, d_pairs, d_index, m, layout):
    out = _alloc(eng, m, layout)
    eng.observe(d_pairs, m, out, layout=layout, index=d_index)          # snk_engine_observe_rows
    return out


def _expected(plain, flags, layout):
    import torch
    want = plain.clone()
    rows = torch.nonzero(flags).flatten()
    want[rows] = torch.flip(plain[rows], dims=[_w_axis(layout)])
    return want


@pytest.mark.parametrize("cfg", CFGS)
def test_flagged_rows_are_the_w_flip_of_the_plain_rows(se, cfg):
    """every geometry, all three layouts, rows permuted by d_index; mirror[i] = (i // 4) & 1 puts each of the four 16-byte
    alignments an NHWC row can start at (its 3 (2H-1)(2W-1) floats are an odd count) on a mirrored and on a plain row"""
    import torch
    from snake_engine.engine import NHWC_F32, NCHW_F32, NCHW_BF16
    eng, pairs, _ = _boards(se, cfg)
    m = len(pairs)
    assert m >= 8
    perm = np.random.RandomState(0).permutation(m).astype(np.int32)
    d_pairs, d_index = torch.as_tensor(pairs, device="cuda"), torch.as_tensor(perm, device="cuda")
    flags = ((torch.arange(m, device="cuda") // 4) & 1).to(torch.uint8)
    dead_row = int(np.flatnonzero(perm == m - 1)[0])
    for layout in (NHWC_F32, NCHW_F32, NCHW_BF16):
        plain = _plain(eng, d_pairs, d_index, m, layout)
        got = _alloc(eng, m, layout)
        eng.observe(d_pairs, m, got, layout=layout, index=d_index, mirror=flags)
        assert torch.equal(_bits(got), _bits(_expected(plain, flags, layout))), (cfg, layout)
        assert not _bits(got[dead_row]).any().item() and not _bits(plain[dead_row]).any().item()
        # the flip moved something: the mirrored launch is not the plain one
        assert not torch.equal(_bits(got), _bits(plain))
    # the dead row, mirrored: still all zero
    one = torch.ones(m, dtype=torch.uint8, device="cuda")
    got = _alloc(eng, m, NHWC_F32)
    eng.observe(d_pairs, m, got, index=d_index, mirror=one)
    assert not _bits(got[dead_row]).any().item()


@pytest.mark.parametrize("cfg", ["9x9x3", "11x11x4", "19x19x8"])
def test_null_and_zero_flags_write_the_plain_bytes(se, cfg):
    import torch
    from snake_engine._lib import check
    from snake_engine.engine import NHWC_F32, NCHW_F32, NCHW_BF16, _stream
    eng, pairs, _ = _boards(se, cfg)
    m = len(pairs)
    perm = np.random.RandomState(1).permutation(m).astype(np.int32)
    d_pairs, d_index = torch.as_tensor(pairs, device="cuda"), torch.as_tensor(perm, device="cuda")
    zeros = torch.zeros(m, dtype=torch.uint8, device="cuda")
    for layout in (NHWC_F32, NCHW_F32, NCHW_BF16):
        for index in (d_index, None):
            plain = _plain(eng, d_pairs, index, m, layout)
            got0 = _alloc(eng, m, layout)
            eng.observe(d_pairs, m, got0, layout=layout, index=index, mirror=zeros)
            assert torch.equal(_bits(got0), _bits(plain)), (cfg, layout, "zero flags")
            gotn = _alloc(eng, m, layout)
            check(eng.L.snk_engine_observe_mirror(eng.h, d_pairs.data_ptr(), index.data_ptr() if index is not None else None, None,
                                                  m, layout, gotn.data_ptr(), _stream()))
            assert torch.equal(_bits(gotn), _bits(plain)), (cfg, layout, "NULL flags")


def test_two_observations_per_wavefront(se):
    """from 32 768 rows on a wavefront encodes two observations one after the other (the second one's record is fetched
    while the first is written, its flag read when its turn comes): 32 768 + 5 rows of the 11x11x4 pairs, the flag alternating every four rows"""
    import torch
    eng, pairs, _ = _boards(se, "11x11x4")
    m = 32768 + 5
    d_pairs = torch.as_tensor(pairs, device="cuda")
    d_index = (torch.arange(m, device="cuda") % len(pairs)).to(torch.int32)
    flags = ((torch.arange(m, device="cuda") // 4) & 1).to(torch.uint8)
    plain = _plain(eng, d_pairs, d_index, m, 0)
    got = _alloc(eng, m, 0)
    eng.observe(d_pairs, m, got, index=d_index, mirror=flags)
    rows = torch.nonzero(flags).flatten()
    assert torch.equal(_bits(got[rows]), _bits(torch.flip(plain[rows], dims=[2])))
    rows = torch.nonzero(flags == 0).flatten()
    assert torch.equal(_bits(got[rows]), _bits(plain[rows]))


def test_mirroring_is_not_a_rotation(se):
    """a mirrored row of a state with last_move 1 is the flip of its own plain row -- and NOT the plain row of the same board
    with last_move 3, which is what swapping the rotation count instead of flipping the columns would write"""
    import torch
    from snake_engine.engine import state_from_compact
    z = load_golden("tic_11x11x4.npz")
    s = load_golden("states_11x11x4.npz")
    j = next(j for j in range(len(s["state_index"])) if int(z["st_dir"][s["state_index"][j]][s["snake_id"][j]]) & 3 == 1)
    si, sn = int(s["state_index"][j]), int(s["snake_id"][j])
    st = golden_state(z, si)
    turned = {k: np.array(v, copy=True) for k, v in st.items()}
    turned["dir"][sn] = 3
    eng = se.Engine(2, 11, 11, 4, 1, 0.15)
    eng.import_states([state_from_compact(11, 11, 4, st), state_from_compact(11, 11, 4, turned)])
    pairs = torch.as_tensor(np.array([[0, sn], [1, sn]], np.int32), device="cuda")
    plain = _plain(eng, pairs, None, 2, 0)
    got = _alloc(eng, 2, 0)
    eng.observe(pairs, 2, got, mirror=torch.tensor([1, 0], dtype=torch.uint8, device="cuda"))
    assert torch.equal(_bits(got[0]), _bits(torch.flip(plain[0], dims=[1])))
    assert torch.equal(_bits(got[1]), _bits(plain[1]))
    assert torch.equal(plain[1], torch.rot90(plain[0], 2, dims=[0, 1]))          # last_move 3 is the half turn of last_move 1
    assert not torch.equal(_bits(got[0]), _bits(plain[1]))


def test_mirror_rejects_mask_key_and_row_active(se):
    import torch
    eng = se.Engine(1, 7, 7, 2, 1, 0.15, seed=1)
    eng.reset()
    pairs = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    flags = torch.ones(1, dtype=torch.uint8, device="cuda")
    planes = _alloc(eng, 1, 0)
    for kw in (dict(mask=eng.new((1, 3), torch.uint8)), dict(key=eng.new((1, 2), torch.int64)),
               dict(sub_active=eng.new((1,), torch.uint8, 1), row_active=eng.new((1,), torch.uint8))):
        with pytest.raises(ValueError, match="mirror"):
            eng.observe(pairs, 1, planes, mirror=flags, **kw)
