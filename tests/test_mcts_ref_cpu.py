"""The NumPy model of the search kernels (tests/mcts_ref.py) checked on its own, without a GPU: Philox4x32-10 against
known-answer vectors, softermax / argmaxs against the tables recorded from the reference, the move choice against
numpy.searchsorted, and the table model's rules on a handful of hand-made cases."""
import numpy as np

from conftest import load_golden

import mcts_ref as M


def _words(s):
    return [int(w, 16) for w in s.split()]


def test_philox4x32_10_known_answers():
    """counter / key -> output, the Random123 known-answer vectors of philox4x32 with 10 rounds"""
    kat = [("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, out in kat:
        got = M.philox4x32_10(_words(ctr), _words(key))[0].tolist()
        assert got == _words(out), (ctr, key, [f"{w:08x}" for w in got])
    # rows are independent: a batch gives what the rows give one by one
    rows = np.array([0, 1, 63, 64, 1000, 0xFFFFFFFF], dtype=np.uint64)
    batch = M.philox4x32_10((rows, 7, 3, M.DRAW_TAG), (0x89ABCDEF, 0x01234567))
    for i, r in enumerate(rows):
        assert np.array_equal(batch[i], M.philox4x32_10((int(r), 7, 3, M.DRAW_TAG), (0x89ABCDEF, 0x01234567))[0])


def test_philox_uniform_layout():
    """counter (row, ctr0, ctr1, 'MCTS'), key (seed low, seed high), u = (r0 * 2^32 + r1 + 0.5) / 2^64"""
    seed = 0x0123456789ABCDEF
    u = M.philox_uniform(np.arange(5), 7, 3, seed)
    for i in range(5):
        r = M.philox4x32_10((i, 7, 3, 0x4D435453), (0x89ABCDEF, 0x01234567))[0]
        assert u[i] == ((int(r[0]) << 32) + int(r[1]) + 0.5) / 2.0 ** 64
    assert ((u > 0) & (u < 1)).all()
    assert not np.array_equal(u, M.philox_uniform(np.arange(5), 3, 7, seed)), "ctr0 and ctr1 are different counter words"
    assert not np.array_equal(u, M.philox_uniform(np.arange(5), 7, 3, (seed >> 32) | ((seed & 0xFFFFFFFF) << 32)))


def test_softermax_and_argmaxs_agree_with_the_recorded_tables():
    z = load_golden("tables.npz")
    for base in (2, 3, 10, 100):
        pmf, ref = M.softermax3(base, z["z"]), z[f"pmf_b{base}"]
        assert np.array_equal(pmf == 0, ref == 0)
        assert np.abs(pmf - ref).max() <= 2e-6, (base, np.abs(pmf - ref).max())
        assert np.abs(pmf.sum(axis=1) - 1).max() <= 1e-12
    assert M.argmaxs(z["argmax_z"]).tolist() == z["argmax"].tolist()
    # the documented clamps: all cells -1 -> uniform; +1 cells share the mass
    assert np.array_equal(M.softermax3(100, [[-1, -1, -1]]), np.full((1, 3), 1.0 / 3.0))
    assert M.softermax3(2, [[1, 0.5, -1], [1, 1, 0], [1, 1, 1]]).tolist() == [[1, 0, 0], [0.5, 0.5, 0], [1 / 3, 1 / 3, 1 / 3]]


def test_choice3_is_searchsorted_right_on_the_normalised_cumsum():
    rng = np.random.RandomState(3)
    n = 10_000
    pmf = rng.random_sample((n, 3)).astype(np.float32)
    pmf[rng.random_sample((n, 3)) < 0.15] = 0          # zero cells, as obstacle masks give
    pmf[pmf.sum(axis=1) == 0] = 1.0 / 3.0
    pmf = (pmf / pmf.sum(axis=1, keepdims=True)).astype(np.float32)       # sums to 1 only up to float32 rounding
    u = rng.random_sample(n)
    cdfs = []
    for i in range(n):
        cdf = pmf[i].astype(np.float64).cumsum()
        cdf /= cdf[-1]
        cdfs.append(cdf)
        if i % 4 == 1 and cdf[0] < 1.0:
            u[i] = cdf[0]                              # exactly on an edge: 'right' puts it in the next cell
        elif i % 4 == 2 and cdf[1] < 1.0:
            u[i] = cdf[1]
        elif i % 4 == 3 and cdf[0] > 0.0:
            u[i] = np.nextafter(cdf[0], 0.0)           # the last value of the first cell
    want = np.array([np.searchsorted(cdfs[i], u[i], side="right") for i in range(n)])
    got = M.choice3(pmf, u)
    assert np.array_equal(got, want)
    assert got.max() == 2 and got.min() == 0
    assert np.array_equal(np.stack(cdfs), M.choice_cdf(pmf))


def test_table_model_rules():
    t = M.TableModel(1024)
    keys = [(5, 9), (0, 0), (0, 7), (1, 7), (7, 0), (5, 9), (5, 10)]
    rows, new = t.lookup(keys, [1, 1, 1, 1, 1, 1, 0], now=1, max_age=2)
    assert rows == [(5, 9), None, (1, 7), (1, 7), (7, 1), (5, 9), None]
    assert new == {(5, 9), (1, 7), (7, 1)} and t.occupied() == 3
    t.set_priors(rows, np.arange(21, dtype=np.float32).reshape(7, 3))
    assert t.entries[(5, 9)]["total"].tolist() == [15, 16, 17] and t.entries[(5, 9)]["visit"].tolist() == [1, 1, 1]
    # exists during turn now iff now - touch <= max_age + 1; a stale hit is re-created in place; every hit touches
    assert t.find([(5, 9)], now=4, max_age=2)[0] == [(5, 9)] and t.find([(5, 9)], now=5, max_age=2)[0] == [None]
    assert t.find([(5, 9)], now=4, max_age=2)[1][0].tolist() == [15, 16, 17, 1, 1, 1, 3]
    assert t.lookup([(5, 9)], None, now=4, max_age=2)[1] == set() and t.entries[(5, 9)]["touch"] == 4
    assert t.lookup([(7, 0)], None, now=5, max_age=2)[1] == {(7, 1)} and t.occupied() == 3
    # a rebuild keeps an entry iff now - touch <= max_age
    t.lookup([(1, 7)], None, now=3, max_age=2)
    t.rebuild(2048, now=5, max_age=2)
    assert set(t.entries) == {(5, 9), (7, 1), (1, 7)} and t.cap == 2048
    t.rebuild(1024, now=6, max_age=2)
    assert set(t.entries) == {(5, 9), (7, 1)}
    # probing wraps, and the occupied set does not depend on the order of insertion
    a, b = M.TableModel(1024), M.TableModel(1024)
    ks = [((j << 10) | (1020 + j % 4), j + 1) for j in range(40)]
    a.lookup(ks, None, 1, 8)
    b.lookup(ks[::-1], None, 1, 8)
    assert a.slot_set() == b.slot_set() == set(range(1020, 1024)) | set(range(36))
    # a full table: further keys get nothing and raise the flag
    f = M.TableModel(4)
    f.lookup([(i, i) for i in range(1, 5)], None, 1, 8)
    rows, new = f.lookup([(9, 9), (2, 2)], None, 1, 8)
    assert rows == [None, (2, 2)] and new == set() and f.overflowed == 1 and f.occupied() == 4


def test_back_up_models_on_a_hand_made_case():
    tot = np.array([[0.5, 0.25, -0.5], [0.0, 1.0, -1.0]], np.float32)
    vis = np.ones((2, 3), np.float32)
    entry = np.array([0, M.NONE, 1, 1], dtype=np.uint32)
    pe = np.array([[1, 9], [0, 0], [0, 1], [9, 9]], dtype=np.uint32)
    pm = np.array([[2, 0], [0, 0], [1, 0], [0, 0]], dtype=np.uint8)
    ln = np.array([1, 2, 2, 0], np.int32)
    est = np.array([0.5, 9.0, -0.25, 3.0], np.float32)
    t2, v2, l2 = M.backup_production(tot, vis, entry, est, pe, pm, ln, 2)
    assert t2.tolist() == [[0.5, 0.0, -0.5], [-0.25, 1.0, -0.5]] and v2.tolist() == [[1, 2, 1], [2, 1, 2]]
    assert l2.tolist() == [2, 2, 2, 1]
    # the sequential order re-reads the statistics: row 2's estimate sees what row 0 added to entry 1
    pmf = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 1], [1, 0, 0]], np.float32)
    t3, v3, _ = M.backup_sequential(tot, vis, entry, pmf, pe, pm, ln, 2)
    assert t3[1, 2] == np.float32(-1.0) + np.float32(-0.5) and v3[1, 2] == 2           # row 0: est = q[0][2] = -0.5
    r2 = t3[1, 2] / v3[1, 2]                                                             # row 2 reads -1.5 / 2
    assert t3[0, 1] == np.float32(0.25) + r2 and t3[1, 0] == r2
    t4, v4 = M.terminal_backup(tot, vis, np.array([1, -1, 0, 1], np.int8), pe, pm, ln, 2, sequential=False)
    assert t4.tolist() == [[-1.5, 0.25, -0.5], [0.0, 1.0, 0.0]] and v4.tolist() == [[3, 1, 1], [1, 1, 2]]
    act, steps = M.retire([1, 1, 0, 1], [0, 1, 1, 0], [5, 5, 1, 3], 3, (1 << 33) + 5)
    assert act.tolist() == [1, 0, 0, 0] and steps == (1 << 33) + 8
