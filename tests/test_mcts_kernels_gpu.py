"""The search's device side (csrc/mcts.hip) kernel by kernel against the NumPy model of tests/mcts_ref.py: every entry
point called directly, in the mode bench.py times (one thread per row, float atomics, Philox draws) as well as in the
sequential parity mode, at row counts that cross the wavefront (64) and the block (256) edges.

Tolerances: the pmf is compared with the float64 model within 2e-6 (the bound test_softermax_argmax_tables uses on the
same inputs: the device's float32 powf / atanhf against NumPy's); everything else -- entries, flags, moves, estimates,
statistics, paths, counters -- is compared exactly."""
import numpy as np
import pytest

from conftest import load_golden

import mcts_ref as M

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 255, 257, 1000]
NONE = M.NONE


class Dev:
    """the C ABI of the search with NumPy in and out"""

    def __init__(self, torch, se):
        from snake_engine._lib import lib, check
        self.torch, self.se, self.L, self.check = torch, se, lib(), check
        self.st = torch.cuda.current_stream().cuda_stream

    def up(self, a, dtype=None):
        a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        elif a.dtype == np.uint64:
            a = a.view(np.int64)
        return self.torch.as_tensor(a, device="cuda")

    def zeros(self, shape, dtype):
        return self.torch.zeros(shape, dtype=dtype, device="cuda")

    @staticmethod
    def p(t):
        return None if t is None else t.data_ptr()

    def table(self, capacity):
        from snake_engine.mcts import TranspositionTable
        return TranspositionTable(capacity)

    def lookup(self, tt, keys, now, max_age, active=None):
        m = len(keys)
        k, a = self.up(np.asarray(keys, dtype=np.uint64).reshape(m, 2)), None if active is None else self.up(active, np.uint8)
        e, nw = self.zeros(m, self.torch.int32), self.zeros(m, self.torch.uint8)
        self.check(self.L.snk_tt_lookup_insert(tt.h, k.data_ptr(), self.p(a), m, now, max_age, e.data_ptr(), nw.data_ptr(), self.st))
        return e.cpu().numpy().view(np.uint32), nw.cpu().numpy()

    def find(self, tt, keys, now, max_age, want_stat=True):
        m = len(keys)
        k = self.up(np.asarray(keys, dtype=np.uint64).reshape(m, 2))
        e = self.zeros(m, self.torch.int32)
        s = self.torch.full((m, 7), -77.0, dtype=self.torch.float32, device="cuda") if want_stat else None
        self.check(self.L.snk_tt_find(tt.h, k.data_ptr(), m, now, max_age, e.data_ptr(), self.p(s), self.st))
        return e.cpu().numpy().view(np.uint32), (s.cpu().numpy() if want_stat else None)

    def set_priors(self, tt, entry, q):
        e, qq = self.up(entry), self.up(q, np.float32)
        self.check(self.L.snk_tt_set_priors(tt.h, e.data_ptr(), None, len(entry), qq.data_ptr(), None, self.st))

    def read_q(self, tt, entry_buf, stride, m):
        e = self.up(entry_buf)
        q = self.torch.full((m, 3), -77.0, dtype=self.torch.float32, device="cuda")
        self.check(self.L.snk_tt_read_q(tt.h, e.data_ptr(), stride, m, q.data_ptr(), self.st))
        return q.cpu().numpy()


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    import snake_engine
    return Dev(torch, snake_engine)


def _rand_keys(rng, n):
    """n distinct key pairs, both words non-zero"""
    k = rng.randint(1, 1 << 62, size=(n, 2)).astype(np.uint64)
    assert len({tuple(r) for r in k.tolist()}) == n
    return k


def _check_lookup(rows, new, entry, is_new):
    """rows / new: the model's verdict; entry / is_new: the device's.  Returns {key: entry}."""
    by_key = {}
    for i, k in enumerate(rows):
        if k is None:
            assert entry[i] == NONE and is_new[i] == 0, i
        else:
            assert entry[i] != NONE, (i, k)
            assert by_key.setdefault(k, int(entry[i])) == int(entry[i]), "rows of one key share its entry"
    assert len(set(by_key.values())) == len(by_key), "distinct keys, distinct entries"
    for k in by_key:
        n_new = int(sum(is_new[i] for i, r in enumerate(rows) if r == k))
        assert n_new == (1 if k in new else 0), (k, n_new)
    return by_key


# ------------------------------------------------------------------------------------------------------------ the table
def test_table_probing_wraps_past_the_last_slot(dev):
    tt, model = dev.table(1024), M.TableModel(1024)
    rng = np.random.RandomState(1)
    keys = np.array([[(int(rng.randint(1, 1 << 40)) << 10) | (1020 + j % 4), int(rng.randint(1, 1 << 62))] for j in range(40)], dtype=np.uint64)
    entry, is_new = dev.lookup(tt, keys, 1, 8)
    rows, new = model.lookup(keys.tolist(), None, 1, 8)
    by_key = _check_lookup(rows, new, entry, is_new)
    assert set(by_key.values()) == model.slot_set() == set(range(1020, 1024)) | set(range(36))
    assert len(by_key) == 40 and is_new.sum() == 40
    found, _ = dev.find(tt, keys, 1, 8)
    assert np.array_equal(found, entry), "snk_tt_find follows the same wrapped probe sequence"
    assert tt.status() == (1024, 40, 0)


def test_table_keys_that_share_key_lo(dev):
    tt, model = dev.table(1024), M.TableModel(1024)
    rng = np.random.RandomState(2)
    base = np.array([[0x1234567890ABCDEF, int(h)] for h in rng.randint(1, 1 << 62, size=32)], dtype=np.uint64)
    rows_idx = rng.permutation(np.repeat(np.arange(32), rng.randint(1, 5, size=32)))
    keys = base[rows_idx]
    entry, is_new = dev.lookup(tt, keys, 1, 8)
    rows, new = model.lookup(keys.tolist(), None, 1, 8)
    by_key = _check_lookup(rows, new, entry, is_new)
    assert len(by_key) == 32 and is_new.sum() == 32 and tt.status()[1] == 32
    assert set(by_key.values()) == model.slot_set()
    found, _ = dev.find(tt, base, 1, 8)
    assert [int(e) for e in found] == [by_key[tuple(k)] for k in base.tolist()]


def test_table_keys_with_a_zero_word(dev):
    tt, model = dev.table(1024), M.TableModel(1024)
    x, y = 0x0F0F0F0F12345678, 0x7000000000000421
    keys = np.array([[0, x], [x, 0], [0, 0], [0, y], [1, y], [y, 0], [0, x], [0, 0]], dtype=np.uint64)
    entry, is_new = dev.lookup(tt, keys, 1, 8)
    rows, new = model.lookup(keys.tolist(), None, 1, 8)
    by_key = _check_lookup(rows, new, entry, is_new)
    assert len(by_key) == 4 and entry[2] == NONE and entry[7] == NONE          # (0, y) and (1, y) are one key: the remap's price
    assert set(by_key.values()) == model.slot_set() and tt.status()[1] == 4
    once = np.array([i not in (4, 6) for i in range(8)])          # priors from one row per key
    dev.set_priors(tt, np.where(once, entry, NONE).astype(np.uint32), np.arange(24, dtype=np.float32).reshape(8, 3))
    model.set_priors([r if once[i] else None for i, r in enumerate(rows)], np.arange(24, dtype=np.float32).reshape(8, 3))
    found, stat = dev.find(tt, keys[[0, 1, 2, 5]], 1, 8)
    want_rows, want_stat = model.find(keys[[0, 1, 2, 5]].tolist(), 1, 8)
    assert [int(e) for e in found] == [NONE if k is None else by_key[k] for k in want_rows]
    assert found[2] == NONE and (found[[0, 1, 3]] != NONE).all()
    assert np.array_equal(stat, want_stat) and np.array_equal(stat[2], np.zeros(7, np.float32))
    e2, n2 = dev.lookup(tt, keys, 2, 8)
    assert np.array_equal(e2, entry) and n2.sum() == 0


def test_table_fills_up_then_overflows(dev):
    tt, model = dev.table(1024), M.TableModel(1024)
    rng = np.random.RandomState(3)
    keys = _rand_keys(rng, 1024 + 5)
    full, extra = keys[:1024], keys[1024:]
    entry, is_new = dev.lookup(tt, full, 1, 8)
    rows, new = model.lookup(full.tolist(), None, 1, 8)
    by_key = _check_lookup(rows, new, entry, is_new)
    assert sorted(by_key.values()) == list(range(1024)) and is_new.sum() == 1024
    assert tt.status() == (1024, 1024, 0) and model.overflowed == 0
    found, _ = dev.find(tt, full, 1, 8)
    assert np.array_equal(found, entry)
    e2, n2 = dev.lookup(tt, full, 2, 8)
    assert np.array_equal(e2, entry) and n2.sum() == 0 and tt.status() == (1024, 1024, 0)
    e3, n3 = dev.lookup(tt, extra, 2, 8)
    rows3, new3 = model.lookup(extra.tolist(), None, 2, 8)
    assert rows3 == [None] * 5 and not new3 and model.overflowed == 1
    assert (e3 == NONE).all() and n3.sum() == 0
    assert tt.status() == (1024, 1024, 1)
    f3, s3 = dev.find(tt, extra, 2, 8)
    assert (f3 == NONE).all() and not s3.any()
    tt.clear()
    assert tt.status() == (1024, 0, 0)
    f4, _ = dev.find(tt, full[:64], 2, 8)
    assert (f4 == NONE).all()


@pytest.mark.parametrize("m", ROWS)
def test_table_find_is_read_only_and_honours_the_eviction_boundary(dev, m):
    tt, model = dev.table(1024), M.TableModel(1024)
    rng = np.random.RandomState(100 + m)
    max_age, now = 4, 12
    keys = _rand_keys(rng, min(m, 600))
    turn = 1 + (6 + np.arange(len(keys))) % 12           # key 0: age 5 = max_age + 1 (the last turn it exists); key 11: age 6
    by_key = {}
    for t in range(1, 13):
        sel = np.flatnonzero(turn == t)
        if not len(sel):
            continue
        e, nw = dev.lookup(tt, keys[sel], t, max_age)
        rows, new = model.lookup(keys[sel].tolist(), None, t, max_age)
        by_key.update(_check_lookup(rows, new, e, nw))
        q = rng.randint(-1024, 1025, size=(len(sel), 3)).astype(np.float32) / 1024
        dev.set_priors(tt, e, q)
        model.set_priors(rows, q)
    # m probe rows: the inserted keys (repeated to fill m rows), absent keys, a (0, 0)
    probe = keys[np.arange(m) % len(keys)]
    probe[3::7] = _rand_keys(rng, len(probe[3::7]))
    if m > 2:
        probe[2] = 0
    found, stat = dev.find(tt, probe, now, max_age)
    want_rows, want_stat = model.find(probe.tolist(), now, max_age)
    assert [int(e) for e in found] == [NONE if k is None else by_key[k] for k in want_rows]
    assert np.array_equal(stat, want_stat)
    if m >= 63:
        ages = want_stat[[k is not None for k in want_rows], 6]
        assert ages.max() == max_age + 1 and any(k is None and tuple(p) in by_key for k, p in zip(want_rows, probe.tolist()))
    found2, _ = dev.find(tt, probe, now, max_age, want_stat=False)
    assert np.array_equal(found2, found)
    # nothing was touched: one turn later the entries of age max_age + 1 have gone stale, as if find had never run
    e3, n3 = dev.lookup(tt, keys, now + 1, max_age)
    rows3, new3 = model.lookup(keys.tolist(), None, now + 1, max_age)
    _check_lookup(rows3, new3, e3, n3)
    assert n3.sum() == len(new3) == int((now + 1 - turn > max_age + 1).sum())


def _aged_table(dev, rng, n_keys, n_pairs):
    """a 4096-slot table whose entries were touched at turns 1..12; the last 2 * n_pairs keys share key_lo in pairs"""
    tt, model = dev.table(4096), M.TableModel(4096)
    keys = _rand_keys(rng, n_keys)
    keys[n_keys - n_pairs:, 0] = keys[n_keys - 2 * n_pairs:n_keys - n_pairs, 0]
    turn = 1 + np.arange(n_keys) % 12
    turn[n_keys - 2 * n_pairs:] = 7 + np.arange(2 * n_pairs) % 6           # the pairs survive (touch >= 7), on the boundary too
    for t in range(1, 13):
        sel = np.flatnonzero(turn == t)
        e, nw = dev.lookup(tt, keys[sel], t, 5)
        rows, new = model.lookup(keys[sel].tolist(), None, t, 5)
        _check_lookup(rows, new, e, nw)
        q = rng.randint(-1024, 1025, size=(len(sel), 3)).astype(np.float32) / 1024
        dev.set_priors(tt, e, q)
        model.set_priors(rows, q)
    return tt, model, keys, turn


@pytest.mark.parametrize("new_cap", [1024, 4096, 8192])
def test_table_rebuild_keeps_exactly_the_survivors(dev, new_cap):
    rng = np.random.RandomState(new_cap)
    tt, model, keys, turn = _aged_table(dev, rng, 640, 20)
    now, max_age = 12, 5
    assert tt.status() == (4096, 640, 0)
    tt.rebuild(new_cap, now, max_age)
    model.rebuild(new_cap, now, max_age)
    survives = now - turn <= max_age
    assert survives[turn == 7].all() and not survives[turn == 6].any() and (turn == 6).any() and (turn == 7).any()
    assert tt.status() == (new_cap, model.occupied(), 0) and model.occupied() == int(survives.sum())
    # find sees an entry up to age max_age + 1: a wrongly kept entry of age 6 would be found here
    found, stat = dev.find(tt, keys, now, max_age)
    want_rows, want_stat = model.find(keys.tolist(), now, max_age)
    assert np.array_equal(found != NONE, survives) and [k is not None for k in want_rows] == survives.tolist()
    assert np.array_equal(stat, want_stat), "statistics and touch turns survive the rebuild unchanged"
    assert (found[-40:] != NONE).all(), "keys that share key_lo both survive"
    assert len(set(found[survives].tolist())) == int(survives.sum())
    assert set(found[survives].tolist()) == model.slot_set()


def test_table_rebuild_into_too_few_slots_raises_the_overflow_flag(dev):
    tt, model = dev.table(4096), M.TableModel(4096)
    keys = _rand_keys(np.random.RandomState(5), 1500)
    e, nw = dev.lookup(tt, keys, 12, 5)
    _check_lookup(*model.lookup(keys.tolist(), None, 12, 5), e, nw)
    assert tt.status() == (4096, 1500, 0)
    tt.rebuild(1024, 12, 5)
    model.rebuild(1024, 12, 5)
    assert model.overflowed == 1 and model.occupied_after_rebuild() == 1024
    assert tt.status() == (1024, 1024, 1), "476 survivors were dropped: the new table must say so"


@pytest.mark.parametrize("m", ROWS)
def test_read_q_strides(dev, m):
    rng = np.random.RandomState(m)
    s = _Search(dev, rng, 23)
    for stride in (1, 5):
        buf = rng.randint(0, 1 << 31, size=(m, stride)).astype(np.uint32)
        ent = rng.randint(0, s.n, size=m).astype(np.uint32)
        ent[rng.random_sample(m) < 0.2] = NONE
        buf[:, 0] = s.slots(ent)
        want, ok = M.read_q(s.tot, s.vis, ent)
        got = dev.read_q(s.tt, buf.reshape(-1), stride, m)
        assert got.tobytes() == want.tobytes()
        assert not got[~ok].any()


# ------------------------------------------------------------------------------------------------------------ select / back-up
class _Search:
    """a 1024-slot table with n entries; the model's statistics live in tot / vis [n][3], indexed by key number.
    Statistics start as priors that are multiples of 2^-10, then one contended production back-up makes every visit count
    1..50 and every total a multiple of 2^-10 (exact in any order): q = total / visit is a proper ratio."""

    def __init__(self, dev, rng, n, cap=1024, ratio=True, priors=None):
        self.dev, self.n = dev, n
        self.tt = dev.table(cap)
        self.keys = _rand_keys(rng, n)
        self.ent, nw = dev.lookup(self.tt, self.keys, 1, 8)
        assert nw.sum() == n and len(set(self.ent.tolist())) == n and NONE not in self.ent
        self.tot = (rng.randint(-1024, 1025, size=(n, 3)).astype(np.float32) / 1024) if priors is None else np.asarray(priors, np.float32)
        self.vis = np.ones((n, 3), np.float32)
        dev.set_priors(self.tt, self.ent, self.tot)
        if ratio:
            cnt = rng.randint(0, 50, size=(n, 3))
            e, mv = np.repeat(np.arange(n), cnt.sum(axis=1)), np.concatenate([np.repeat(np.arange(3), c) for c in cnt])
            perm = rng.permutation(len(e))
            e, mv = e[perm].astype(np.uint32), mv[perm].astype(np.uint8)
            est = rng.randint(-1024, 1025, size=len(e)).astype(np.float32) / 1024
            self.backup(e, est, e.reshape(-1, 1), mv.reshape(-1, 1), np.ones(len(e), np.int32), 1)
            assert self.vis.max() <= 50 and self.vis.min() >= 1
            self.check_stats()

    def slots(self, ent):
        """key numbers -> device entries (NONE stays NONE)"""
        ent = np.asarray(ent, dtype=np.uint32)
        out = np.full(ent.shape, NONE, dtype=np.uint32)
        out[ent != NONE] = self.ent[ent[ent != NONE]]
        return out

    def check_stats(self):
        found, stat = self.dev.find(self.tt, self.keys, 1, 8)
        assert np.array_equal(found, self.ent)
        assert stat[:, 0:3].tobytes() == self.tot.tobytes(), "totals are bit-equal to the model's"
        assert stat[:, 3:6].tobytes() == self.vis.tobytes(), "visit counts are bit-equal to the model's"

    def select(self, entry, base, D, pe, pm, ln, tape=None, rank=None, tape_base=0, seed=0, ctr=(0, 0), want_est=True, want_pmf=True,
               gate=None):
        """one snk_mcts_select launch.  entry / pe in key numbers.  Returns moves, est, pmf, path_entry (key numbers), path_move, len."""
        d, t = self.dev, self.dev.torch
        m = len(entry)
        d_e, d_pe, d_pm, d_ln = d.up(self.slots(entry)), d.up(self.slots(pe)), d.up(pm, np.uint8), d.up(ln, np.int32)
        mv = t.full((m,), 9, dtype=t.uint8, device="cuda")
        est = t.full((m,), -77.0, dtype=t.float32, device="cuda") if want_est else None
        pmf = t.full((m, 3), -77.0, dtype=t.float32, device="cuda") if want_pmf else None
        d_tape = None if tape is None else d.up(tape, np.float64)
        d_rank = None if rank is None else d.up(rank, np.int32)
        d.check(d.L.snk_mcts_select(self.tt.h, d_e.data_ptr(), m, float(base), d.p(d_tape), d.p(d_rank), int(tape_base), int(seed), ctr[0], ctr[1],
                                    mv.data_ptr(), d.p(est), d.p(pmf), d_pe.data_ptr(), d_pm.data_ptr(), d_ln.data_ptr(), D, d.p(gate), d.st))
        back = {int(s): j for j, s in enumerate(self.ent)}
        got_pe = d_pe.cpu().numpy().view(np.uint32)
        pe_keys = np.array([NONE if int(x) == NONE else back.get(int(x), NONE - 1) for x in got_pe.reshape(-1)], dtype=np.uint32).reshape(got_pe.shape)
        return (mv.cpu().numpy(), None if est is None else est.cpu().numpy(), None if pmf is None else pmf.cpu().numpy(),
                pe_keys, d_pm.cpu().numpy(), d_ln.cpu().numpy())

    def backup(self, entry, est, pe, pm, ln, D, sequential=False, pmf=None, gate=None, apply=True):
        """one snk_mcts_backup launch and the model's version of it on tot / vis; returns (device len, model len)"""
        d = self.dev
        m = len(entry)
        d_e, d_pe, d_pm, d_ln = d.up(self.slots(entry)), d.up(self.slots(pe)), d.up(pm, np.uint8), d.up(ln, np.int32)
        d_est = None if est is None else d.up(est, np.float32)
        d_pmf = None if pmf is None else d.up(pmf, np.float32)
        d.check(d.L.snk_mcts_backup(self.tt.h, d_e.data_ptr(), m, d.p(d_est), d.p(d_pmf), d_pe.data_ptr(), d_pm.data_ptr(), d_ln.data_ptr(), D,
                                    int(sequential), d.p(gate), d.st))
        want_len = np.asarray(ln, np.int32)
        if apply:
            if sequential:
                self.tot, self.vis, want_len = M.backup_sequential(self.tot, self.vis, entry, pmf, pe, pm, ln, D)
            else:
                self.tot, self.vis, want_len = M.backup_production(self.tot, self.vis, entry, est, pe, pm, ln, D)
        assert np.array_equal(d_pe.cpu().numpy().view(np.uint32), self.slots(pe).reshape(d_pe.shape)) and np.array_equal(d_pm.cpu().numpy(), pm)
        return d_ln.cpu().numpy(), want_len

    def terminal(self, rewards, pe, pm, ln, D, sequential):
        d = self.dev
        d_r, d_pe, d_pm, d_ln = d.up(rewards, np.int8), d.up(self.slots(pe)), d.up(pm, np.uint8), d.up(ln, np.int32)
        d.check(d.L.snk_mcts_terminal_backup(self.tt.h, d_r.data_ptr(), len(rewards), d_pe.data_ptr(), d_pm.data_ptr(), d_ln.data_ptr(), D,
                                             int(sequential), d.st))
        self.tot, self.vis = M.terminal_backup(self.tot, self.vis, rewards, pe, pm, ln, D, sequential)
        assert np.array_equal(d_ln.cpu().numpy(), ln), "the terminal back-up leaves len alone"


def _rows(rng, s, m, D, p_none=0.15):
    """m rows over the table's entries, some without one, with paths of length 0..D whose unused tail holds other valid entries"""
    entry = rng.randint(0, s.n, size=m).astype(np.uint32)
    entry[rng.random_sample(m) < p_none] = NONE
    pe = rng.randint(0, s.n, size=(m, D)).astype(np.uint32)
    pm = rng.randint(0, 3, size=(m, D)).astype(np.uint8)
    ln = (np.arange(m) % (D + 1)).astype(np.int32)
    rng.shuffle(ln)
    return entry, pe, pm, ln


def _gate(dev, v):
    return dev.up(np.array([v], np.int32))


def test_select_priors_from_the_recorded_tables(dev):
    """visits 1, so q == z exactly: the pmf of every recorded row, and of rows with +1 cells, against the float64 model"""
    z = np.concatenate([load_golden("tables.npz")["z"], np.array([[1, 0.5, -1], [1, 1, 0], [1, 1, 1], [-1, 1, -1]], np.float32)])
    m = len(z)
    rng = np.random.RandomState(8)
    s = _Search(dev, rng, m, cap=4096, ratio=False, priors=z)
    entry = np.arange(m, dtype=np.uint32)
    pe, pm, ln = np.zeros((m, 1), np.uint32), np.zeros((m, 1), np.uint8), np.ones(m, np.int32)
    u = rng.random_sample(m)
    for base in (2, 100):
        mv, est, pmf, _, _, _ = s.select(entry, base, 1, pe, pm, ln, tape=u)
        want = M.softermax3(base, z)
        err = np.abs(pmf - want).max()
        print(f"base {base}: max |pmf - float64 model| = {err:.3e} on {m} rows")
        assert np.array_equal(pmf == 0, want == 0)
        assert err <= 2e-6, err
        all_wall = (z == -1).all(axis=1)
        assert all_wall.sum() == 1 and (pmf[all_wall] == np.float32(1.0 / 3.0)).all()
        clamp = np.array([[1, 0, 0], [0.5, 0.5, 0], [1 / 3, 1 / 3, 1 / 3], [0, 1, 0]], np.float32)
        assert np.array_equal(pmf[-4:], clamp), "z == +1: the mass is shared by the +1 cells"
        assert np.array_equal(mv, M.choice3(pmf, u))
        assert est.tobytes() == M.est_of(pmf, z).tobytes()


@pytest.mark.parametrize("m", ROWS)
def test_select_estimate_is_the_float32_formula_on_ratio_statistics(dev, m):
    rng = np.random.RandomState(200 + m)
    s = _Search(dev, rng, 37)
    entry, pe, pm, ln = _rows(rng, s, m, 3)
    u = rng.random_sample(m)
    mv, est, pmf, _, _, _ = s.select(entry, 10, 3, pe, pm, ln, tape=u)
    q, ok = M.q_of(s.tot, s.vis, entry)
    assert len(np.unique(s.vis)) > 10, "visits vary: q is a ratio"
    want = M.softermax3(10, q)
    assert np.abs(pmf[ok] - want[ok]).max(initial=0) <= 2e-6
    assert est[ok].tobytes() == M.est_of(pmf, q)[ok].tobytes(), "est = (p0*q0 + p1*q1) + p2*q2 with q = total / visit, float32"
    assert not est[~ok].any() and (mv[~ok] == 1).all()
    assert (pmf[~ok] == -77.0).all(), "a row without an entry writes no pmf"
    assert np.array_equal(mv, M.select_moves(pmf, u, ok))
    got_q = dev.read_q(s.tt, s.slots(entry), 1, m)
    assert got_q.tobytes() == q.tobytes()


@pytest.mark.parametrize("m", ROWS)
def test_select_taped_draws_and_cdf_edges(dev, m):
    rng = np.random.RandomState(300 + m)
    s = _Search(dev, rng, 29)
    entry, pe, pm, ln = _rows(rng, s, m, 3)
    ok = entry != NONE
    rank = (np.cumsum(ok) - 1).astype(np.int32)              # a permutation with gaps, as the cumsum of an active mask gives
    n_act, tape_base = int(ok.sum()), 17
    tape = rng.random_sample(tape_base + n_act + 3)
    _, _, pmf, _, _, _ = s.select(entry, 3, 3, pe, pm, ln, tape=tape, rank=rank, tape_base=tape_base)
    # put some rows' uniforms exactly on the float64 cdf edges of the pmf the device returned, and just below the first
    cdf = M.choice_cdf(np.where(ok[:, None], pmf, np.float32(1 / 3)))
    kind = np.arange(m) % 4
    for i in np.flatnonzero(ok):
        if kind[i] == 1:
            tape[tape_base + rank[i]] = cdf[i, 0]
        elif kind[i] == 2:
            tape[tape_base + rank[i]] = cdf[i, 1]
        elif kind[i] == 3 and cdf[i, 0] > 0:
            tape[tape_base + rank[i]] = np.nextafter(cdf[i, 0], 0.0)
    tape[tape >= 1.0] = 0.5                                  # cdf[1] == 1 where the third cell is a wall: not a uniform
    mv, _, pmf2, _, _, _ = s.select(entry, 3, 3, pe, pm, ln, tape=tape, rank=rank, tape_base=tape_base)
    assert pmf2.tobytes() == pmf.tobytes()
    u = M.taped_uniform(tape, tape_base, rank, m, ok)
    assert np.array_equal(mv, M.select_moves(pmf, u, ok))
    on_first = ok & (kind == 1) & (u == cdf[:, 0]) & (cdf[:, 1] > cdf[:, 0])
    on_second = ok & (kind == 2) & (u == cdf[:, 1])
    below = ok & (kind == 3) & (cdf[:, 0] > 0) & (u < cdf[:, 0])
    assert (mv[on_first] == 1).all() and (mv[on_second] == 2).all() and (mv[below] == 0).all(), "searchsorted(..., 'right')"
    if m >= 63:
        assert on_first.any() and on_second.any() and below.any()
    # without d_rank row i reads tape[tape_base + i]
    tape2 = rng.random_sample(tape_base + m)
    mv2, _, pmf3, _, _, _ = s.select(entry, 3, 3, pe, pm, ln, tape=tape2, rank=None, tape_base=tape_base)
    assert np.array_equal(mv2, M.select_moves(pmf3, M.taped_uniform(tape2, tape_base, None, m, ok), ok))


def test_select_philox_draws_every_row(dev):
    m = 1000
    rng = np.random.RandomState(4)
    s = _Search(dev, rng, 211)
    entry, pe, pm, ln = _rows(rng, s, m, 8)
    ok = entry != NONE
    seed = 0x9E3779B97F4A7C15
    assert seed & 0xFFFFFFFF and seed >> 32
    mv, _, pmf, _, _, _ = s.select(entry, 2, 8, pe, pm, ln, seed=seed, ctr=(7, 3))
    u = M.philox_uniform(np.arange(m), 7, 3, seed)
    want = M.select_moves(pmf, u, ok)
    assert np.array_equal(mv, want), f"{int((mv != want).sum())} of {m} rows differ from the model's Philox draw"
    assert len(np.unique(mv[ok])) == 3
    mv2, _, pmf2, _, _, _ = s.select(entry, 2, 8, pe, pm, ln, seed=seed, ctr=(8, 3))
    want2 = M.select_moves(pmf2, M.philox_uniform(np.arange(m), 8, 3, seed), ok)
    assert np.array_equal(mv2, want2) and not np.array_equal(want, want2)
    # the counter words and the seed halves are not interchangeable
    for other in (M.philox_uniform(np.arange(m), 3, 7, seed), M.philox_uniform(np.arange(m), 7, 3, (seed >> 32) | ((seed & 0xFFFFFFFF) << 32))):
        assert not np.array_equal(M.select_moves(pmf, other, ok), mv)


@pytest.mark.parametrize("D", [3, 8])
@pytest.mark.parametrize("m", ROWS)
def test_select_appends_at_len_only_below_the_depth(dev, m, D):
    rng = np.random.RandomState(400 + m + D)
    s = _Search(dev, rng, 19)
    entry, pe, pm, ln = _rows(rng, s, m, D)
    u = rng.random_sample(m)
    mv, est, pmf, got_pe, got_pm, got_ln = s.select(entry, 2, D, pe, pm, ln, tape=u)
    ok = entry != NONE
    want_pe, want_pm = M.select_append(entry, mv, pe, pm, ln, D)
    assert np.array_equal(got_pe, want_pe) and np.array_equal(got_pm, want_pm)
    assert np.array_equal(got_ln, ln), "select leaves len alone"
    full = ok & (ln == D)
    assert np.array_equal(got_pe[full | ~ok], pe[full | ~ok]) and np.array_equal(got_pm[full | ~ok], pm[full | ~ok])
    if m >= 63:
        assert full.any() and (ok & (ln == 0)).any() and (~ok).any()
    assert (mv[~ok] == 1).all() and not est[~ok].any()
    # optional outputs: the same moves and paths without d_est / d_pmf
    mv2, _, _, pe2, pm2, _ = s.select(entry, 2, D, pe, pm, ln, tape=u, want_est=False, want_pmf=False)
    assert np.array_equal(mv2, mv) and np.array_equal(pe2, got_pe) and np.array_equal(pm2, got_pm)


@pytest.mark.parametrize("m", ROWS)
def test_select_gate(dev, m):
    rng = np.random.RandomState(500 + m)
    s = _Search(dev, rng, 19)
    entry, pe, pm, ln = _rows(rng, s, m, 3)
    u = rng.random_sample(m)
    mv, est, pmf, got_pe, got_pm, got_ln = s.select(entry, 2, 3, pe, pm, ln, tape=u, gate=_gate(dev, 1))
    assert (mv == 9).all() and (est == -77.0).all() and (pmf == -77.0).all()
    assert np.array_equal(got_pe, pe) and np.array_equal(got_pm, pm) and np.array_equal(got_ln, ln)
    open_ = s.select(entry, 2, 3, pe, pm, ln, tape=u, gate=_gate(dev, 0))
    plain = s.select(entry, 2, 3, pe, pm, ln, tape=u)
    for a, b in zip(open_, plain):
        assert a.tobytes() == b.tobytes()
    assert (plain[0] != 9).all()


def test_back_up_production_order_under_contention(dev):
    """1000 rows whose paths draw on 8 entries: hundreds of atomics land on each counter"""
    rng = np.random.RandomState(6)
    for D in (3, 8):
        s = _Search(dev, rng, 8, ratio=False)
        entry, pe, pm, ln = _rows(rng, s, 1000, D)
        est = rng.randint(-1024, 1025, size=1000).astype(np.float32) / 1024
        got_len, want_len = s.backup(entry, est, pe, pm, ln, D)
        s.check_stats()
        ok = entry != NONE
        assert np.array_equal(got_len, want_len)
        assert np.array_equal(got_len, np.where(ok & (ln < D), ln + 1, ln))
        assert s.vis.max() > 40, "contention: dozens of rows add to one counter"


@pytest.mark.parametrize("m", ROWS)
def test_back_up_sequential_order_with_live_re_reads(dev, m):
    rng = np.random.RandomState(600 + m)
    s = _Search(dev, rng, 8)
    for D in (3, 8):
        entry, pe, pm, ln = _rows(rng, s, m, D)
        pmf = rng.random_sample((m, 3)).astype(np.float32)
        pmf /= pmf.sum(axis=1, keepdims=True)
        got_len, want_len = s.backup(entry, None, pe, pm, ln, D, sequential=True, pmf=pmf)
        s.check_stats()                                       # the second round starts from totals that are arbitrary floats
        assert np.array_equal(got_len, want_len)


@pytest.mark.parametrize("sequential", [0, 1])
@pytest.mark.parametrize("m", ROWS)
def test_terminal_back_up(dev, m, sequential):
    rng = np.random.RandomState(700 + m + sequential)
    s = _Search(dev, rng, 8)                                  # totals are multiples of 2^-10: +-1 sums are exact in any order
    for D in (3, 8):
        _, pe, pm, ln = _rows(rng, s, m, D)
        rewards = rng.randint(-1, 2, size=m).astype(np.int8)
        before = s.tot.copy()
        s.terminal(rewards, pe, pm, ln, D, sequential)
        s.check_stats()
        if not rewards.any() or not ln[rewards != 0].any():
            assert np.array_equal(before, s.tot)
    s.terminal(np.zeros(m, np.int8), pe, pm, ln, D, sequential)      # None everywhere: nothing is added
    s.check_stats()


@pytest.mark.parametrize("sequential", [0, 1])
@pytest.mark.parametrize("m", ROWS)
def test_back_up_gate(dev, m, sequential):
    rng = np.random.RandomState(1000 + m + sequential)
    s = _Search(dev, rng, 8)
    entry, pe, pm, ln = _rows(rng, s, m, 3)
    est = rng.randint(-1024, 1025, size=m).astype(np.float32) / 1024
    pmf = np.full((m, 3), 1 / 3, np.float32)
    got_len, _ = s.backup(entry, est, pe, pm, ln, 3, sequential=sequential, pmf=pmf, gate=_gate(dev, 1), apply=False)
    assert np.array_equal(got_len, ln)
    s.check_stats()                                           # nothing moved
    got_len, want_len = s.backup(entry, est, pe, pm, ln, 3, sequential=sequential, pmf=pmf, gate=_gate(dev, 0))
    assert np.array_equal(got_len, want_len)
    if m >= 63:
        assert not np.array_equal(got_len, ln), "with the word 0 the back-up runs"
    s.check_stats()


# ------------------------------------------------------------------------------------------------------------ retire, root moves
@pytest.mark.parametrize("B", ROWS)
def test_retire_counts_and_retires(dev, B):
    t = dev.torch
    rng = np.random.RandomState(800 + B)
    active = (rng.random_sample(B) < 0.7).astype(np.uint8)
    active[-1] = 1                                            # the last, partial wavefront has something to count
    done = (rng.random_sample(B) < 0.3).astype(np.uint8)
    depth = rng.randint(1, 9, size=B).astype(np.int32)
    tick, start = 4, (1 << 33) + 5
    for gate_word in (1, 0, None):
        d_act, d_done, d_depth = dev.up(active), dev.up(done), dev.up(depth)
        ctr = t.full((1,), start, dtype=t.int64, device="cuda")
        gate = None if gate_word is None else _gate(dev, gate_word)
        dev.check(dev.L.snk_mcts_retire(d_act.data_ptr(), d_done.data_ptr(), d_depth.data_ptr(), tick, B, ctr.data_ptr(), dev.p(gate), dev.st))
        got_act, got_ctr = d_act.cpu().numpy(), int(ctr.item())
        if gate_word == 1:
            assert np.array_equal(got_act, active) and got_ctr == start, "a gated tick retires nothing and counts nothing"
            continue
        want_act, want_ctr = M.retire(active, done, depth, tick, start)
        assert got_ctr == want_ctr == start + int(active.sum())
        assert np.array_equal(got_act, want_act)
        assert not got_act[active == 0].any(), "inactive stays inactive whatever done says"
        assert np.array_equal(got_act == 0, (active == 0) | (done != 0) | (tick >= depth))


def _root_moves(dev, V, alive, base, training, tape=None, rank=None, tape_base=0, seed=0, ctr=(0, 0)):
    t = dev.torch
    m = len(alive)
    d_V, d_alive = dev.up(V, np.float32), dev.up(alive, np.uint8)
    d_tape = None if tape is None else dev.up(tape, np.float64)
    d_rank = None if rank is None else dev.up(rank, np.int32)
    mv = t.full((m,), 9, dtype=t.uint8, device="cuda")
    dev.check(dev.L.snk_mcts_root_moves(d_V.data_ptr(), d_alive.data_ptr(), m, float(base), int(training), dev.p(d_tape), dev.p(d_rank),
                                        int(tape_base), int(seed), ctr[0], ctr[1], mv.data_ptr(), dev.st))
    return mv.cpu().numpy()


def test_root_moves_play_mode_is_argmaxs(dev):
    z = load_golden("tables.npz")
    V = z["argmax_z"]
    alive = np.ones(len(V), np.uint8)
    alive[::9] = 0
    mv = _root_moves(dev, V, alive, 100, 0)
    assert np.array_equal(mv, M.root_moves_play(V, alive))
    assert np.array_equal(mv[alive != 0], z["argmax"][alive != 0]) and (mv[alive == 0] == 1).all()
    ties = (V[:, 0] == V[:, 1]) | (V[:, 1] == V[:, 2]) | (V[:, 0] == V[:, 2])
    assert (ties & (alive != 0)).any()


@pytest.mark.parametrize("m", ROWS)
def test_root_moves_training_mode(dev, m):
    t = dev.torch
    rng = np.random.RandomState(900 + m)
    V = (rng.random_sample((m, 3)) * 1.8 - 0.9).astype(np.float32)
    V[rng.random_sample((m, 3)) < 0.2] = -1.0
    alive = (rng.random_sample(m) < 0.8).astype(np.uint8)
    d_V = dev.up(V)
    pmf, am = t.empty((m, 3), dtype=t.float32, device="cuda"), t.empty((m,), dtype=t.uint8, device="cuda")
    dev.check(dev.L.snk_softermax_argmax(d_V.data_ptr(), m, 2.0, pmf.data_ptr(), am.data_ptr(), dev.st))
    pmf = pmf.cpu().numpy()
    assert np.abs(pmf - M.softermax3(2, V)).max() <= 2e-6 and np.array_equal(am.cpu().numpy(), M.argmaxs(V))
    rank = (np.cumsum(alive) - 1).astype(np.int32)
    tape_base = 5
    tape = rng.random_sample(tape_base + m)
    cdf = M.choice_cdf(pmf)
    for i in np.flatnonzero(alive)[::3]:
        if cdf[i, 0] < 1.0:
            tape[tape_base + rank[i]] = cdf[i, 0]             # on the edge
    mv = _root_moves(dev, V, alive, 2, 1, tape=tape, rank=rank, tape_base=tape_base)
    assert np.array_equal(mv, M.root_moves_training(pmf, M.taped_uniform(tape, tape_base, rank, m, alive), alive))
    mv = _root_moves(dev, V, alive, 2, 1, tape=tape, rank=None, tape_base=tape_base)
    assert np.array_equal(mv, M.root_moves_training(pmf, M.taped_uniform(tape, tape_base, None, m, alive), alive))
    seed = 0xC0FFEE1234567891
    mv = _root_moves(dev, V, alive, 2, 1, seed=seed, ctr=(11, 2))
    assert np.array_equal(mv, M.root_moves_training(pmf, M.philox_uniform(np.arange(m), 11, 2, seed), alive))
    assert (mv[alive == 0] == 1).all()


# ------------------------------------------------------------------------------------------------------------ overflow, end to end
def test_a_search_that_overflows_its_table_is_reported(dev):
    """1280 root rows into 1024 slots.  A row whose lookup found no room has no entry: every kernel of the tick skips it like an
    inactive row and nothing is appended to its path.  The root read-out is the one place that reads a path cell select may
    never have written: for a row that gets no entry in any tick of this first turn it sees the buffer's initial 'none' and
    returns zeros (a row that finds room at a later tick reads that later entry instead -- wrong, but in bounds, and the turn
    is refused anyway).  The turn's end reports the overflow."""
    torch, se = dev.torch, dev.se
    from snake_engine._lib import EngineError
    from snake_engine.mcts import DeviceMCTS
    from stubnet_device import stub_q_device
    G = 320
    eng = se.Engine(G, 11, 11, 4, 3, 0.15, seed=5)
    eng.reset()
    mcts = DeviceMCTS(stub_q_device, 11, 11, 4, 2, True, 8, 8, seed=3, tt_capacity=1024)
    slots = torch.arange(G, dtype=torch.int32, device="cuda")
    alive = eng.alive(slots=slots)
    V, moves = mcts.search(eng, slots, alive)
    assert mcts.tt.status() == (1024, 1024, 1)
    Vh = V.cpu().numpy().reshape(-1, 3)
    assert np.isfinite(Vh).all() and (np.abs(Vh) <= 1).all()
    n_none = int((~Vh.any(axis=1)).sum())
    print(f"{n_none} of {G * 4} root rows found no room in the table")
    assert n_none >= 1, "root rows without an entry read as none"
    assert (moves.cpu().numpy() <= 2).all()
    with pytest.raises(EngineError, match="overflow"):
        mcts.end_of_turn()
