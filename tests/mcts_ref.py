"""A NumPy model of the search's device side, one function per kernel entry point -- test infrastructure.

Written from the contract (include/snake_engine.h, the transposition cache and the rollout tick; the reference's
Agent / MCTSAgent: agent.py:25-223), not from csrc/mcts.hip.  Where the header fixes a float32 operation order the model
redoes it in np.float32 in that order (q = total / visit; est = (p0*q0 + p1*q1) + p2*q2; the sequential back-up's live
re-reads): the library is built without contraction or fast-math and with correctly rounded division, so those results
are comparable bit for bit.  Everything else (softermax, the cdf of a move choice, the Philox uniform) is float64.

Entries: the model does not know which slot a key lands in (that depends on which lane wins a race), only WHICH slots
end up occupied -- with linear probing from key_lo & mask and no deletions that set does not depend on insertion order.
The per-kernel models therefore take statistics as arrays total[n][3], visit[n][3] indexed by an entry number of the
caller's choosing; NONE marks a row without an entry.
"""
import numpy as np

NONE = 0xFFFFFFFF
F32 = np.float32
_M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- Philox4x32-10
# Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3" (SC'11), section 4: ten rounds of
#   (c0, c1, c2, c3) <- (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)),  key += (W0, W1) between rounds
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
DRAW_TAG = 0x4D435453       # counter word 3 of every search draw


def philox4x32_10(counter, key):
    """counter: four uint32 words (scalars or equal-length arrays), key: two.  Returns uint64 array [n][4] of 32-bit words."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & np.uint64(_M32) for w in counter]
    n = max(len(w) for w in c)
    c = [np.broadcast_to(w, (n,)).copy() for w in c]
    k0, k1 = int(key[0]) & _M32, int(key[1]) & _M32
    m32, sh = np.uint64(_M32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]          # 32 x 32 -> 64 bits: fits uint64
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return np.stack(c, axis=1)


def philox_uniform(rows, ctr0, ctr1, seed):
    """the uniform of row i: counter (i, ctr0, ctr1, 'MCTS'), key (seed low, seed high); u = (r0 * 2^32 + r1 + 0.5) / 2^64"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10((np.asarray(rows, dtype=np.uint64), ctr0, ctr1, DRAW_TAG), (seed & _M32, seed >> 32))
    return (r[:, 0].astype(np.float64) * 4294967296.0 + r[:, 1].astype(np.float64) + 0.5) / 18446744073709551616.0


def taped_uniform(tape, tape_base, rank, m, draws=None):
    """row i reads tape[tape_base + (rank[i] if rank is given else i)].  draws (optional mask): the rows that draw at all;
    theirs must lie inside the tape, the others (whose rank may be -1) get a placeholder nobody may use."""
    idx = tape_base + (np.arange(m) if rank is None else np.asarray(rank, dtype=np.int64))
    draws = np.ones(m, bool) if draws is None else np.asarray(draws) != 0
    assert ((idx[draws] >= 0) & (idx[draws] < len(tape))).all(), "a row that draws points outside the tape"
    return np.where(draws, np.asarray(tape, dtype=np.float64)[np.clip(idx, 0, len(tape) - 1)], np.nan)


# ---------------------------------------------------------------------------------------------- Agent.softermax / choice / argmaxs
def softermax3(base, z):
    """Agent.softermax (agent.py:114-122) on rows of 3, float64.  Two clamps the kernel documents: an all-zero row of
    powers (every z == -1) is the uniform pmf (the reference's own rule); a power of +inf (z == +1, where the reference
    divides inf by inf) shares the mass equally among the infinite cells."""
    z = np.asarray(z, dtype=np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        nrm = np.power(float(base), np.arctanh(z))
        inf = np.isinf(nrm)
        sigma = (nrm[:, 0] + nrm[:, 1]) + nrm[:, 2]
        pmf = nrm / sigma[:, None]
    pmf[sigma == 0.0] = 1.0 / 3.0
    has_inf = inf.any(axis=1)
    pmf[has_inf] = inf[has_inf] / inf[has_inf].sum(axis=1, keepdims=True)
    return pmf


def choice_cdf(pmf):
    """the cdf numpy.random.choice builds from p: float64 cumsum, divided by its last element"""
    cdf = np.cumsum(np.asarray(pmf).reshape(-1, 3).astype(np.float64), axis=1)
    return cdf / cdf[:, 2:3]


def choice3(pmf, u):
    """numpy.random.choice([0, 1, 2], p=pmf) given the uniform it would have drawn: cdf.searchsorted(u, side='right'),
    i.e. the number of cdf elements <= u (u < 1 = cdf[2], so the answer is 0, 1 or 2)"""
    cdf = choice_cdf(pmf)
    return (cdf <= np.asarray(u, dtype=np.float64).reshape(-1, 1)).sum(axis=1).astype(np.uint8)


def argmaxs(Z):
    """Agent.argmaxs (agent.py:124-137): strict comparisons, so ties fall to the later cell"""
    Z = np.asarray(Z).reshape(-1, 3)
    a, b, c = Z[:, 0], Z[:, 1], Z[:, 2]
    return np.where(a > b, np.where(a > c, 0, 2), np.where(b > c, 1, 2)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- the table
def canonical_key(lo, hi):
    """(0, 0) is no key; a single zero word is remapped to 1 (zero is the empty sentinel of both words)"""
    lo, hi = int(lo) & 0xFFFFFFFFFFFFFFFF, int(hi) & 0xFFFFFFFFFFFFFFFF
    if lo == 0 and hi == 0:
        return None
    return (lo or 1, hi or 1)


class TableModel:
    """cached_values / total_rewards / visit_cnts / cache_hit as one dict keyed by the canonical key pair.
    entries[key] = dict(total float32[3], visit float32[3], touch int); statistics of a new entry are NaN until
    set_priors gives them (the device leaves them undefined)."""

    def __init__(self, capacity):
        self.cap = int(capacity)
        self.entries = {}
        self.overflowed = 0
        self.lost = 0            # survivors a too-small rebuild had no slot for (which ones: not determined)

    def clear(self):
        self.entries, self.overflowed, self.lost = {}, 0, 0

    def occupied(self):
        return len(self.entries)

    def exists(self, key, now, max_age):
        e = self.entries.get(key)
        return e is not None and now - e["touch"] <= max_age + 1

    def lookup(self, keys, active, now, max_age):
        """find-or-insert one launch of rows.  Returns (row_key, new_keys): the canonical key of every row that has an entry
        afterwards (None: (0,0), inactive, or no room) and the set of keys exactly one of whose rows reports is_new."""
        rows = [canonical_key(lo, hi) if (active is None or active[i]) else None for i, (lo, hi) in enumerate(keys)]
        absent = {k for k in rows if k is not None and k not in self.entries}
        free = self.cap - len(self.entries)
        if len(absent) > free:
            if free:
                raise NotImplementedError("which of the new keys get the last free slots depends on the race")
            self.overflowed = 1
        new = set()
        for k in dict.fromkeys(rows):
            if k is None:
                continue
            e = self.entries.get(k)
            if e is None:
                if len(self.entries) < self.cap:
                    self.entries[k] = dict(total=np.full(3, np.nan, F32), visit=np.full(3, np.nan, F32), touch=now)
                    new.add(k)
            else:
                if now - e["touch"] > max_age + 1:      # evicted in the reference: re-created in place, statistics await priors
                    new.add(k)
                e["touch"] = now
        return [k if k in self.entries else None for k in rows], new

    def find(self, keys, now, max_age):
        """read-only probe: (row_key or None, stat7 float32 [m][7] = total, visit, age; zeros where none)"""
        out, stat = [], np.zeros((len(keys), 7), F32)
        for i, (lo, hi) in enumerate(keys):
            k = canonical_key(lo, hi)
            if k is not None and self.exists(k, now, max_age):
                e = self.entries[k]
                stat[i, 0:3], stat[i, 3:6], stat[i, 6] = e["total"], e["visit"], F32(now - e["touch"])
                out.append(k)
            else:
                out.append(None)
        return out, stat

    def set_priors(self, row_keys, q):
        q = np.asarray(q, F32).reshape(-1, 3)
        for k, qk in zip(row_keys, q):
            if k is not None:
                self.entries[k]["total"] = qk.copy()
                self.entries[k]["visit"] = np.ones(3, F32)

    def rebuild(self, new_capacity, now, max_age):
        """end-of-turn eviction: keeps entries with now - touch <= max_age, statistics and touch turns unchanged"""
        keep = {k: e for k, e in self.entries.items() if now - e["touch"] <= max_age}
        self.cap, self.overflowed, self.lost = int(new_capacity), 0, 0
        if len(keep) > self.cap:
            self.overflowed, self.lost = 1, len(keep) - self.cap
        self.entries = keep

    def occupied_after_rebuild(self):
        return len(self.entries) - self.lost

    def slot_set(self):
        """the occupied slots under linear probing from key_lo & mask (independent of insertion order)"""
        assert len(self.entries) <= self.cap
        used, mask = set(), self.cap - 1
        for lo, _ in self.entries:
            s = lo & mask
            while s in used:
                s = (s + 1) & mask
            used.add(s)
        return used


# ---------------------------------------------------------------------------------------------- rollout tick
def q_of(total, visit, entry):
    """q = total / visit in float32 for the rows that have an entry (zeros elsewhere); returns (q [m][3], has_entry [m])"""
    entry = np.asarray(entry, dtype=np.int64) & NONE
    ok = entry != NONE
    q = np.zeros((len(entry), 3), F32)
    e = entry[ok]
    q[ok] = np.asarray(total, F32)[e] / np.asarray(visit, F32)[e]
    return q, ok


read_q = q_of       # snk_tt_read_q: none rows give three zeros, the rest the float32 division


def est_of(pmf, q):
    """est = (p0*q0 + p1*q1) + p2*q2, float32, in this order"""
    pmf, q = np.asarray(pmf, F32), np.asarray(q, F32)
    return (pmf[:, 0] * q[:, 0] + pmf[:, 1] * q[:, 1]) + pmf[:, 2] * q[:, 2]


def select_moves(pmf, u, has_entry):
    """move ~ pmf given the row's uniform; a row without an entry moves 1 (straight on)"""
    return np.where(has_entry, choice3(pmf, u), 1).astype(np.uint8)


def select_append(entry, moves, path_entry, path_move, path_len, D):
    """(entry, move) is appended at path[len] where the row has an entry and len < D; len itself is left alone"""
    pe, pm = np.array(path_entry, copy=True).reshape(-1, D), np.array(path_move, copy=True).reshape(-1, D)
    entry = np.asarray(entry, dtype=np.int64) & NONE
    for i in range(len(entry)):
        L = int(path_len[i])
        if entry[i] != NONE and L < D:
            pe[i, L], pm[i, L] = entry[i], moves[i]
    return pe, pm


def _exact_f32(acc):
    out = acc.astype(F32)
    if not np.array_equal(out.astype(np.float64), acc):
        raise ValueError("the order-free back-up model needs sums that float32 holds exactly")
    return out


def backup_production(total, visit, entry, est, path_entry, path_move, path_len, D):
    """one thread per row, float atomics: every ancestor edge gets visit += 1, total += est[row]; len advances by one
    where len < D.  The order of the additions is not determined, so the model only accepts inputs whose sums are exact."""
    entry = np.asarray(entry, dtype=np.int64) & NONE
    tot, vis = np.asarray(total, F32).astype(np.float64), np.asarray(visit, F32).astype(np.float64)
    pe, pm = np.asarray(path_entry).reshape(-1, D), np.asarray(path_move).reshape(-1, D)
    new_len = np.array(path_len, dtype=np.int32, copy=True)
    for i in range(len(entry)):
        if entry[i] == NONE:
            continue
        L = int(path_len[i])
        for j in range(L):
            tot[int(pe[i, j]), int(pm[i, j])] += float(est[i])
            vis[int(pe[i, j]), int(pm[i, j])] += 1.0
        if L < D:
            new_len[i] = L + 1
    return _exact_f32(tot), _exact_f32(vis), new_len


def backup_sequential(total, visit, entry, pmf, path_entry, path_move, path_len, D):
    """the reference's order (agent.py:208-220): rows ascending; est from the row's entry as it stands NOW (earlier rows
    of this launch included); the path walked from its end; float32 throughout"""
    entry = np.asarray(entry, dtype=np.int64) & NONE
    tot, vis = np.array(total, dtype=F32, copy=True), np.array(visit, dtype=F32, copy=True)
    pmf = np.asarray(pmf, F32).reshape(-1, 3)
    pe, pm = np.asarray(path_entry).reshape(-1, D), np.asarray(path_move).reshape(-1, D)
    new_len = np.array(path_len, dtype=np.int32, copy=True)
    for i in range(len(entry)):
        if entry[i] == NONE:
            continue
        e = int(entry[i])
        q = tot[e] / vis[e]
        r = F32(F32(F32(pmf[i, 0] * q[0]) + F32(pmf[i, 1] * q[1])) + F32(pmf[i, 2] * q[2]))
        L = int(path_len[i])
        for j in range(L - 1, -1, -1):
            a, mv = int(pe[i, j]), int(pm[i, j])
            vis[a, mv] = F32(vis[a, mv] + F32(1.0))
            tot[a, mv] = F32(tot[a, mv] + r)
        if L < D:
            new_len[i] = L + 1
    return tot, vis, new_len


def terminal_backup(total, visit, rewards, path_entry, path_move, path_len, D, sequential):
    """agent.py:60-72: rows with reward +1 / -1 add it (and one visit) along their whole path; 0 = None adds nothing"""
    tot, vis = np.array(total, dtype=F32, copy=True), np.array(visit, dtype=F32, copy=True)
    pe, pm = np.asarray(path_entry).reshape(-1, D), np.asarray(path_move).reshape(-1, D)
    if not sequential:
        tot, vis = tot.astype(np.float64), vis.astype(np.float64)
    for i in range(len(rewards)):
        if not rewards[i]:
            continue
        for j in range(int(path_len[i]) - 1, -1, -1):
            a, mv = int(pe[i, j]), int(pm[i, j])
            vis[a, mv] = vis[a, mv] + tot.dtype.type(1.0)
            tot[a, mv] = tot[a, mv] + tot.dtype.type(rewards[i])
    return (tot, vis) if sequential else (_exact_f32(tot), _exact_f32(vis))


def retire(sub_active, done, sub_depth, tick, sim_steps):
    """the sub-games that moved are counted, then one retires iff it was active and (done or tick >= its depth cap)"""
    act = np.asarray(sub_active) != 0
    out = act & ~((np.asarray(done) != 0) | (tick >= np.asarray(sub_depth)))
    return out.astype(np.uint8), int(sim_steps) + int(act.sum())


def root_moves_play(V, alive):
    return np.where(np.asarray(alive) != 0, argmaxs(V), 1).astype(np.uint8)


def root_moves_training(pmf, u, alive):
    return np.where(np.asarray(alive) != 0, choice3(pmf, u), 1).astype(np.uint8)
