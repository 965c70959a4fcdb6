"""CPU checker of the random walks (grx_rw_*), in two independent forms of the definition in include/gunrock/gunrock_mi355x.h:

scalar(...)      the definition transcribed into plain Python integers: one walk after the other, one step after the other, its own
                 splitmix64, the 128-bit product as a Python product, the row and the membership bisections as loops.
vectorised(...)  numpy, one step for all walkers at once: the draws from ga.rw_draw, the 128-bit product in 32-bit halves, the weighted
                 choice as one searchsorted over the running sum of ALL sorted weights, membership as one searchsorted over
                 (row * n + column) keys.

Both return {"walks", "lengths", "visits", "steps", "ended_early", "biased_tries", "forced_fallbacks"}.  Not a test module."""
import numpy as np

import gunrockinst_amd as ga

M64 = (1 << 64) - 1


# ---------------- graphs ----------------

def csr(n, rows, cols, weights=None):
    """CSR of the arcs in the order given within a row (stable); weights travel along"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    ro = np.zeros(n + 1, dtype=np.int32)
    ro[1:] = np.cumsum(np.bincount(rows, minlength=n))
    w = None if weights is None else np.asarray(weights)[order].astype(np.int32)
    return n, ro, cols[order].astype(np.int32), w


def symmetric(n, pairs):
    a = np.array([p[0] for p in pairs], dtype=np.int64)
    b = np.array([p[1] for p in pairs], dtype=np.int64)
    return csr(n, np.concatenate([a, b]), np.concatenate([b, a]))[:3]


def path(n):
    return symmetric(n, [(i, i + 1) for i in range(n - 1)])


def star(n):
    return symmetric(n, [(0, i) for i in range(1, n)])


def complete(n):
    return symmetric(n, [(i, j) for i in range(n) for j in range(i + 1, n)])


def directed_cycle(n):
    return csr(n, np.arange(n), (np.arange(n) + 1) % n)[:3]


def directed_path(n):
    return csr(n, np.arange(n - 1), np.arange(1, n))[:3]


def cycle_with_tail(c, t):
    """a directed cycle of c vertices; from vertex 0 also a tail of t vertices into a sink"""
    rows = list(range(c)) + [0] + list(range(c, c + t - 1))
    cols = [(i + 1) % c for i in range(c)] + [c] + list(range(c + 1, c + t))
    return csr(c + t, rows, cols)[:3]


def gnp(n, p, seed, directed=True):
    rng = np.random.default_rng(seed)
    a = rng.random((n, n)) < p
    if not directed:
        a = np.triu(a, 1)
        a = a | a.T
    rows, cols = np.nonzero(a)
    return csr(n, rows, cols)[:3]


def row_col_weights(ro, ci, mod=7):
    """the (row + col) % mod + 1 weights"""
    rows = np.repeat(np.arange(ro.shape[0] - 1, dtype=np.int64), np.diff(ro))
    return ((rows + ci) % mod + 1).astype(np.int32)


def shuffled_rows(ro, ci, w, rng):
    """the entries permuted within every row, the weights carried along"""
    rows = np.repeat(np.arange(ro.shape[0] - 1, dtype=np.int64), np.diff(ro))
    order = np.lexsort((rng.random(ci.shape[0]), rows))
    return ci[order], None if w is None else w[order]


def sorted_copy(n, ro, ci, w):
    """every row sorted by (column, weight); the inclusive prefix of the weights per row"""
    ro = np.asarray(ro, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ro))
    wt = np.zeros(ci.shape[0], dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    order = np.lexsort((wt, ci, rows))
    return ro, ci[order], wt[order]


# ---------------- the scalar form ----------------

def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw(seed, walk, step, t):
    return mix(seed ^ mix((walk << 32) | (step << 8) | t))


def scalar(n, ro, ci, starts, length, weights=None, seed=0, bias=(1, 1, 1), tries=32):
    ro, sci, sw = sorted_copy(n, ro, ci, weights)
    ro, sci, sw = [int(x) for x in ro], [int(x) for x in sci], [int(x) for x in sw]
    prefix = [0] * len(sci)
    for v in range(n):
        run = 0
        for i in range(ro[v], ro[v + 1]):
            run += sw[i]
            prefix[i] = run
    weighted = weights is not None
    b_return, b_in, b_out = (int(b) for b in bias)
    biased = not (b_return == b_in == b_out)
    amax = max(b_return, b_in, b_out)

    def choose(v, r):
        b, d = ro[v], ro[v + 1] - ro[v]
        if d == 0:
            return None
        if not weighted:
            return sci[b + (((r >> 32) * d) >> 32)]
        total = prefix[b + d - 1]
        if total == 0:
            return None
        t = (r * total) >> 64
        lo, hi = 0, d - 1
        while lo < hi:
            mid = (lo + hi) // 2
            if prefix[b + mid] > t:
                hi = mid
            else:
                lo = mid + 1
        return sci[b + lo]

    def holds(p, x):
        lo, hi = ro[p], ro[p + 1]
        while lo < hi:
            mid = (lo + hi) // 2
            if sci[mid] < x:
                lo = mid + 1
            else:
                hi = mid
        return lo < ro[p + 1] and sci[lo] == x

    walks = np.full((len(starts), length + 1), -1, dtype=np.int32)
    lengths = np.zeros(len(starts), dtype=np.int32)
    total_tries = forced = 0
    for w, start in enumerate(starts):
        v, p = int(start), None
        walks[w, 0] = v
        count = 1
        for s in range(length):
            if not biased or s == 0:
                x = choose(v, draw(seed, w, s, 0))
            else:
                x = None
                for j in range(tries):
                    x = choose(v, draw(seed, w, s, 2 * j))
                    if x is None:
                        break
                    total_tries += 1
                    b = b_return if x == p else b_in if holds(p, x) else b_out
                    if (((draw(seed, w, s, 2 * j + 1) >> 32) * amax) >> 32) < b:
                        break
                else:
                    forced += 1
            if x is None:
                break
            walks[w, s + 1] = x
            count += 1
            p, v = v, x
        lengths[w] = count
    return _result(n, walks, lengths, total_tries, forced, length)


def _result(n, walks, lengths, tries, forced, length):
    return {"walks": walks, "lengths": lengths, "visits": np.bincount(walks[walks >= 0], minlength=n).astype(np.int64),
            "steps": int(lengths.astype(np.int64).sum() - lengths.shape[0]), "ended_early": int((lengths <= length).sum()),
            "biased_tries": int(tries), "forced_fallbacks": int(forced)}


# ---------------- the vectorised form ----------------

def mulhi(a, b):
    """the high 64 bits of a * b, uint64 arrays, in 32-bit halves"""
    lo32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    a0, a1, b0, b1 = a & lo32, a >> s32, b & lo32, b >> s32
    m1, m2 = a1 * b0, a0 * b1
    carry = (((a0 * b0) >> s32) + (m1 & lo32) + (m2 & lo32)) >> s32
    return a1 * b1 + (m1 >> s32) + (m2 >> s32) + carry


def vectorised(n, ro, ci, starts, length, weights=None, seed=0, bias=(1, 1, 1), tries=32):
    ro, sci, sw = sorted_copy(n, ro, ci, weights)
    weighted = weights is not None
    running = np.cumsum(sw).astype(np.uint64)  # over all sorted entries
    before = np.concatenate([[0], running])[ro[:-1]].astype(np.uint64)  # the running sum in front of a row
    after = np.concatenate([[0], running])[ro[1:]].astype(np.uint64)
    deg = np.diff(ro)
    can_leave = (after > before) if weighted else (deg > 0)
    keys = np.repeat(np.arange(n, dtype=np.int64), deg) * n + sci  # ascending: the rows are sorted
    b_return, b_in, b_out = (int(b) for b in bias)
    biased = not (b_return == b_in == b_out)
    amax = np.uint64(max(b_return, b_in, b_out))
    starts = np.asarray(starts, dtype=np.int64)
    count = starts.shape[0]
    ids = np.arange(count, dtype=np.uint64)

    def choose(v, r):
        """the choice at the vertices v (all can be left) with the draws r"""
        if not weighted:
            return sci[ro[v] + ((r >> np.uint64(32)) * deg[v].astype(np.uint64) >> np.uint64(32)).astype(np.int64)]
        t = mulhi(r, after[v] - before[v])
        return sci[np.searchsorted(running, before[v] + t, side="right")]

    walks = np.full((count, length + 1), -1, dtype=np.int32)
    walks[:, 0] = starts
    v = starts.copy()
    p = np.full(count, -1, dtype=np.int64)
    alive = np.ones(count, dtype=bool)
    total_tries = forced = 0
    for s in range(length):
        alive &= can_leave[np.where(alive, v, 0)]
        at = np.nonzero(alive)[0]
        if at.shape[0] == 0:
            break
        x = choose(v[at], ga.rw_draw(seed, ids[at], s, 0))
        if biased and s > 0:
            pending = np.ones(at.shape[0], dtype=bool)
            for j in range(tries):
                sel = np.nonzero(pending)[0]
                if sel.shape[0] == 0:
                    break
                w = at[sel]
                if j:
                    x[sel] = choose(v[w], ga.rw_draw(seed, ids[w], s, 2 * j))
                total_tries += sel.shape[0]
                q = p[w] * n + x[sel]
                pos = np.minimum(np.searchsorted(keys, q), keys.shape[0] - 1)
                b = np.where(x[sel] == p[w], b_return, np.where(keys[pos] == q, b_in, b_out)).astype(np.uint64)
                a = ((ga.rw_draw(seed, ids[w], s, 2 * j + 1) >> np.uint64(32)) * amax) >> np.uint64(32)
                pending[sel[a < b]] = False
            forced += int(pending.sum())
        walks[at, s + 1] = x
        p[at] = v[at]
        v[at] = x
    lengths = (walks >= 0).sum(axis=1).astype(np.int32)
    return _result(n, walks, lengths, total_tries, forced, length)
