"""The numpy restatement of robust_csrc/rt_robust.h, operation by operation in f32, and the bucket corpora that the
CPU test (tests/test_robust_host.py) and the GPU test (tests/test_gpu_robust.py) share.  The order of the buckets is taken from
integer keys (uint64) by rank counting: no float is ever sorted.  Plain numpy, no GPU."""
import numpy as np

import _extreme_planes as xp

f32 = np.float32
BUCKET_COUNTS = (3, 5, 7, 9, 11, 13, 15)
GINI, TRIM = 0, 1


def counts(K, e):
    """e samples over K buckets: e div K + (k < e mod K)."""
    return [e // K + (1 if k < e % K else 0) for k in range(K)]


def sample_counts(K):
    """The three counts of the tests: every bucket one sample, one bucket two, and ragged."""
    return (K, K + 1, 4 * K + 3)


def widths(K):
    """(mode, c) of the tests: "gini", and "trim" with c in {0, 1, h}."""
    h = (K - 1) // 2
    return [(GINI, 0)] + [(TRIM, c) for c in sorted({0, 1, h})]


def fold(buckets, records, first):
    """buckets (K, P, 3) += records (P, n, 3) in place, record j to bucket (first + j) mod K, in ascending j."""
    K = buckets.shape[0]
    for j in range(records.shape[1]):
        k = (first + j) % K
        buckets[k] = (buckets[k] + records[:, j]).astype(f32)


def keys(y):
    u = np.ascontiguousarray(y, f32).view(np.uint32).astype(np.uint64)
    k = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return np.where(np.isnan(y), np.uint64(0xFFFFFFFF), k)


def ranks(key):
    """key (K, N) -> rank (K, N): the buckets that precede k, ties by k."""
    K = key.shape[0]
    rank = np.zeros(key.shape, np.int32)
    for k in range(K):
        for j in range(K):
            if j < k:
                rank[k] += key[j] <= key[k]
            elif j > k:
                rank[k] += key[j] < key[k]
    return rank


def resolve(B, e, mode=GINI, c=0):
    """B (K, N, 3) f32 at the count e -> dict(linear (N, 3), gini, kept int32, variance (N,), accum (N, 3), moments (N, 2))."""
    B = np.asarray(B, f32)
    K, N = B.shape[:2]
    assert K in BUCKET_COUNTS and e >= K
    h = (K - 1) // 2
    K_f, e_f, zero = f32(K), f32(e), f32(0)
    with np.errstate(all="ignore"):
        m = np.stack([B[k] / f32(n) for k, n in enumerate(counts(K, e))])
        y = (m[..., 0] + m[..., 1]) + m[..., 2]
        rank = ranks(keys(y))
        assert (np.sort(rank, 0) == np.arange(K, dtype=np.int32)[:, None]).all()          # a permutation, whatever B holds
        T, g = np.zeros(N, f32), np.zeros(N, f32)
        for k in range(K):
            ys = np.where(y[k] > 0, y[k], zero)
            T = T + ys
            g = g + (2 * rank[k] - (K - 1)).astype(f32) * ys
        G = np.where(T > 0, g / (K_f * T), zero)
        G = np.where(G > 0, G, zero)
        G = np.where(G < 1, G, f32(1))
        if mode == GINI:
            cw = np.floor((f32(1) - G) * f32(h)).astype(np.int32)
        else:
            cw = np.full(N, c, np.int32)
        assert (cw >= 0).all() and (cw <= h).all()
        s = np.zeros((N, 3), f32)
        for k in range(K):
            kept = (h - cw <= rank[k]) & (rank[k] <= h + cw)
            s = np.where(kept[:, None], s + m[k], s)
        r = s / (2 * cw + 1).astype(f32)[:, None]
        c1 = np.maximum(cw, 1)
        lo, hi = np.zeros(N, f32), np.zeros(N, f32)
        for k in range(K):
            lo = np.where(rank[k] == h - c1, y[k], lo)
            hi = np.where(rank[k] == h + c1, y[k], hi)
        w = [np.where(y[k] < lo, lo, np.where(y[k] < hi, y[k], hi)) for k in range(K)]
        sw = np.zeros(N, f32)
        for k in range(K):
            sw = sw + w[k]
        mw = sw / K_f
        dw = np.zeros(N, f32)
        for k in range(K):
            d = w[k] - mw
            dw = dw + d * d
        v = (dw / (K_f - f32(1))) / K_f
        yr = (r[:, 0] + r[:, 1]) + r[:, 2]
        out = dict(linear=r, gini=G, kept=(2 * cw + 1).astype(np.int32), variance=v, accum=r * e_f,
                   moments=np.stack([yr * e_f, (v * (e_f - f32(1)) + yr * yr) * e_f], -1))
    for a in out.values():
        assert a.dtype in (np.float32, np.int32)
    return {n: np.ascontiguousarray(a) for n, a in out.items()}


OUTPUTS = ("linear", "gini", "kept", "variance", "accum", "moments")


# ---- the corpora -----------------------------------------------------------------------------------------------------------------------
def records(seed, P, n):
    """(P, n, 3) sample colours: mostly moderate, one in 16 a firefly, a few exactly zero."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 1.5, (P, n, 3)).astype(f32)
    a[rng.random((P, n)) < 1 / 16] *= f32(300)
    a[rng.random((P, n)) < 1 / 32] = 0
    return a


def corpus(K, e, N, seed=0):
    """(B (K, N, 3), {name: slice of pixels}): random positive sums; ties (two equal buckets, all equal, all zero); a planted outlier;
    negative sums; and the extreme tier of tests/_extreme_planes.py: each of its small, huge and non-finite values in one bucket of a
    pixel and in every bucket of a pixel, then salted stretches of each class."""
    rng = np.random.default_rng([4290, K, e, seed])
    n = np.array(counts(K, e), f32)[:, None, None]
    B = (rng.uniform(0.05, 2.0, (K, N, 3)).astype(f32) * n).astype(f32)
    parts, at = {}, [0]

    def take(name, count):
        s = slice(at[0], at[0] + count)
        assert s.stop <= N, (name, N)
        parts[name] = s
        at[0] = s.stop
        return s

    s = take("two equal", 8)
    B[1, s] = B[K - 1, s] * (n[1] / n[K - 1])                       # (equal sums where the counts are: equal means or nearly)
    B[0, s.start:s.start + 4] = B[2, s.start:s.start + 4]
    s = take("all equal", 4)
    B[:, s] = B[0, s]
    s = take("all zero", 4)
    B[:, s] = 0
    B[K // 2, s.start + 2:s.stop] = -0.0
    s = take("outlier", 12)
    B[np.arange(12) % K, np.arange(s.start, s.stop)] *= f32(1000)
    s = take("negative", 8)
    B[:, s] *= rng.choice(np.array([-1, 1], f32), (K, 8, 1))
    B[:, s.start:s.start + 2] = -np.abs(B[:, s.start:s.start + 2])
    specials = np.concatenate([xp.SMALL, xp.HUGE, xp.NONFINITE])
    s = take("one bucket", len(specials))
    for j, v in enumerate(specials):
        B.view(np.uint32)[j % K, s.start + j, j % 3] = v.view(np.uint32)
    s = take("every bucket", len(specials))
    for j, v in enumerate(specials):
        B.view(np.uint32)[:, s.start + j, :] = v.view(np.uint32)
    s = take("two nan", 4)
    B[0, s, 0] = np.nan
    B[K - 1, s, 2] = -np.nan
    for name, vals, share in (("small", xp.SMALL, 0.5), ("huge", xp.HUGE, 0.15), ("nonfinite", xp.NONFINITE, 0.05)):
        s = take("salted " + name, 48)
        B[:, s] = xp.salted(B[:, s], vals, share, rng)
    take("random", N - at[0])
    return B, parts


def property_buckets(K, e, factor, N=None):
    """Pixels whose clean buckets hold sums that make every mean exactly (0.25, 0.25, 0.25), bucket p mod K of pixel p times `factor`."""
    N = K if N is None else N
    n = np.array(counts(K, e), f32)[:, None, None]
    B = np.broadcast_to(f32(0.25) * n, (K, N, 3)).astype(f32)
    B[np.arange(N) % K, np.arange(N)] *= f32(factor)
    return B
