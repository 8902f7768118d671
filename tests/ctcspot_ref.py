"""The definition of CTC phrase spotting (include/paraformer_hip.h "CTC phrase spotting") in plain numpy, float64 by default, and
the case table the CPU and GPU tests share.  No import from the package.  On GRID inputs (on_grid) float64 and float32 agree
exactly, so the float32 twin and kernel must equal it bit for bit; dtype=np.float32 restates the arithmetic off the grid."""
import numpy as np

P = 16                                    # the kernel's ring depth (kSpotRing): T = P - 1, P, P + 1 are in the table
GRID = 64.0


def spot(lp, y, thr, max_hits, dtype=np.float64):
    """-> (n_hits, begin_end [max_hits, 2] int32, score [max_hits] float32), slots at and beyond n_hits (-1, -1, 0)"""
    f = dtype
    lp = np.asarray(lp)
    T, U = lp.shape[0], len(y)
    S = 2 * U - 1
    lab = [y[s // 2] if s % 2 == 0 else 0 for s in range(S)]
    v, st = np.full(S, -np.inf, f), np.full(S, -1, np.int64)
    hits, cur = [], None                                                       # cur = (begin, end, e, dur)
    for t in range(T):
        nv, nst = v.copy(), st.copy()
        for s in range(S):
            x = f(lp[t, lab[s]])
            if s == 0:
                nv[0], nst[0] = x, t
                continue
            best, src = v[s], st[s]
            if v[s - 1] > best:
                best, src = v[s - 1], st[s - 1]
            if s % 2 == 0 and y[s // 2] != y[s // 2 - 1] and v[s - 2] > best:
                best, src = v[s - 2], st[s - 2]
            nv[s], nst[s] = f(x + best), src
        v, st = nv, nst
        e, begin = v[S - 1], int(st[S - 1])
        dur = t - begin + 1
        if not (e > -np.inf and e >= f(f(thr) * f(dur))):
            continue
        if cur is None or begin > cur[1]:
            if cur is not None:
                hits.append(cur)
            cur = (begin, t, e, dur)
        elif f(e * f(cur[3])) > f(cur[2] * f(dur)):
            cur = (begin, t, e, dur)
    if cur is not None:
        hits.append(cur)
    be, sc = np.full((max_hits, 2), -1, np.int32), np.zeros(max_hits, np.float32)
    for i, h in enumerate(hits[:max_hits]):
        be[i], sc[i] = (h[0], h[1]), np.float32(h[2])
    return len(hits), be, sc


def on_grid(lp, thr):
    """every value a multiple of 1/64, and T * T * max|value| * 64 < 2^24: sums and the products with a duration are exact"""
    a = np.asarray(lp, np.float64)
    T = max(a.shape[0], 1)
    return bool(np.all(a * GRID == np.round(a * GRID))) and thr * GRID == round(thr * GRID) and \
        T <= 64 and T * T * max(float(np.abs(a).max(initial=0.0)), abs(thr)) * GRID < 2 ** 24


def grid_rows(rng, T, V):
    return (-rng.integers(0, 8 * 64, size=(T, V)) / GRID).astype(np.float32)


def planted(T, V, cells):
    lp = np.full((T, V), -8.0, np.float32)
    for t, c, x in cells:
        lp[t, c] = x
    return lp


def _cases():
    """(tag, lp [T, V], phrases, thr, max_hits, expected n_hits per phrase or None)"""
    rng = np.random.default_rng(23)
    mix = [[3], [3, 3], [3, 4], [2, 3, 4]]
    long32 = [int(v) for v in rng.integers(1, 40, size=32)]
    a20 = [int(v) for v in rng.integers(1, 40, size=20)]
    b20 = [a20[-1]] + [int(v) for v in rng.integers(1, 40, size=19)]
    out = [
        ("U=1, K=1", grid_rows(rng, 9, 6), [[3]], -4.0, 4, None),
        ("U=2 repeated: through the blank", planted(12, 6, [(2, 3, 0), (3, 0, -0.5), (4, 3, 0), (8, 3, 0), (9, 3, 0)]), [[3, 3]], -1.0, 4, [1]),
        ("U=2 distinct: the skip", planted(12, 6, [(2, 3, 0), (3, 4, 0)]), [[3, 4]], -1.0, 4, [1]),
        ("U=32, S=63", grid_rows(rng, 64, 40), [long32], -8.0, 8, None),
        ("S=63 and S=1 share a row", grid_rows(rng, 40, 40), [long32, [long32[-1]]], -8.0, 8, None),
        ("two chains of S=39 on two rows", grid_rows(rng, 30, 40), [a20, b20], -8.0, 8, None),
        ("70 phrases, six rows, two workgroups", grid_rows(rng, P + 1, 9),
         [[int(v) for v in rng.integers(1, 9, size=3)] for _ in range(70)], -5.0, 3, None),
        ("two occurrences", planted(12, 6, [(2, 3, 0), (3, 4, 0), (7, 3, 0), (8, 4, 0)]), [[3, 4]], -1.0, 4, [2]),
        ("three overlapping candidates: the best", planted(12, 6, [(2, 3, 0), (3, 4, -0.5), (4, 4, 0), (5, 4, -1.0)]), [[3, 4]], -1.0, 4, [1]),
        ("an exact tie keeps the earlier", planted(12, 6, [(2, 3, 0), (3, 4, -0.5), (4, 4, -0.25)]), [[3, 4]], -1.0, 4, [1]),
        ("at the threshold, and one step below",
         planted(12, 6, [(2, 3, -1.0), (3, 4, -1.0), (7, 3, -1.0), (8, 4, -1.0 - 1 / GRID)]), [[3, 4]], -1.0, 4, [1]),
        ("more hits than max_hits", planted(10, 6, [(t, 3, 0) for t in (0, 2, 4, 6, 8)]), [[3]], -1.0, 2, [5]),
    ]
    for T in (1, P - 1, P, P + 1):
        out.append(("T=%d" % T, grid_rows(rng, T, 6), mix, -6.0, 3, None))
    return out


CASES = _cases()
