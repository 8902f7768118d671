"""numpy reference of the top-k selection (csrc/k_topk.hip) and of the n-best enumeration (pf_host_nbest).

Order within a row y[0..V): entry a ranks before entry b when y[a] > y[b], or y[a] == y[b] and a > b (of equal values the
larger index first; -0.0 == +0.0).  NaN entries are never ranked.  n = min(K, non-NaN entries); slots r >= n hold id -1
and value -inf."""
import itertools

import numpy as np


def topk_row(y, K):
    """(ids [K] int64, val [K] float32, n) of one row."""
    y = np.asarray(y, np.float32)
    idx = np.flatnonzero(~np.isnan(y))
    v = y[idx]
    with np.errstate(invalid="ignore"):
        order = np.lexsort((-idx, -v))          # primary key -value ascending, then -index ascending
    pick = idx[order][:K]
    ids = np.full(K, -1, np.int64)
    val = np.full(K, -np.inf, np.float32)
    ids[:len(pick)] = pick
    val[:len(pick)] = y[pick]
    return ids, val, len(pick)


def topk_ref(x, K, V=None):
    """x [..., ld] -> ids [..., K] int64, val [..., K] float32, n [...] int32 over the first V entries of each row."""
    x = np.asarray(x, np.float32)
    V = x.shape[-1] if V is None else V
    rows = x.reshape(-1, x.shape[-1])
    ids = np.zeros((rows.shape[0], K), np.int64)
    val = np.zeros((rows.shape[0], K), np.float32)
    n = np.zeros(rows.shape[0], np.int32)
    for r in range(rows.shape[0]):
        ids[r], val[r], n[r] = topk_row(rows[r, :V], K)
    lead = x.shape[:-1]
    return ids.reshape(lead + (K,)), val.reshape(lead + (K,)), n.reshape(lead)


def hyp_score(val, ranks):
    """float64 sum of the float32 values val[l, ranks[l]], added sequentially from l = 0 up."""
    s = 0.0
    for l, r in enumerate(ranks):
        s = s + float(np.float32(val[l][r]))
    return s


def nbest_brute(val, n, n_free, N):
    """Every rank vector r with r[l] < n[l] and r[l] == 0 for l >= n_free, by descending score, ties to the
    lexicographically smaller vector; the first N as (ranks list of tuples, scores list of float)."""
    L = len(n)
    if any(int(k) == 0 for k in n):
        return [], []
    spans = [range(int(n[l])) if l < n_free else range(1) for l in range(L)]
    hyps = [(hyp_score(val, r), r) for r in itertools.product(*spans)]
    hyps.sort(key=lambda h: (-h[0], h[1]))
    hyps = hyps[:N]
    return [h[1] for h in hyps], [h[0] for h in hyps]
