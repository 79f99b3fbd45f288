"""numpy restatement of the fp32 top-k contract (oracle/oracle.c oracle_topk / oracle_inv_norms with fp32 inputs where the oracle
converts fp16 to fp32).  Every operation is a separate fp32 numpy ufunc (multiply, then add: no fma), the sums run column by column
in element order, so each row's chain is the oracle's sequential chain.

    inv[i]   = (float)(1.0 / (double)sqrtf(s)),  s = s + v * v over the row in order; 0 when s is not > 0
    qn[j]    = q[j] * qinv   when qinv != 0
    xn[c][j] = x[c][j] * pinv[c]   when pinv[c] != 0
    score    = s + qn[j] * xn[c][j] over j in order
    order    = (score desc, id asc); missing results are (-inf, -1)
"""
import numpy as np


def inv_norms(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    xt = np.ascontiguousarray(x.T)                       # [dim][n]: a column of the sum is one contiguous row
    s = np.zeros(x.shape[0], dtype=np.float32)
    tmp = np.empty_like(s)
    for j in range(x.shape[1]):
        np.multiply(xt[j], xt[j], out=tmp)
        np.add(s, tmp, out=s)
    inv = np.zeros(x.shape[0], dtype=np.float32)
    pos = s > 0
    inv[pos] = (1.0 / np.sqrt(s[pos]).astype(np.float64)).astype(np.float32)      # np.sqrt of fp32 is the correctly rounded sqrtf
    return inv


def normalised(x):
    """rows scaled by their inverse norms and rounded to fp32; rows with inverse norm 0 untouched"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    inv = inv_norms(x)
    out = x * inv[:, None]
    out[inv == 0] = x[inv == 0]
    return out


def scores(pool, queries, qblock=32):
    """fp32 [nq][n]: the contract's score of every (query, row) pair.  Blocks of queries run on a few threads (the ufuncs release
    the GIL); every pair's chain is the same whichever thread adds it."""
    from concurrent.futures import ThreadPoolExecutor
    pt = np.ascontiguousarray(normalised(pool).T)        # [dim][n]
    qn = normalised(queries)
    nq, n, dim = qn.shape[0], pt.shape[1], pt.shape[0]
    out = np.empty((nq, n), dtype=np.float32)

    def block(lo):
        q = qn[lo:lo + qblock]
        s = np.zeros((q.shape[0], n), dtype=np.float32)
        tmp = np.empty_like(s)
        for j in range(dim):
            np.multiply(q[:, j:j + 1], pt[j][None, :], out=tmp)
            np.add(s, tmp, out=s)
        out[lo:lo + qblock] = s

    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(block, range(0, nq, qblock)))
    return out


def topk(pool, ids, queries, k):
    """-> (scores fp32 [nq][k], ids int64 [nq][k]) by (score desc, id asc), padded with (-inf, -1)"""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    sc = scores(pool, queries)
    nq, n = sc.shape
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    kk = min(k, n)
    for q in range(nq):
        row = sc[q]
        if n > 4 * k:                                    # only rows that reach the k-th best value can be in the answer
            kth = np.partition(row, n - kk)[n - kk]
            keep = np.nonzero(row >= kth)[0]
        else:
            keep = np.arange(n)
        order = np.lexsort((ids[keep], -row[keep]))[:kk]
        out_s[q, :kk] = row[keep][order]
        out_i[q, :kk] = ids[keep][order]
    return out_s, out_i
