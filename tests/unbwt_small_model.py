"""NumPy model of banzai_amd/csrc/unbwt_small.hip: the inverse BWT of one small block, phase by phase as the workgroup does it --
a byte histogram per wavefront over its eighth of the column, the exclusive bases over (byte, wavefront), the stable LF^-1
permutation T ranked 64 positions a step, the walk X[i] = T^i(ptr) by pointer doubling with T^m squared in place, and
S[i] = L[X[i + 1]].  Indices are 16 bits wide, as in the kernel, and X is stored from X[1] on."""
import numpy as np

SMALL_MAX = 8192
WAVES = 8
IDX = np.uint16


def build_T(col):
    """the rank phase: T[base[L[i]]++] = i, stable, by wavefront segments and steps of 64 lanes"""
    L = np.frombuffer(bytes(col), dtype=np.uint8)
    n = L.size
    seg = (n + 64 * WAVES - 1) // (64 * WAVES) * 64
    cur = np.zeros((WAVES, 256), dtype=np.uint32)
    bounds = [(w * seg, min(n, w * seg + seg)) for w in range(WAVES)]
    for w, (lo, hi) in enumerate(bounds):  # count
        if lo < hi:
            cur[w] = np.bincount(L[lo:hi], minlength=256)
    flat = cur.T.reshape(-1)               # bases: bytes first, the wavefronts inside a byte
    starts = np.cumsum(flat, dtype=np.uint32) - flat
    assert int(flat.sum()) == n
    cur = starts.reshape(256, WAVES).T.copy()
    P = np.zeros(n, dtype=IDX)
    for w, (lo, hi) in enumerate(bounds):  # rank
        for j in range(lo, hi, 64):
            c = L[j:min(j + 64, hi)]
            lanes = np.arange(c.size)
            same = c[None, :] == c[:, None]                      # same[l][k]: lane k holds lane l's byte
            before = (same & (lanes[None, :] < lanes[:, None])).sum(axis=1)
            at = cur[w][c]
            P[at + before] = (j + lanes).astype(IDX)
            first = before == 0
            cur[w][c[first]] = at[first] + same[first].sum(axis=1)
    return L, P


def inverse(col, ptr):
    """-> the block the column and origin pointer stand for, by the kernel's phases"""
    n = len(col)
    assert 1 <= n <= SMALL_MAX and 0 <= ptr < n
    L, P = build_T(col)
    X1 = np.zeros(n, dtype=IDX)  # X1[i] = X[i + 1]; X[0] = ptr
    m = 1
    while m <= n:
        ext = min(m, n + 1 - m)
        r = np.arange(ext)
        src = np.where(r > 0, X1[np.maximum(r, 1) - 1], IDX(ptr)).astype(IDX)
        X1[m + r - 1] = P[src]
        if 2 * m > n:
            break
        P = P[P]  # (through registers in the kernel: every read before any write)
        assert P.dtype == IDX
        m <<= 1
    return L[X1].tobytes()
