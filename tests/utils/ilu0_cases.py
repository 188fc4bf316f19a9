"""Inputs and the oracle shared by test_ilu0.py and test_ilu0_gpu.py.

Every matrix is strictly row diagonally dominant, |a_ii| = 1 + sum_j |a_ij|
over the row's off-diagonal entries with random signs (phases for complex
dtypes), so ILU(0) exists and its entries stay bounded.  The oracle is a
plain-Python IKJ ILU(0), ilu0_ref, in float64 / complex128.
"""
import functools

import numpy as np
import scipy.sparse as sps

from utils.trisolve_cases import wide_dtype


def dominant(rows, cols, n, dt, seed):
    """scipy CSR of dtype dt on the off-diagonal pattern (rows, cols) (no
    duplicates, rows != cols) plus a dominant diagonal; sorted indices."""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    assert np.all(rows != cols)
    assert len(np.unique(rows * n + cols)) == len(rows)
    v = rng.uniform(0.1, 1.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    if np.issubdtype(dt, np.complexfloating):
        v = v * np.exp(2j * np.pi * rng.random(len(rows)))
    d = 1.0 + np.bincount(rows, weights=np.abs(v), minlength=n)
    d = d * rng.choice([-1.0, 1.0], n)
    ar = np.arange(n)
    A = sps.csr_matrix((np.concatenate([v, d]),
                        (np.concatenate([rows, ar]),
                         np.concatenate([cols, ar]))), shape=(n, n))
    A.sort_indices()
    return A.astype(dt)


def _unique_pairs(rows, cols, n):
    key = np.unique(np.asarray(rows, np.int64) * n + np.asarray(cols, np.int64))
    return key // n, key % n


# -- patterns (off-diagonal entries) -------------------------------------------
def _blocks_pattern(nb=1100, bs=6):
    b = np.repeat(np.arange(nb) * bs, bs * bs)
    r = b + np.tile(np.repeat(np.arange(bs), bs), nb)
    c = b + np.tile(np.tile(np.arange(bs), bs), nb)
    off = r != c
    return r[off], c[off], nb * bs


def _coupled_pattern(extra=300, seed=31):
    r, c, n = _blocks_pattern()
    rng = np.random.default_rng(seed)
    er = rng.integers(0, n, extra)
    ec = rng.integers(0, n, extra)
    keep = er // 6 != ec // 6
    r, c = _unique_pairs(np.concatenate([r, er[keep]]),
                         np.concatenate([c, ec[keep]]), n)
    return r, c, n


def _band_pattern(n=1500, dist=12, p=0.5, seed=37, thin_upper=1.0):
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for d in range(1, dist + 1):
        i = np.arange(d, n)
        lo = rng.random(len(i)) < p
        up = rng.random(len(i)) < p * thin_upper
        rows += [i[lo], i[up] - d]
        cols += [i[lo] - d, i[up]]
    return np.concatenate(rows), np.concatenate(cols), n


def _arrow_pattern(free=5000, mid=1100, deg=20, seed=41):
    rng = np.random.default_rng(seed)
    n = free + mid + 1
    last = n - 1
    mr = np.repeat(np.arange(free, free + mid), deg)
    mc = np.concatenate([rng.choice(free, deg, replace=False)
                         for _ in range(mid)])
    lr = np.full(free + 1, last)
    lc = np.append(np.arange(free), free + int(rng.integers(mid)))
    r = np.concatenate([mr, mc, lr, lc])
    c = np.concatenate([mc, mr, lc, lr])
    return r, c, n


_PATTERNS = {
    "blocks": _blocks_pattern,
    "coupled": _coupled_pattern,
    "band": _band_pattern,
    "arrow": _arrow_pattern,
    "nonsym": functools.partial(_band_pattern, seed=43, thin_upper=0.4),
}
case_names = list(_PATTERNS)


@functools.lru_cache(maxsize=None)
def case(name, dt=np.float64):
    """The named test matrix as scipy CSR of dtype dt (built once; do not
    modify)."""
    r, c, n = _PATTERNS[name]()
    return dominant(r, c, n, np.dtype(dt).type, seed=len(name) + 100)


def tridiagonal(n=200, dt=np.float64):
    i = np.arange(1, n)
    return dominant(np.concatenate([i, i - 1]), np.concatenate([i - 1, i]),
                    n, dt, seed=7)


def convection_diffusion(nx=32, c1=40.0, c2=20.0):
    """Upwind convection-diffusion on an nx x nx grid, h = 1 / (nx + 1):
    kron(I, D1) + kron(D2, I) with D = tridiag(-1 - c h, 2 + c h, -1)."""
    h = 1.0 / (nx + 1)

    def D(c):
        return sps.diags([np.full(nx - 1, -1.0 - c * h),
                          np.full(nx, 2.0 + c * h), np.full(nx - 1, -1.0)],
                         [-1, 0, 1])

    eye = sps.identity(nx)
    return (sps.kron(eye, D(c1)) + sps.kron(D(c2), eye)).tocsr()


# -- oracle ---------------------------------------------------------------------
def ilu0_ref(A):
    """Plain-Python IKJ ILU(0) of scipy CSR A (sorted, duplicate-free, full
    diagonal) in float64 / complex128: the factor on A's pattern as one CSR,
    L strictly below the diagonal (its unit diagonal implied), U on and
    above."""
    A = A.tocsr()
    w = wide_dtype(A.dtype)
    ip, ix = A.indptr, A.indices
    v = A.data.astype(w).tolist()
    n = A.shape[0]
    where = [dict(zip(ix[ip[i]: ip[i + 1]].tolist(),
                      range(ip[i], ip[i + 1]))) for i in range(n)]
    for i in range(n):
        mine = where[i]
        for q in range(ip[i], ip[i + 1]):
            k = int(ix[q])
            if k >= i:
                break
            dk = where[k][k]
            m = v[q] / v[dk]
            v[q] = m
            for t in range(dk + 1, ip[k + 1]):
                p = mine.get(int(ix[t]))
                if p is not None:
                    v[p] -= m * v[t]
    return sps.csr_matrix((np.array(v, dtype=w), ix.copy(), ip.copy()),
                          shape=A.shape)


@functools.lru_cache(maxsize=None)
def case_ref(name, dt=np.float64):
    """ilu0_ref of case(name, dt), computed once."""
    return ilu0_ref(case(name, dt))


def split(F):
    """(L, U) of a factor stored as one CSR: L unit lower, U upper."""
    n = F.shape[0]
    L = (sps.tril(F, -1) + sps.identity(n, dtype=F.dtype)).tocsr()
    U = sps.triu(F).tocsr()
    L.sort_indices()
    U.sort_indices()
    return L, U


def ref_solve(F, r):
    """U^-1 L^-1 r by scipy triangular solves with the factors of F, in the
    wide dtype of (F, r)."""
    from scipy.sparse.linalg import spsolve_triangular as sp_solve

    w = wide_dtype(np.result_type(F.dtype, np.asarray(r).dtype))
    L, U = split(F.astype(w))
    y = sp_solve(L, np.asarray(r).astype(w), lower=True, unit_diagonal=True)
    return sp_solve(U, y, lower=False)


def check_factor(fac, A, F=None, exact=False):
    """The checks every factorisation gets: L unit lower, U upper, stored on
    A's pattern, L U == A on the pattern (everywhere with exact=True) within
    tol scaled by max |A|, and, given the reference factor F, elementwise
    agreement with it within tol."""
    from utils.trisolve_cases import tol

    n = A.shape[0]
    t = tol(A.dtype)
    L, U = to_scipy(fac.L), to_scipy(fac.U)
    assert L.dtype == A.dtype and U.dtype == A.dtype
    assert L.nnz + U.nnz == A.nnz + n == fac.nnz + n
    assert (sps.triu(L, 1)).nnz == 0 and (sps.tril(U, -1)).nnz == 0
    assert np.array_equal(L.diagonal(), np.ones(n, dtype=A.dtype))
    # the two triangles together are exactly A's pattern
    both = (L + U).tocsr()
    both.sort_indices()
    assert np.array_equal(both.indptr, A.indptr)
    assert np.array_equal(both.indices, A.indices)
    d = defect(L, U, A)
    print(f"max |LU - A| / max|A| on the pattern: {d:.3e}")
    assert d <= t["atol"]
    if exact:
        d = defect(L, U, A, on_pattern=False)
        print(f"max |LU - A| / max|A| everywhere: {d:.3e}")
        assert d <= t["atol"]
    if F is not None:
        Lr, Ur = split(F)
        for got, ref in ((L, Lr), (U, Ur)):
            assert np.array_equal(got.indptr, ref.indptr)
            assert np.array_equal(got.indices, ref.indices)
            err = np.abs(got.data - ref.data)
            print(f"max elementwise difference to ilu0_ref: {err.max():.3e}")
            assert np.allclose(got.data, ref.data, **t)


def check_schedule(fac, name):
    """The launches of the factorisation for the named case."""
    from sparse.linalg import TRSV_CHAIN_WIDTH

    sch = fac.schedule
    widths = np.bincount(np.asarray(fac._Ls.levels)).tolist()
    groups = fac._sched[:, 3].tolist()
    if name == "blocks":
        assert sch == [("wide", i, i + 1) for i in range(6)]
        assert widths == [1100] * 6 and groups == [1] * 6
    elif name == "coupled":
        assert sch[:6] == [("wide", i, i + 1) for i in range(6)]
        assert sch[6:] == [("chain", 6, fac.nlevels)] and fac.nlevels > 8
        assert widths[:7] == [1076, 1056, 1049, 1048, 1058, 1067, 79]
        assert widths[-1] == 1 and max(widths[6:]) <= TRSV_CHAIN_WIDTH
    elif name in ("band", "nonsym"):
        assert sch == [("chain", 0, fac.nlevels)]
        assert 800 <= fac.nlevels <= 900 and groups == [8]
    elif name == "arrow":
        assert sch == [("wide", 0, 1), ("wide", 1, 2), ("chain", 2, 3)]
        assert widths == [5000, 1100, 1]
        assert groups == [1, 8, 64]  # lanes per row; the last row is long
    else:
        raise KeyError(name)


def to_scipy(M):
    S = M.to_scipy_sparse_csr()
    S.sort_indices()
    return S


def defect(L, U, A, on_pattern=True):
    """max |L U - A| (on A's stored positions only, or everywhere), as a
    fraction of max |A|, in the wide dtype."""
    w = wide_dtype(A.dtype)
    A = A.astype(w)
    R = (L.astype(w) @ U.astype(w) - A).tocsr()
    if on_pattern:
        mask = A.copy()
        mask.data[:] = 1.0
        R = R.multiply(mask).tocsr()
    top = abs(A).max() if A.nnz else 1.0
    return (abs(R).max() if R.nnz else 0.0) / top
