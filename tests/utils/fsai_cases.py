"""Inputs, the oracle and the checks shared by test_fsai.py and
test_fsai_gpu.py.

Every matrix is Hermitian and strictly diagonally dominant with a real
positive diagonal: strict-lower random values in +-[0.1, 1] (random phases
for complex dtypes), plus the conjugate transpose, plus 1 + sum_j |a_ij| on
the diagonal.  So every pattern block S = A[J, J] is positive definite and
well conditioned, and a float32 / complex64 run of the oracle agrees with the
wide one to <= 8e-8 elementwise — far inside tol(dt).

The oracle, fsai_ref, is a plain numpy loop over the rows of the pattern in
float64 / complex128: S y = e_m by np.linalg.cholesky and two solves,
G[i, J] = conj(y) / sqrt(y_m).
"""
import functools

import numpy as np
import scipy.sparse as sps

from utils.trisolve_cases import tol, wide_dtype


def hermitian_dominant(rows, cols, n, dt, seed):
    """scipy CSR of dtype dt from the strict-lower pattern (rows > cols, no
    duplicates); sorted indices."""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    assert np.all(rows > cols)
    assert len(np.unique(rows * n + cols)) == len(rows)
    v = rng.uniform(0.1, 1.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    if np.issubdtype(dt, np.complexfloating):
        v = v * np.exp(2j * np.pi * rng.random(len(rows)))
    L = sps.csr_matrix((v, (rows, cols)), shape=(n, n))
    off = L + L.conj().T
    d = 1.0 + np.asarray(abs(off).sum(axis=1)).ravel()
    A = (off + sps.diags(d)).tocsr()
    A.sort_indices()
    return A.astype(dt)


# -- strict-lower patterns -------------------------------------------------------
def _blocks_pattern(nb=1100, bs=6):
    b = np.repeat(np.arange(nb) * bs, bs * bs)
    r = b + np.tile(np.repeat(np.arange(bs), bs), nb)
    c = b + np.tile(np.tile(np.arange(bs), bs), nb)
    low = r > c
    return r[low], c[low], nb * bs


def _band_pattern(n=1500, dist=12, p=0.5, seed=37):
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for d in range(1, dist + 1):
        i = np.arange(d, n)
        i = i[rng.random(len(i)) < p]
        rows.append(i)
        cols.append(i - d)
    return np.concatenate(rows), np.concatenate(cols), n


def _stair_pattern(n=200, width=70):
    """Dense lower band: row i has min(i + 1, width) entries with its
    diagonal, so every length from 1 to width occurs."""
    rows, cols = [], []
    for i in range(1, n):
        c = np.arange(max(0, i - width + 1), i)
        rows.append(np.full(len(c), i))
        cols.append(c)
    return np.concatenate(rows), np.concatenate(cols), n


def _wide_pattern(n=600, per_row=60, seed=53):
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(1, n):
        c = np.unique(rng.integers(0, i, per_row))
        rows.append(np.full(len(c), i))
        cols.append(c)
    return np.concatenate(rows), np.concatenate(cols), n


def _arrow_pattern(n=420, last=300, seed=59):
    """A sub-diagonal, and a last row of `last` entries below its diagonal:
    one pattern row of last + 1 entries."""
    rng = np.random.default_rng(seed)
    i = np.arange(1, n - 1)
    c = np.append(rng.choice(n - 2, last - 1, replace=False), n - 2)
    return (np.concatenate([i, np.full(last, n - 1)]),
            np.concatenate([i - 1, np.sort(c)]), n)


_PATTERNS = {
    "blocks": _blocks_pattern,
    "band": _band_pattern,
    "stair": _stair_pattern,
    "wide": _wide_pattern,
    "arrow": _arrow_pattern,
}
case_names = ["stencil"] + list(_PATTERNS)


@functools.lru_cache(maxsize=None)
def case(name, dt=np.float64):
    """The named test matrix as scipy CSR of dtype dt (built once; do not
    modify)."""
    if name == "stencil":
        from sparse import gallery

        A = to_scipy(gallery.poisson2d(24, 20)).astype(dt)
        A.sort_indices()
        return A
    r, c, n = _PATTERNS[name]()
    return hermitian_dominant(r, c, n, np.dtype(dt).type, seed=len(name) + 200)


# -- pattern and oracle ----------------------------------------------------------
def lower_pattern(M, power=1):
    """The pattern of fsai: the structure of tril(M^power), formed on a copy
    of M whose values are all ones, plus the whole diagonal; scipy CSR of
    ones with sorted indices."""
    n = M.shape[0]
    ones = sps.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
    S = ones
    for _ in range(power - 1):
        S = S @ ones
    P = (sps.tril(S) + sps.identity(n)).tocsr()
    P.sort_indices()
    P.data[:] = 1.0
    return P


def hermitian(A):
    """The matrix fsai sees: the stored lower triangle of A and its conjugate
    transpose, in the wide dtype."""
    A = A.astype(wide_dtype(A.dtype))
    low = sps.tril(A, -1)
    H = (low + low.conj().T + sps.diags(A.diagonal())).tocsr()
    H.sort_indices()
    return H


def fsai_ref(A, P):
    """The definition, row by row, in float64 / complex128: scipy CSR on the
    structure of P."""
    H = hermitian(A)
    n = H.shape[0]
    dense = H.toarray() if n <= 2000 else None
    data = np.zeros(P.nnz, dtype=H.dtype)
    for i in range(n):
        s, e = P.indptr[i], P.indptr[i + 1]
        J = P.indices[s:e]
        assert J[-1] == i
        S = (dense[np.ix_(J, J)] if dense is not None
             else H[J][:, J].toarray())
        C = np.linalg.cholesky(S)
        em = np.zeros(len(J), dtype=H.dtype)
        em[-1] = 1.0
        y = np.linalg.solve(C.conj().T, np.linalg.solve(C, em))
        assert abs(y[-1].imag) <= 1e-14 * abs(y[-1]) and y[-1].real > 0
        data[s:e] = y.conj() / np.sqrt(y[-1].real)
    return sps.csr_matrix((data, P.indices.copy(), P.indptr.copy()),
                          shape=P.shape)


@functools.lru_cache(maxsize=None)
def case_ref(name, dt=np.float64, power=1):
    """(P, fsai_ref) of case(name, dt), computed once."""
    A = case(name, dt)
    P = lower_pattern(A, power)
    return P, fsai_ref(A, P)


# -- checks ----------------------------------------------------------------------
def to_scipy(M):
    """A scipy copy of M: on the host to_scipy_sparse_csr shares M's memory,
    which refactor rewrites in place."""
    S = M.to_scipy_sparse_csr().copy()
    S.sort_indices()
    return S


def check_fsai(fac, A, P, ref=None, exact=False):
    """The checks every FSAI gets.  G is stored exactly on P; its diagonal is
    real and positive; (G A)[i, j] vanishes on the pattern positions j < i
    within atol as a fraction of max |A|; diag(G A G^H) is 1 within tol (with
    exact=True G A G^H is the identity everywhere); G^H is the exact conjugate
    transpose; and, given the oracle's `ref`, G agrees with it elementwise
    within tol.  Returns G as scipy CSR."""
    t = tol(A.dtype)
    n = A.shape[0]
    G, GH = to_scipy(fac.G), to_scipy(fac.GH)
    assert G.dtype == A.dtype and GH.dtype == A.dtype
    assert fac.shape == A.shape and fac.dtype == A.dtype
    assert np.array_equal(G.indptr, P.indptr)
    assert np.array_equal(G.indices, P.indices)
    assert fac.nnz == P.nnz
    assert fac.max_row == (int(np.diff(P.indptr).max()) if n else 0)
    d = G.diagonal()
    assert np.all(d.imag == 0) and np.all(d.real > 0)
    back = G.conj().T.tocsr()
    back.sort_indices()
    assert np.array_equal(GH.indptr, back.indptr)
    assert np.array_equal(GH.indices, back.indices)
    assert np.array_equal(GH.data, back.data)
    H = hermitian(A)
    Gw = G.astype(H.dtype)
    GA = (Gw @ H).tocsr()
    strict = sps.tril(P, -1).tocsr()
    on = GA.multiply(strict).tocsr()
    top = abs(H).max() if H.nnz else 1.0
    worst = (abs(on).max() if on.nnz else 0.0) / top
    print(f"max |(G A)[i, j]| / max|A| on the pattern, j < i: {worst:.3e}")
    assert worst <= t["atol"]
    E = (GA @ Gw.conj().T).tocsr()
    dd = E.diagonal()
    print(f"max |diag(G A G^H) - 1|: {np.abs(dd - 1).max() if n else 0:.3e}")
    assert np.allclose(dd, 1.0, **t)
    if exact:
        R = (E - sps.identity(n)).tocsr()
        worst = abs(R).max() if R.nnz else 0.0
        print(f"max |G A G^H - I| everywhere: {worst:.3e}")
        assert worst <= t["atol"] + t["rtol"]
    if ref is not None:
        assert np.array_equal(ref.indptr, G.indptr)
        assert np.array_equal(ref.indices, G.indices)
        print("max elementwise difference to fsai_ref: "
              f"{np.abs(G.data - ref.data).max() if n else 0:.3e}")
        assert np.allclose(G.data, ref.data, **t)
    return G


def apply_ref(G, r):
    """G^H (G r) with scipy in the wide dtype."""
    w = wide_dtype(np.result_type(G.dtype, np.asarray(r).dtype))
    Gw = G.astype(w)
    return Gw.conj().T @ (Gw @ np.asarray(r).astype(w))


def row_lengths(names=("stair", "arrow")):
    """The pattern row lengths that occur in the named cases."""
    out = set()
    for name in names:
        out |= set(np.diff(lower_pattern(case(name)).indptr).tolist())
    return out
