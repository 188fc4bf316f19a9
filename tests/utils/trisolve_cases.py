"""Inputs and oracles shared by test_trisolve.py and test_trisolve_gpu.py.

Inputs are diagonally dominant triangles, |a_ii| = 1 + sum_j |a_ij| with
random signs, so the solution stays O(|b|) however many levels there are.
The oracle is scipy's spsolve_triangular in fp64 / complex128 on the
EXPLICITLY extracted triangle.
"""
import numpy as np
import scipy.sparse as sps
from scipy.sparse.linalg import spsolve_triangular as sp_solve


def tol(dt):
    if np.dtype(dt) in (np.float32, np.complex64):
        return dict(rtol=2e-4, atol=2e-5)
    return dict(rtol=1e-10, atol=1e-12)


def wide_dtype(dt):
    return np.complex128 if np.issubdtype(dt, np.complexfloating) \
        else np.float64


def from_strict(rows, cols, n, lower, dt, seed, unit=False, other_side=True):
    """Full test matrix from the strict-LOWER pattern (rows > cols).

    Values get random signs (and phases for complex dtypes) and a dominant
    diagonal.  lower=False mirrors the pattern through the anti-diagonal
    (i -> n-1-i), which keeps the dependency structure.  With unit=True the
    strict rows are scaled by 1/|a_ii| so that the implied unit diagonal
    dominates, and the STORED diagonal is junk that must be ignored.  With
    other_side, entries are added on the other side of the diagonal; they
    must be ignored too.  Returns (A, T): the matrix to hand to the solver
    and the explicit triangle for the oracle, both scipy CSR of dtype dt."""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    assert np.all(rows > cols)
    if not lower:
        rows, cols = n - 1 - rows, n - 1 - cols
    v = rng.uniform(0.1, 1.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    if np.issubdtype(dt, np.complexfloating):
        v = v * np.exp(2j * np.pi * rng.random(len(rows)))
    S = sps.csr_matrix((v, (rows, cols)), shape=(n, n))  # sums duplicates
    d = 1.0 + np.asarray(abs(S).sum(axis=1)).ravel()
    d = d * rng.choice([-1.0, 1.0], n)
    if unit:
        S = sps.diags(1.0 / np.abs(d)) @ S
        T = (S + sps.identity(n)).tocsr()
        stored = S + sps.diags(np.full(n, 7.0))
    else:
        T = (S + sps.diags(d)).tocsr()
        stored = T
    A = stored
    if other_side:
        o = sps.random(n, n, min(1.0, 3.0 / max(n, 1)), random_state=seed + 1)
        A = A + (sps.triu(o, 1) if lower else sps.tril(o, -1))
    return A.tocsr().astype(dt), T.astype(dt)


def random_strict(n, per_row, seed, free=0):
    """Strict-lower pattern: rows >= free get ~per_row random columns below
    the diagonal, rows < free none."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(max(free, 1), n):
        c = np.unique(rng.integers(0, i, per_row))
        rows.append(np.full(len(c), i))
        cols.append(c)
    if not rows:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(rows), np.concatenate(cols)


def battery_case(dt, lower, unit, seed=11):
    """n = 1500: one level of 1100 independent rows (wider than the chain
    cap, so its own wide launch) followed by 400 rows with random
    dependencies (narrow levels: one chain launch)."""
    n = 1500
    r, c = random_strict(n, 6, seed, free=1100)
    return from_strict(r, c, n, lower, dt, seed, unit=unit)


def oracle(T, b, lower, unit=False):
    w = wide_dtype(T.dtype)
    return sp_solve(T.astype(w).tocsr(), np.asarray(b).astype(w), lower=lower,
                    unit_diagonal=unit)


def rhs(shape, dt, seed=5):
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1.0, 1.0, shape)
    if np.issubdtype(dt, np.complexfloating):
        b = b + 1j * rng.uniform(-1.0, 1.0, shape)
    return b.astype(dt)


def py_levels(T, lower):
    """Plain-Python level reference on the strict part of triangle T."""
    T = T.tocsr()
    n = T.shape[0]
    lv = [0] * n
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        best = -1
        for p in range(T.indptr[i], T.indptr[i + 1]):
            j = T.indices[p]
            if j != i:
                best = max(best, lv[j])
        lv[i] = best + 1
    return np.array(lv, dtype=np.int64)


def bidiagonal(n, dt=np.float64):
    i = np.arange(1, n)
    return from_strict(i, i - 1, n, True, dt, seed=3, other_side=False)


def replay_schedule(solver, T, b):
    """Solve by walking solver.schedule on the host the way the kernels do
    (rows of a level only read rows of earlier levels), asserting that
    dependency on the way.  Checks order / level_ptr / schedule without a
    GPU."""
    T = T.tocsr()
    n = T.shape[0]
    order = solver._order.cpu().numpy().astype(np.int64)
    lp = solver._level_ptr.cpu().numpy()
    x = np.zeros(n, dtype=wide_dtype(T.dtype))
    done = np.zeros(n, dtype=bool)
    last = 0
    for kind, lo, hi in solver.schedule:
        assert kind in ("wide", "chain") and lo == last and hi > lo
        last = hi
        for lvl in range(lo, hi):
            rows = order[lp[lvl]: lp[lvl + 1]]
            assert np.all(np.diff(rows) > 0)  # (level, row) order
            new = {}
            for i in rows:
                s, e = T.indptr[i], T.indptr[i + 1]
                cj, cv = T.indices[s:e], T.data[s:e]
                off = cj != i
                assert done[cj[off]].all()
                new[i] = (b[i] - cv[off] @ x[cj[off]]) / cv[~off].sum()
            for i, v in new.items():
                x[i] = v
            done[rows] = True
    assert last == solver.nlevels and done.all()
    return x
