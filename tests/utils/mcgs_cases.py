"""Inputs and oracles shared by test_mcgs.py and test_mcgs_gpu.py.

Inputs are diagonally dominant, |a_ii| = 1 + sum_j |a_ij| with random signs
(and phases for complex dtypes), so Gauss-Seidel iterates stay O(|b|).

Colouring oracle: plain-Python sequential greedy over A ∪ Aᵀ in decreasing
(h(i), i) priority, the hash re-implemented here in numpy.  Sweep oracle:
scipy in fp64 / complex128 on the matrix permuted by `order`: with B = A[p][:,
p] and L, U, D its triangles, a forward sweep from y0 is y0 + (D+L)⁻¹ (P b −
B y0), a backward one uses D+U, and x[p] = y.
"""
import functools

import numpy as np
import scipy.sparse as sps
from scipy.sparse.linalg import spsolve_triangular as sp_solve

from utils.trisolve_cases import wide_dtype


# -- inputs -------------------------------------------------------------------
def from_pattern(rows, cols, n, dt, seed):
    """scipy CSR of dtype dt with the given off-diagonal pattern (rows !=
    cols), random values and a dominant diagonal."""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    assert np.all(rows != cols)
    v = rng.uniform(0.1, 1.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    if np.issubdtype(dt, np.complexfloating):
        v = v * np.exp(2j * np.pi * rng.random(len(rows)))
    S = sps.csr_matrix((v, (rows, cols)), shape=(n, n))  # sums duplicates
    d = (1.0 + np.asarray(abs(S).sum(axis=1)).ravel()) \
        * rng.choice([-1.0, 1.0], n)
    A = (S + sps.diags(d)).tocsr().astype(dt)
    A.sort_indices()
    return A


def _sym_pairs(n, per_row, seed, lo=0):
    """About per_row entries a row in a symmetric pattern on rows lo..n-1."""
    rng = np.random.default_rng(seed)
    m = (n - lo) * per_row // 2
    r = rng.integers(lo, n, m)
    c = rng.integers(lo, n, m)
    keep = r != c
    r, c = r[keep], c[keep]
    return np.concatenate([r, c]), np.concatenate([c, r])


@functools.lru_cache(maxsize=None)
def random_sym(dt=np.float64, n=1500, seed=31):
    """Symmetric pattern, about 6 off-diagonal entries a row, nonsymmetric
    values: mean row length above 4, so 8 lanes per row."""
    r, c = _sym_pairs(n, 6, seed)
    return from_pattern(r, c, n, dt, seed)


@functools.lru_cache(maxsize=None)
def dense_block(dt=np.float64, seed=37):
    """A dense 70 x 70 block (70 colours: the 64-colour window must move;
    rows of 70 entries: 64 lanes per row) next to 130 sparse rows."""
    nb, n = 70, 200
    i, j = np.nonzero(~np.eye(nb, dtype=bool))
    r, c = _sym_pairs(n, 4, seed, lo=nb)
    return from_pattern(np.concatenate([i, r]), np.concatenate([j, c]), n,
                        dt, seed)


@functools.lru_cache(maxsize=None)
def lower_bidiagonal(n=300, dt=np.float64):
    """Diagonal plus first subdiagonal: the pattern is NOT symmetric."""
    i = np.arange(1, n)
    return from_pattern(i, i - 1, n, dt, seed=41)


@functools.lru_cache(maxsize=None)
def diagonal_only(n=100, dt=np.float64):
    return from_pattern([], [], n, dt, seed=43)


def rhs(shape, dt, seed=5):
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1.0, 1.0, shape)
    if np.issubdtype(dt, np.complexfloating):
        b = b + 1j * rng.uniform(-1.0, 1.0, shape)
    return b.astype(dt)


def to_csr_array(A, idx="int32"):
    """csr_array of scipy A on the runtime's device with int32 or int64
    column indices."""
    import torch

    from sparse import csr_array

    Ad = csr_array(A)
    assert Ad._indices.dtype == torch.int32
    if idx == "int64":
        Ad = csr_array.from_local(Ad._indptr, Ad._indices.to(torch.int64),
                                  Ad._values, Ad.partition, Ad.shape)
    return Ad


def raw_csr_array(data, indices, indptr, n):
    """csr_array over exactly these arrays: unsorted rows and duplicates
    stay, which the constructor would fix."""
    import torch

    from sparse import csr_array
    from sparse.parallel.partition import RowPartition
    from sparse.runtime import runtime

    dev = runtime().device
    return csr_array.from_local(
        torch.as_tensor(np.asarray(indptr, dtype=np.int64), device=dev),
        torch.as_tensor(np.asarray(indices, dtype=np.int32), device=dev),
        torch.as_tensor(np.asarray(data), device=dev),
        RowPartition.equal(n, 1), (n, n))


def shuffled_with_duplicates():
    """random_sym(n=200) with every row's entries shuffled and one
    off-diagonal entry and the diagonal stored twice (the second time at
    half the value).  Returns (the pattern's scipy matrix, the csr_array
    over the raw arrays, the scipy matrix with the duplicates summed)."""
    A = random_sym(n=200, seed=3)
    rng = np.random.default_rng(0)
    indptr, indices, data = [0], [], []
    for i in range(200):
        s, e = A.indptr[i], A.indptr[i + 1]
        p = rng.permutation(e - s)
        idx, val = A.indices[s:e][p], A.data[s:e][p]
        twice = np.flatnonzero(idx != i)[:1]
        twice = np.append(twice, np.flatnonzero(idx == i))
        indices += list(idx) + list(idx[twice])
        data += list(val) + list(0.5 * val[twice])
        indptr.append(len(indices))
    Ad = raw_csr_array(data, indices, indptr, 200)
    assert not Ad.to_scipy_sparse_csr().has_sorted_indices
    summed = sps.csr_matrix((data, indices, indptr), shape=(200, 200))
    summed.sum_duplicates()
    return A, Ad, summed


def red_black(nx, ny):
    """Grid-parity colours of poisson2d(nx, ny) (row = ix * ny + iy)."""
    ix, iy = np.divmod(np.arange(nx * ny), ny)
    return ((ix + iy) % 2).astype(np.int32)


# -- colouring oracle -----------------------------------------------------------
def py_hash(i, seed=0):
    x = np.asarray(i).astype(np.uint32) ^ np.uint32(seed)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    x = x ^ (x >> np.uint32(16))
    return x


def adjacency(A):
    """Neighbour lists of the graph of A ∪ Aᵀ without the diagonal; stored
    zeros count."""
    A = A.tocsr()
    n = A.shape[0]
    r = np.repeat(np.arange(n), np.diff(A.indptr))
    c = A.indices.astype(np.int64)
    off = r != c
    P = sps.csr_matrix((np.ones(2 * off.sum()),
                        (np.concatenate([r[off], c[off]]),
                         np.concatenate([c[off], r[off]]))), shape=(n, n))
    return [P.indices[P.indptr[i]: P.indptr[i + 1]] for i in range(n)]


def py_greedy(A, seed=0):
    """Sequential greedy in decreasing (h(i), i), plain Python."""
    n = A.shape[0]
    nbrs = adjacency(A)
    h = py_hash(np.arange(n), seed)
    visit = sorted(range(n), key=lambda i: (int(h[i]), i), reverse=True)
    colors = [-1] * n
    for i in visit:
        taken = {colors[j] for j in nbrs[i]}
        c = 0
        while c in taken:
            c += 1
        colors[i] = c
    return np.array(colors, dtype=np.int32)


def check_coloring(A, colors):
    """Proper over A ∪ Aᵀ, colours 0..C-1 all used, C <= max degree + 1."""
    colors = np.asarray(colors)
    n = A.shape[0]
    assert colors.shape == (n,) and colors.dtype == np.int32
    nbrs = adjacency(A)
    for i in range(n):
        assert not np.any(colors[nbrs[i]] == colors[i]), i
    if n:
        ncolors = int(colors.max()) + 1
        assert colors.min() == 0
        assert len(np.unique(colors)) == ncolors
        assert ncolors <= max(len(x) for x in nbrs) + 1


# -- sweep oracles ----------------------------------------------------------------
def _triangles(A, order):
    w = wide_dtype(A.dtype)
    B = A.astype(w).tocsr()[order][:, order]
    D = sps.diags(B.diagonal())
    return B, (sps.tril(B, -1) + D).tocsr(), (sps.triu(B, 1) + D).tocsr(), D


def sweep_oracle(A, order, x0, b, direction="forward", iterations=1):
    order = np.asarray(order).astype(np.int64)
    B, DL, DU, _ = _triangles(A, order)
    w = B.dtype
    y = np.asarray(x0).astype(w)[order]
    pb = np.asarray(b).astype(w)[order]
    passes = {"forward": [True], "backward": [False],
              "symmetric": [True, False]}[direction]
    for _ in range(iterations):
        for lower in passes:
            y = y + sp_solve(DL if lower else DU, pb - B @ y, lower=lower)
    x = np.empty_like(y)
    x[order] = y
    return x


def sgs_oracle(A, order, r):
    """(D+U)⁻¹ D (D+L)⁻¹ r in the ordering `order`."""
    order = np.asarray(order).astype(np.int64)
    B, DL, DU, D = _triangles(A, order)
    y = sp_solve(DL, np.asarray(r).astype(B.dtype)[order], lower=True)
    y = sp_solve(DU, D @ y, lower=False)
    x = np.empty_like(y)
    x[order] = y
    return x


def check_sweeps(gs, A, dt, shapes=None, iterations=2):
    """gs.sweep in every direction against the oracle, on right-hand sides of
    shape (n,), (n, 3) and (n, 33) unless told otherwise."""
    from sparse import asdistarray
    from utils.trisolve_cases import tol

    n = A.shape[0]
    order = gs.order.cpu().numpy()
    for shape in shapes or [(n,), (n, 3), (n, 33)]:
        b = rhs(shape, dt)
        x0 = rhs(shape, dt, seed=6)
        for direction in ("forward", "backward", "symmetric"):
            x = asdistarray(x0.copy())
            assert gs.sweep(x, b, direction, iterations) is x
            assert x.shape == shape and x.dtype == np.dtype(dt)
            ref = sweep_oracle(A, order, x0, b, direction, iterations)
            assert np.allclose(np.asarray(x), ref, **tol(dt)), \
                (shape, direction)


def replay(gs, A, x0, b, backward=False):
    """One sweep by walking order / color_ptr on the host the way the kernels
    do, asserting on the way that the classes partition the rows in
    increasing row order and that no row reads a row of its own class."""
    A = A.tocsr()
    n = A.shape[0]
    order = gs.order.cpu().numpy().astype(np.int64)
    cp = gs.color_ptr.cpu().numpy()
    colors = gs.colors.cpu().numpy()
    assert cp[0] == 0 and cp[-1] == n and len(cp) == gs.ncolors + 1
    assert np.array_equal(np.sort(order), np.arange(n))
    x = np.asarray(x0).astype(wide_dtype(A.dtype)).copy()
    classes = range(gs.ncolors)
    for k in (reversed(classes) if backward else classes):
        rows = order[cp[k]: cp[k + 1]]
        assert np.all(np.diff(rows) > 0)  # (colour, row) order
        assert np.all(colors[rows] == k)
        inside = np.zeros(n, dtype=bool)
        inside[rows] = True
        for i in rows:
            s, e = A.indptr[i], A.indptr[i + 1]
            cj, cv = A.indices[s:e], A.data[s:e]
            off = cj != i
            assert not inside[cj[off]].any()
            x[i] = (b[i] - cv[off] @ x[cj[off]]) / cv[~off].sum()
    return x
