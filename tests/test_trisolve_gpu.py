"""Level-scheduled triangular solve kernels (relax.hip) vs scipy — all @gpu.

Same oracle and inputs as test_trisolve.py (utils/trisolve_cases.py); the
schedule-shape tests pin which kernel runs which levels and check the result.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from utils.common import types
from utils.trisolve_cases import (battery_case, bidiagonal, from_strict,
                                  oracle, rhs, tol)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _require_ext():
    if torch.cuda.is_available():
        from sparse.kernels import require

        require()


def _device_csr(A, idx):
    """csr_array of scipy A on the GPU with int32 or int64 column indices."""
    from sparse import csr_array

    Ad = csr_array(A)
    assert Ad._values.is_cuda and Ad._indices.dtype == torch.int32
    if idx == "int64":
        Ad = csr_array.from_local(Ad._indptr, Ad._indices.to(torch.int64),
                                  Ad._values, Ad.partition, Ad.shape)
    return Ad


def _check(solver, T, lower, dt, unit=False, shapes=None):
    n = T.shape[0]
    for shape in shapes or [(n,), (n, 3), (n, 33)]:
        b = rhs(shape, dt)
        x = solver.solve(b)
        assert x.local.is_cuda and x.shape == shape
        assert x.dtype == np.dtype(dt)
        assert np.allclose(np.asarray(x), oracle(T, b, lower, unit), **tol(dt))


@pytest.mark.parametrize("idx", ["int32", "int64"])
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("unit", [False, True])
def test_matches_scipy_gpu(dt, lower, unit, idx):
    from sparse.linalg import TriangularSolver

    A, T = battery_case(dt, lower, unit)
    s = TriangularSolver(_device_csr(A, idx), lower=lower, unit_diagonal=unit)
    # 1100 independent rows: a wide launch; the dependent rest: one chain
    assert [k for k, _, _ in s.schedule] == ["wide", "chain"]
    assert s._order.dtype == torch.int32
    _check(s, T, lower, dt, unit)


def test_entries_outside_and_duplicates_gpu():
    from sparse import csr_array
    from sparse.linalg import spsolve_triangular

    data = np.array([2.0, 0.5, 0.25, 1.0, 3.0, 9.0, 0.0, -1.0, 4.0])
    indices = np.array([0, 0, 0, 1, 1, 2, 0, 1, 2])
    indptr = np.array([0, 1, 6, 9])
    A = csr_array((data, indices, indptr), shape=(3, 3))
    assert A._values.is_cuda
    dense = np.array([[2.0, 0, 0], [0.75, 4.0, 0], [0.0, -1.0, 4.0]])
    b = np.array([1.0, 2.0, 3.0])
    x = spsolve_triangular(A, b, lower=True)
    assert np.allclose(np.asarray(x), np.linalg.solve(dense, b), rtol=1e-13)


def test_singular_and_shape_errors_gpu():
    from sparse import csr_array
    from sparse.linalg import TriangularSolver, spsolve_triangular

    missing = sps.csr_matrix(np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 1, 3]]))
    with pytest.raises(np.linalg.LinAlgError):
        TriangularSolver(csr_array(missing))
    with pytest.raises(ValueError):
        TriangularSolver(csr_array(sps.random(4, 5, 0.5, random_state=0,
                                              format="csr")))
    with pytest.raises(ValueError):
        spsolve_triangular(csr_array(sps.identity(4, format="csr")),
                           np.ones(5))


@pytest.mark.parametrize("lower", [True, False])
def test_tiny_gpu(lower):
    from sparse import csr_array
    from sparse.linalg import TriangularSolver, spsolve_triangular

    s0 = TriangularSolver(csr_array((0, 0)), lower=lower)
    assert s0.schedule == []
    assert np.asarray(s0.solve(np.zeros(0))).shape == (0,)
    one = csr_array(sps.csr_matrix(np.array([[4.0]])))
    x = spsolve_triangular(one, np.array([2.0]), lower=lower)
    assert np.allclose(np.asarray(x), [0.5])


# -- schedule shapes ----------------------------------------------------------
@pytest.mark.parametrize("lower", [True, False])
def test_all_chain_poisson_gpu(lower):
    from sparse import gallery
    from sparse.linalg import TriangularSolver

    A = gallery.poisson2d(32, 32)
    S = A.to_scipy_sparse_csr()
    T = (sps.tril(S) if lower else sps.triu(S)).tocsr()
    s = TriangularSolver(A, lower=lower)
    assert s.schedule == [("chain", 0, 63)]
    _check(s, T, lower, np.float64)


def test_all_chain_bidiagonal_gpu():
    from sparse import csr_array
    from sparse.linalg import TriangularSolver

    n = 3000
    A, T = bidiagonal(n)
    s = TriangularSolver(csr_array(A), lower=True)
    assert s.nlevels == n and s.schedule == [("chain", 0, n)]
    _check(s, T, True, np.float64)


def test_mixed_schedule_gpu():
    from sparse import csr_array
    from sparse.linalg import TriangularSolver

    n = 6000
    rng = np.random.default_rng(17)
    mid = np.arange(3000, 3100)
    tail = np.arange(3100, n)
    rows = np.concatenate([mid, mid, np.repeat(tail, 4)])
    cols = np.concatenate([
        mid - 1, np.zeros(100, np.int64),
        np.column_stack([np.full(len(tail), 3099),
                         rng.integers(0, 3000, (len(tail), 3))]).ravel()])
    A, T = from_strict(rows, cols, n, True, np.float64, 17)
    s = TriangularSolver(csr_array(A), lower=True)
    assert s.schedule == [("wide", 0, 1), ("chain", 1, 101),
                          ("wide", 101, 102)]
    _check(s, T, True, np.float64)


@pytest.mark.parametrize("extra", [0, 1])
def test_chain_cap_boundary_gpu(extra):
    """A level of exactly TRSV_CHAIN_WIDTH rows is stepped through by the
    chain kernel, one row more makes it a wide launch; the last row depends
    on all of them (the long row of the chain kernel)."""
    from sparse import csr_array
    from sparse.linalg import TRSV_CHAIN_WIDTH, TriangularSolver

    width = TRSV_CHAIN_WIDTH + extra
    n = width + 1
    A, T = from_strict(np.full(width, width), np.arange(width), n, True,
                       np.float64, 1, other_side=False)
    s = TriangularSolver(csr_array(A), lower=True)
    assert s.schedule == ([("wide", 0, 1), ("chain", 1, 2)] if extra
                          else [("chain", 0, 2)])
    _check(s, T, True, np.float64)


@functools.lru_cache(maxsize=None)
def _row_group_pattern():
    """5000 independent rows, then three levels of 1100 rows with 2, 20 and
    200 strict entries each, and one row of 5000 entries in the last."""
    rng = np.random.default_rng(23)
    free, per = 5000, 1100
    rows, cols = [], []
    prev_lo = None
    start = free
    for length in (2, 20, 200):
        for i in range(start, start + per):
            pick = rng.choice(free, length - (prev_lo is not None),
                              replace=False)
            if prev_lo is not None:  # one entry in the level before
                pick = np.append(pick, prev_lo + rng.integers(per))
            rows.append(np.full(len(pick), i))
            cols.append(pick)
        prev_lo, start = start, start + per
    long_row = start
    rows.append(np.full(free, long_row))
    # 4999 independent rows + one row of the 20-entry level: same level as
    # the 200-entry rows
    cols.append(np.append(np.arange(free - 1), free + per))
    return np.concatenate(rows), np.concatenate(cols), long_row + 1


@pytest.mark.parametrize("dt", types)
def test_row_groups_gpu(dt):
    from sparse import csr_array
    from sparse.linalg import TriangularSolver

    rows, cols, n = _row_group_pattern()
    A, T = from_strict(rows, cols, n, True, dt, 23)
    s = TriangularSolver(csr_array(A), lower=True)
    assert s.schedule == [("wide", i, i + 1) for i in range(4)]
    assert s._sched[:, 3].tolist() == [1, 1, 8, 64]  # lanes per row
    assert int(np.diff(T.indptr).max()) == 5001
    _check(s, T, True, dt, shapes=[(n,), (n, 3)])


# -- buffers and streams ------------------------------------------------------
def test_out_aliasing_and_overwrite_b_gpu():
    from sparse import asdistarray, csr_array
    from sparse.linalg import TriangularSolver, spsolve_triangular

    A, T = battery_case(np.float64, True, False)
    Ad = csr_array(A)
    s = TriangularSolver(Ad, lower=True)
    for shape in [(1500,), (1500, 3)]:
        b = rhs(shape, np.float64)
        ref = oracle(T, b, True)
        bd = asdistarray(b.copy())
        ptr = bd.local.data_ptr()
        assert s.solve(bd, out=bd) is bd and bd.local.data_ptr() == ptr
        assert np.allclose(np.asarray(bd), ref, **tol(np.float64))
        bd = asdistarray(b.copy())
        ptr = bd.local.data_ptr()
        x = spsolve_triangular(Ad, bd, overwrite_b=True)
        assert x is bd and bd.local.data_ptr() == ptr
        assert np.allclose(np.asarray(bd), ref, **tol(np.float64))
        keep = asdistarray(b.copy())
        assert spsolve_triangular(Ad, keep) is not keep
        assert np.array_equal(np.asarray(keep), b)


def test_non_default_stream_gpu():
    from sparse import asdistarray, csr_array
    from sparse.linalg import TriangularSolver

    A, T = battery_case(np.float64, False, False)
    s = TriangularSolver(csr_array(A), lower=False)
    b = rhs((1500,), np.float64)
    bd = asdistarray(b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x = s.solve(bd)
    side.synchronize()
    assert np.allclose(np.asarray(x), oracle(T, b, False), **tol(np.float64))


def test_cache_follows_values_gpu():
    from sparse import csr_array
    from sparse.linalg import spsolve_triangular

    A, T = battery_case(np.float64, True, False)
    Ad = csr_array(A)
    b = rhs((1500,), np.float64)
    spsolve_triangular(Ad, b)
    first = Ad._plan_cache[("trsv", True, False)]
    spsolve_triangular(Ad, b)
    assert Ad._plan_cache[("trsv", True, False)] is first
    Ad.data = 2.0 * A.data
    x = spsolve_triangular(Ad, b)
    assert np.allclose(np.asarray(x), oracle(T, b, True) / 2.0,
                       **tol(np.float64))


def test_sgs_preconditioned_cg_gpu():
    """Same bound as the host test: SGS-CG within 0.7x the iterations of
    plain CG on the 32x32 Poisson problem."""
    from sparse import gallery
    from sparse.linalg import cg, sgs_preconditioner

    A = gallery.poisson2d(32, 32)
    assert A._values.is_cuda
    S = A.to_scipy_sparse_csr()
    b = np.ones(1024)

    def iterations(M):
        count = [0]

        def cb(_x):
            count[0] += 1

        x, info = cg(A, b, tol=1e-8, conv_test_iters=1, M=M, callback=cb)
        assert info == 0
        r = b - S @ np.asarray(x)
        assert np.linalg.norm(r) <= 1e-7 * np.linalg.norm(b)
        return count[0]

    plain = iterations(None)
    sgs = iterations(sgs_preconditioner(A))
    print(f"CG iterations on the GPU: plain {plain}, SGS {sgs}")
    assert sgs <= 0.7 * plain


def test_result_dtype_promotes_gpu():
    from sparse import csr_array
    from sparse.linalg import spsolve_triangular

    A, T = battery_case(np.float32, True, False)
    Ad = csr_array(A)
    for bdt in (np.float64, np.complex128):
        b = rhs((1500,), bdt)
        x = spsolve_triangular(Ad, b)
        assert x.local.is_cuda and x.dtype == np.dtype(bdt)
        assert np.allclose(np.asarray(x), oracle(T.astype(bdt), b, True),
                           **tol(bdt))
