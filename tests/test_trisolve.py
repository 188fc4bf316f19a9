"""Sparse triangular solve / SGS preconditioner vs scipy (host path).

Oracle: scipy fp64 spsolve_triangular on the explicitly extracted triangle
(utils/trisolve_cases.py).  The GPU twin of this file is
test_trisolve_gpu.py.
"""
import numpy as np
import pytest
import scipy.sparse as sps

from utils.common import types
from utils.trisolve_cases import (battery_case, bidiagonal, from_strict,
                                  oracle, py_levels, random_strict,
                                  replay_schedule, rhs, tol)


@pytest.fixture(scope="module")
def poisson32():
    from sparse import gallery

    return gallery.poisson2d(32, 32)


@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("unit", [False, True])
def test_matches_scipy(dt, lower, unit):
    from sparse import DistArray, csr_array
    from sparse.linalg import spsolve_triangular

    A, T = battery_case(dt, lower, unit)
    Ad = csr_array(A)
    for shape in [(1500,), (1500, 3), (1500, 33)]:
        b = rhs(shape, dt)
        x = spsolve_triangular(Ad, b, lower=lower, unit_diagonal=unit)
        assert isinstance(x, DistArray)
        assert x.shape == shape and x.dtype == np.dtype(dt)
        assert np.allclose(np.asarray(x), oracle(T, b, lower, unit), **tol(dt))


def test_other_formats_and_input_kinds():
    import torch

    from sparse import asdistarray, csc_array, csr_array
    from sparse.linalg import spsolve_triangular

    A, T = battery_case(np.float64, True, False)
    b = rhs((1500,), np.float64)
    ref = oracle(T, b, True)
    for Ad in (csr_array(A), csc_array(A.tocsc()), A):
        for bb in (b, torch.as_tensor(b), asdistarray(b)):
            assert np.allclose(np.asarray(spsolve_triangular(Ad, bb)), ref,
                               **tol(np.float64))


def test_entries_outside_the_triangle_are_ignored():
    from sparse import csr_array
    from sparse.linalg import spsolve_triangular

    r, c = random_strict(200, 4, seed=2)
    for lower in (True, False):
        A, T = from_strict(r, c, 200, lower, np.float64, 2, other_side=True)
        assert (A - T).nnz > 0  # there IS something on the other side
        b = rhs((200,), np.float64)
        x = spsolve_triangular(csr_array(A), b, lower=lower)
        assert np.allclose(np.asarray(x), oracle(T, b, lower),
                           **tol(np.float64))


def test_duplicates_are_summed():
    from sparse import csr_array
    from sparse.linalg import spsolve_triangular

    # row 1: (1,0) stored twice, diagonal stored twice; row 2: a stored zero
    data = np.array([2.0, 0.5, 0.25, 1.0, 3.0, 0.0, -1.0, 4.0])
    indices = np.array([0, 0, 0, 1, 1, 0, 1, 2])
    indptr = np.array([0, 1, 5, 8])
    A = csr_array((data, indices, indptr), shape=(3, 3))
    dense = np.array([[2.0, 0, 0], [0.75, 4.0, 0], [0.0, -1.0, 4.0]])
    b = np.array([1.0, 2.0, 3.0])
    x = spsolve_triangular(A, b, lower=True)
    assert np.allclose(np.asarray(x), np.linalg.solve(dense, b), rtol=1e-13)


def test_singular_raises():
    from sparse import csr_array
    from sparse.linalg import TriangularSolver, spsolve_triangular

    missing = sps.csr_matrix(np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 1, 3]]))
    with pytest.raises(np.linalg.LinAlgError):
        spsolve_triangular(csr_array(missing), np.ones(3))
    zero = csr_array((np.array([1.0, 2.0, 0.0, 3.0]), np.array([0, 0, 1, 2]),
                      np.array([0, 1, 3, 4])), shape=(3, 3))
    with pytest.raises(np.linalg.LinAlgError):
        TriangularSolver(zero, lower=True)
    # cancelling duplicates on the diagonal are a zero diagonal too
    cancel = csr_array((np.array([1.0, 2.0, -2.0, 3.0]),
                        np.array([0, 1, 1, 2]), np.array([0, 1, 3, 4])),
                       shape=(3, 3))
    with pytest.raises(np.linalg.LinAlgError):
        TriangularSolver(cancel, lower=False)
    # ... and none of it matters with an implied unit diagonal
    x = spsolve_triangular(csr_array(missing), np.ones(3), unit_diagonal=True)
    assert np.allclose(np.asarray(x), [1.0, -1.0, 2.0])


def test_shape_errors():
    from sparse import csr_array
    from sparse.linalg import TriangularSolver, spsolve_triangular

    with pytest.raises(ValueError):
        TriangularSolver(csr_array(sps.random(4, 5, 0.5, random_state=0,
                                              format="csr")))
    A = csr_array(sps.identity(4, format="csr"))
    for bad in (np.ones(5), np.ones((3, 2)), np.ones((4, 2, 2))):
        with pytest.raises(ValueError):
            spsolve_triangular(A, bad)


@pytest.mark.parametrize("lower", [True, False])
def test_tiny(lower):
    from sparse import csr_array
    from sparse.linalg import TriangularSolver, spsolve_triangular

    s0 = TriangularSolver(csr_array((0, 0)), lower=lower)
    assert s0.nlevels == 0 and s0.schedule == [] and len(s0.levels) == 0
    assert np.asarray(s0.solve(np.zeros(0))).shape == (0,)
    assert np.asarray(s0.solve(np.zeros((0, 3)))).shape == (0, 3)
    one = csr_array(sps.csr_matrix(np.array([[4.0]])))
    x = spsolve_triangular(one, np.array([2.0]), lower=lower)
    assert np.allclose(np.asarray(x), [0.5])
    s1 = TriangularSolver(one, lower=lower)
    assert s1.nlevels == 1 and s1.schedule == [("chain", 0, 1)]


def test_levels_random():
    from sparse import csr_array
    from sparse.linalg import TriangularSolver

    r, c = random_strict(400, 3, seed=9)
    for lower in (True, False):
        A, T = from_strict(r, c, 400, lower, np.float64, 9)
        s = TriangularSolver(csr_array(A), lower=lower)
        ref = py_levels(T, lower)
        assert np.array_equal(np.asarray(s.levels), ref)
        assert s.nlevels == ref.max() + 1
        b = rhs((400,), np.float64)
        assert np.allclose(replay_schedule(s, T, b), oracle(T, b, lower),
                           **tol(np.float64))


def test_levels_numpy_fallback_agrees():
    from sparse.trisolve import _levels_numpy

    r, c = random_strict(300, 3, seed=4)
    for lower in (True, False):
        _, T = from_strict(r, c, 300, lower, np.float64, 4)
        S = (sps.tril(T, -1) if lower else sps.triu(T, 1)).tocsr()
        got = _levels_numpy(S.indptr.astype(np.int64), S.indices, lower)
        assert np.array_equal(got, py_levels(T, lower))


def test_levels_bidiagonal():
    from sparse import csr_array
    from sparse.linalg import TriangularSolver

    n = 500
    A, T = bidiagonal(n)
    with pytest.warns(UserWarning, match="inherently sequential"):
        s = TriangularSolver(csr_array(A), lower=True)
    assert s.nlevels == n
    assert np.array_equal(np.asarray(s.levels), np.arange(n))
    assert s.schedule == [("chain", 0, n)]


def test_levels_poisson(poisson32):
    from sparse.linalg import TriangularSolver

    T = sps.tril(poisson32.to_scipy_sparse_csr()).tocsr()
    s = TriangularSolver(poisson32, lower=True)
    assert s.nlevels == 63
    assert np.array_equal(np.asarray(s.levels), py_levels(T, True))
    assert np.bincount(np.asarray(s.levels)).max() == 32
    assert s.schedule == [("chain", 0, 63)]


def test_schedule_grouping():
    """Wide levels stand alone, runs of narrow levels merge into chains; the
    cap itself is narrow.  (Host logic: the kernels run it in
    test_trisolve_gpu.py.)"""
    from sparse import csr_array
    from sparse.linalg import TRSV_CHAIN_WIDTH, TriangularSolver

    W = TRSV_CHAIN_WIDTH
    for width, first in ((W, "chain"), (W + 1, "wide")):
        n = width + 1
        rows = np.full(width, width)
        A, T = from_strict(rows, np.arange(width), n, True, np.float64, 1,
                           other_side=False)
        s = TriangularSolver(csr_array(A), lower=True)
        want = [("chain", 0, 2)] if first == "chain" else \
            [("wide", 0, 1), ("chain", 1, 2)]
        assert s.schedule == want
        b = rhs((n,), np.float64)
        assert np.allclose(replay_schedule(s, T, b), oracle(T, b, True),
                           **tol(np.float64))


def test_solver_is_a_linear_operator():
    from sparse import asdistarray, csr_array, darray
    from sparse.linalg import LinearOperator, TriangularSolver

    A, T = battery_case(np.float64, False, False)
    s = TriangularSolver(csr_array(A), lower=False)
    assert isinstance(s, LinearOperator) and s.shape == (1500, 1500)
    b = rhs((1500,), np.float64)
    ref = oracle(T, b, False)
    assert np.allclose(np.asarray(s.matvec(b)), ref, **tol(np.float64))
    out = darray.zeros((1500,))
    assert s.matvec(b, out=out) is out
    assert np.allclose(np.asarray(out), ref, **tol(np.float64))
    bd = asdistarray(b.copy())
    assert s.solve(bd, out=bd) is bd  # out may alias b
    assert np.allclose(np.asarray(bd), ref, **tol(np.float64))


def test_overwrite_b():
    from sparse import asdistarray, csr_array
    from sparse.linalg import spsolve_triangular

    A, T = battery_case(np.float64, True, False)
    Ad = csr_array(A)
    b = rhs((1500, 3), np.float64)
    ref = oracle(T, b, True)
    bd = asdistarray(b.copy())
    x = spsolve_triangular(Ad, bd, overwrite_b=True)
    assert x is bd and np.allclose(np.asarray(bd), ref, **tol(np.float64))
    keep = asdistarray(b.copy())
    x = spsolve_triangular(Ad, keep)
    assert x is not keep and np.array_equal(np.asarray(keep), b)


def test_cache_follows_values():
    from sparse import csr_array
    from sparse.linalg import spsolve_triangular

    A, T = battery_case(np.float64, True, False)
    Ad = csr_array(A)
    b = rhs((1500,), np.float64)
    spsolve_triangular(Ad, b)
    first = Ad._plan_cache[("trsv", True, False)]
    spsolve_triangular(Ad, b)
    assert Ad._plan_cache[("trsv", True, False)] is first  # reused
    spsolve_triangular(Ad, b, lower=False)
    assert ("trsv", False, False) in Ad._plan_cache  # one per triangle
    Ad.data = 2.0 * A.data
    assert not any(k[0] == "trsv" for k in Ad._plan_cache)
    x = spsolve_triangular(Ad, b)
    assert np.allclose(np.asarray(x), oracle(T, b, True) / 2.0,
                       **tol(np.float64))


def test_sgs_operator(poisson32):
    from sparse import darray
    from sparse.linalg import LinearOperator, sgs_preconditioner

    M = sgs_preconditioner(poisson32)
    assert isinstance(M, LinearOperator)
    S = poisson32.to_scipy_sparse_csr()
    Minv = np.linalg.inv(((sps.tril(S) @ sps.diags(1.0 / S.diagonal())
                           @ sps.triu(S))).toarray())
    r = rhs((1024,), np.float64)
    assert np.allclose(np.asarray(M.matvec(r)), Minv @ r, rtol=1e-10)
    out = darray.zeros((1024,))
    assert M.matvec(r, out=out) is out
    assert np.allclose(np.asarray(out), Minv @ r, rtol=1e-10)
    assert np.allclose(np.asarray(M.rmatvec(r)), Minv @ r, rtol=1e-10)


def test_sgs_preconditioned_cg(poisson32):
    """SGS-CG needs at most 0.7x the iterations of plain CG on the 32x32
    Poisson problem (scipy's CG with the same preconditioner: 34 vs 59)."""
    from sparse.linalg import cg, sgs_preconditioner

    b = np.ones(1024)

    def iterations(M):
        count = [0]

        def cb(_x):
            count[0] += 1

        x, info = cg(poisson32, b, tol=1e-8, conv_test_iters=1, M=M,
                     callback=cb)
        assert info == 0
        r = b - poisson32.to_scipy_sparse_csr() @ np.asarray(x)
        assert np.linalg.norm(r) <= 1e-7 * np.linalg.norm(b)
        return count[0]

    plain = iterations(None)
    sgs = iterations(sgs_preconditioner(poisson32))
    print(f"CG iterations: plain {plain}, SGS {sgs}")
    assert sgs <= 0.7 * plain


def test_result_dtype_promotes():
    """A float32 triangle with a float64 (or complex) b solves in the
    promoted dtype."""
    from sparse import csr_array
    from sparse.linalg import spsolve_triangular

    A, T = battery_case(np.float32, True, False)
    Ad = csr_array(A)
    for bdt in (np.float64, np.complex128):
        b = rhs((1500,), bdt)
        x = spsolve_triangular(Ad, b)
        assert x.dtype == np.dtype(bdt)
        assert np.allclose(np.asarray(x), oracle(T.astype(bdt), b, True),
                           **tol(bdt))


def test_world_size_above_one_raises(monkeypatch):
    from sparse import csr_array
    from sparse.linalg import (TriangularSolver, sgs_preconditioner,
                               spsolve_triangular)
    from sparse.parallel import comm

    A = csr_array(sps.identity(4, format="csr"))
    monkeypatch.setattr(comm, "world_size", lambda: 2)
    for call in (lambda: TriangularSolver(A),
                 lambda: spsolve_triangular(A, np.ones(4)),
                 lambda: sgs_preconditioner(A)):
        with pytest.raises(NotImplementedError, match="world size"):
            call()
