"""Graph colouring and multicolour Gauss-Seidel vs plain-Python / scipy
oracles (utils/mcgs_cases.py), on the device the runtime has.  The GPU twin
of this file, which pins the kernels, is test_mcgs_gpu.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sps

from utils.common import types
from utils.mcgs_cases import (check_coloring, check_sweeps, dense_block,
                              diagonal_only, lower_bidiagonal, py_greedy,
                              py_hash, random_sym, raw_csr_array, red_black,
                              replay, rhs, sgs_oracle,
                              shuffled_with_duplicates, sweep_oracle,
                              to_csr_array)
from utils.trisolve_cases import tol

EX = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                  "examples")


@pytest.fixture(scope="module")
def poisson32():
    from sparse import gallery

    return gallery.poisson2d(32, 32)


def _colors(A, seed=0):
    from sparse.linalg import greedy_coloring

    c = greedy_coloring(to_csr_array(A), seed=seed)
    return c.cpu().numpy()


# -- colouring ------------------------------------------------------------------
def test_hash_matches_the_definition():
    from sparse.gauss_seidel import _hash32

    def h(i, seed):  # the issue's steps on Python integers
        x = (i ^ seed) & 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        return x

    idx = np.array([0, 1, 2, 1023, 65536, 2**31 - 1, 2**32 - 1])
    for seed in (0, 7, 2**32 - 1):
        want = [h(int(i), seed) for i in idx]
        assert py_hash(idx, seed).tolist() == want
        assert _hash32(idx, seed).tolist() == want


@pytest.mark.parametrize("case", [random_sym, dense_block, lower_bidiagonal,
                                  diagonal_only])
def test_greedy_coloring_is_the_defined_one(case):
    A = case()
    got = _colors(A)
    assert got.dtype == np.int32
    assert np.array_equal(got, py_greedy(A))
    check_coloring(A, got)


def test_greedy_coloring_poisson(poisson32):
    from sparse.linalg import greedy_coloring

    S = poisson32.to_scipy_sparse_csr()
    got = greedy_coloring(poisson32).cpu().numpy()
    assert np.array_equal(got, py_greedy(S))
    check_coloring(S, got)
    assert got.max() + 1 <= 5


def test_dense_block_needs_the_window_to_move():
    got = _colors(dense_block())
    assert got.max() + 1 >= 70
    assert sorted(got[:70].tolist()) == list(range(70))


def test_nonsymmetric_pattern_is_symmetrised():
    A = lower_bidiagonal()
    assert (A != A.T).nnz > 0
    got = _colors(A)
    assert np.all(got[1:] != got[:-1])  # i and i-1 are neighbours
    assert got.max() + 1 <= 3  # a path: degree 2


def test_unsorted_rows_with_duplicates_colour_the_same():
    """A pattern that is not canonical takes the symmetrising route; the
    sweeps skip every stored diagonal entry and add up the duplicates."""
    from sparse.linalg import MulticolorGaussSeidel, greedy_coloring

    A, Ad, summed = shuffled_with_duplicates()
    got = greedy_coloring(Ad).cpu().numpy()
    assert np.array_equal(got, py_greedy(A))
    check_sweeps(MulticolorGaussSeidel(Ad), summed, np.float64)


def test_numpy_fallback_agrees():
    from sparse.gauss_seidel import _greedy_numpy

    for A in (random_sym(n=300, seed=2), dense_block()):
        P = (abs(A) + abs(A).T).tocsr()
        P.sort_indices()
        got = _greedy_numpy(P.indptr.astype(np.int64), P.indices, 0)
        assert np.array_equal(got, py_greedy(A))
        got = _greedy_numpy(P.indptr.astype(np.int64), P.indices, 11)
        assert np.array_equal(got, py_greedy(A, 11))


def test_seeds():
    A = random_sym()
    a, b, other = _colors(A, 5), _colors(A, 5), _colors(A, 6)
    assert np.array_equal(a, b)
    assert np.array_equal(a, py_greedy(A, 5))
    assert not np.array_equal(a, other)
    assert np.array_equal(other, py_greedy(A, 6))
    check_coloring(A, other)


# -- sweeps ---------------------------------------------------------------------
@pytest.mark.parametrize("idx", ["int32", "int64"])
@pytest.mark.parametrize("dt", types)
def test_sweeps_match_scipy(dt, idx):
    from sparse.linalg import MulticolorGaussSeidel

    A = random_sym(dt)
    gs = MulticolorGaussSeidel(to_csr_array(A, idx))
    assert np.array_equal(gs.colors.cpu().numpy(), py_greedy(A))
    assert gs.ncolors == int(gs.colors.max()) + 1
    check_sweeps(gs, A, dt)


def test_default_is_one_forward_sweep():
    from sparse import asdistarray
    from sparse.linalg import MulticolorGaussSeidel

    A = random_sym()
    gs = MulticolorGaussSeidel(to_csr_array(A))
    b, x0 = rhs((1500,), np.float64), rhs((1500,), np.float64, seed=6)
    x = gs.sweep(asdistarray(x0.copy()), b)
    assert np.allclose(np.asarray(x),
                       sweep_oracle(A, gs.order.cpu().numpy(), x0, b),
                       **tol(np.float64))


def test_poisson_greedy_and_red_black(poisson32):
    from sparse.linalg import MulticolorGaussSeidel

    S = poisson32.to_scipy_sparse_csr()
    gs = MulticolorGaussSeidel(poisson32)
    assert np.array_equal(gs.colors.cpu().numpy(), py_greedy(S))
    check_sweeps(gs, S, np.float64)
    rb = MulticolorGaussSeidel(poisson32, colors=red_black(32, 32))
    assert rb.ncolors == 2
    assert np.array_equal(rb.colors.cpu().numpy(), red_black(32, 32))
    assert rb.color_ptr.tolist() == [0, 512, 1024]
    check_sweeps(rb, S, np.float64)


def test_unused_colour_is_an_empty_segment():
    """A caller's colouring that leaves colour 1 unused: the schedule has an
    empty segment, skipped forwards and in reverse."""
    from sparse import gallery
    from sparse.linalg import MulticolorGaussSeidel

    A = gallery.poisson2d(8, 8)
    gs = MulticolorGaussSeidel(A, colors=2 * red_black(8, 8))
    assert gs.ncolors == 3
    assert gs.color_ptr.tolist() == [0, 32, 32, 64]
    check_sweeps(gs, A.to_scipy_sparse_csr(), np.float64)


@pytest.mark.parametrize("case", [dense_block, lower_bidiagonal])
def test_sweeps_other_structures(case):
    from sparse.linalg import MulticolorGaussSeidel

    A = case()
    gs = MulticolorGaussSeidel(to_csr_array(A))
    check_sweeps(gs, A, np.float64)


def test_diagonal_only():
    from sparse import asdistarray
    from sparse.linalg import MulticolorGaussSeidel

    A = diagonal_only()
    gs = MulticolorGaussSeidel(to_csr_array(A))
    assert gs.ncolors == 1 and gs.color_ptr.tolist() == [0, 100]
    assert np.array_equal(gs.order.cpu().numpy(), np.arange(100))
    b = rhs((100,), np.float64)
    x = gs.sweep(asdistarray(rhs((100,), np.float64, seed=6)), b)
    assert np.array_equal(np.asarray(x), b / A.diagonal())


def test_tiny():
    from sparse import asdistarray, csr_array
    from sparse.linalg import MulticolorGaussSeidel, greedy_coloring

    A0 = csr_array((0, 0))
    assert greedy_coloring(A0).shape == (0,)
    g0 = MulticolorGaussSeidel(A0)
    assert g0.ncolors == 0 and g0.color_ptr.tolist() == [0]
    assert np.asarray(g0.sweep(asdistarray(np.zeros(0)), np.zeros(0))).shape \
        == (0,)
    assert np.asarray(g0.matvec(np.zeros((0, 3)))).shape == (0, 3)
    one = csr_array(sps.csr_matrix(np.array([[4.0]])))
    assert greedy_coloring(one).tolist() == [0]
    g1 = MulticolorGaussSeidel(one)
    assert g1.ncolors == 1 and g1.order.tolist() == [0]
    x = g1.sweep(asdistarray(np.array([9.0])), np.array([2.0]), "symmetric")
    assert np.allclose(np.asarray(x), [0.5])


def test_duplicates_and_stored_diagonal():
    """Off-diagonal duplicates add up; stored diagonal entries enter only
    through their sum."""
    from sparse import asdistarray
    from sparse.linalg import MulticolorGaussSeidel

    # row 1: (1,0) twice, the diagonal twice; row 2: a stored zero at (2,0)
    data = np.array([2.0, 0.5, 0.25, 1.0, 3.0, 0.0, -1.0, 4.0])
    indices = np.array([0, 0, 0, 1, 1, 0, 1, 2])
    indptr = np.array([0, 1, 5, 8])
    A = raw_csr_array(data, indices, indptr, 3)
    dense = sps.csr_matrix(np.array([[2.0, 0, 0], [0.75, 4.0, 0],
                                     [0.0, -1.0, 4.0]]))
    gs = MulticolorGaussSeidel(A)
    # the stored zero is an edge: 0, 1 and 2 are pairwise neighbours
    assert gs.ncolors == 3
    b, x0 = np.array([1.0, 2.0, 3.0]), np.array([0.5, -0.5, 0.25])
    x = gs.sweep(asdistarray(x0.copy()), b)
    assert np.allclose(np.asarray(x),
                       sweep_oracle(dense, gs.order.cpu().numpy(), x0, b),
                       rtol=1e-13)


def test_replay_reads_no_row_of_its_own_class():
    from sparse import asdistarray
    from sparse.linalg import MulticolorGaussSeidel

    for A in (random_sym(), lower_bidiagonal(), dense_block()):
        n = A.shape[0]
        gs = MulticolorGaussSeidel(to_csr_array(A))
        assert gs.order.dtype.is_signed and gs.order.element_size() == 4
        b, x0 = rhs((n,), np.float64), rhs((n,), np.float64, seed=6)
        for backward in (False, True):
            direction = "backward" if backward else "forward"
            ref = sweep_oracle(A, gs.order.cpu().numpy(), x0, b, direction)
            assert np.allclose(replay(gs, A, x0, b, backward), ref,
                               **tol(np.float64))
            x = gs.sweep(asdistarray(x0.copy()), b, direction)
            assert np.allclose(np.asarray(x), ref, **tol(np.float64))


def test_result_dtype():
    """x holds the result: a float32 matrix sweeps in a float64 x, and an x
    narrower than A or b is refused."""
    from sparse import asdistarray
    from sparse.linalg import MulticolorGaussSeidel

    A = random_sym(np.float32)
    gs = MulticolorGaussSeidel(to_csr_array(A))
    b, x0 = rhs((1500,), np.float64), rhs((1500,), np.float64, seed=6)
    x = gs.sweep(asdistarray(x0.copy()), b)
    assert x.dtype == np.float64
    assert np.allclose(np.asarray(x),
                       sweep_oracle(A.astype(np.float64),
                                    gs.order.cpu().numpy(), x0, b),
                       **tol(np.float64))
    with pytest.raises(ValueError):
        gs.sweep(asdistarray(x0.astype(np.float32)), b)
    with pytest.raises(TypeError):
        gs.sweep(x0.copy(), b)


# -- errors ---------------------------------------------------------------------
def test_errors(poisson32):
    from sparse import asdistarray, csr_array
    from sparse.linalg import (MulticolorGaussSeidel, greedy_coloring,
                               sgs_preconditioner)

    rect = csr_array(sps.random(4, 5, 0.5, random_state=0, format="csr"))
    with pytest.raises(ValueError):
        MulticolorGaussSeidel(rect)
    with pytest.raises(ValueError):
        greedy_coloring(rect)
    missing = sps.csr_matrix(np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 1, 3]]))
    with pytest.raises(np.linalg.LinAlgError):
        MulticolorGaussSeidel(csr_array(missing))
    zero = csr_array((np.array([1.0, 2.0, 0.0, 3.0]), np.array([0, 0, 1, 2]),
                      np.array([0, 1, 3, 4])), shape=(3, 3))
    with pytest.raises(np.linalg.LinAlgError):
        MulticolorGaussSeidel(zero)
    improper = red_black(32, 32)
    improper[1] = improper[0]  # rows 0 and 1 are neighbours
    with pytest.raises(ValueError, match="improper"):
        MulticolorGaussSeidel(poisson32, colors=improper)
    with pytest.raises(ValueError):
        MulticolorGaussSeidel(poisson32, colors=red_black(32, 32)[:-1])
    with pytest.raises(ValueError):
        MulticolorGaussSeidel(poisson32, colors=-red_black(32, 32))
    with pytest.raises(ValueError, match="ordering"):
        sgs_preconditioner(poisson32, ordering="colour")
    gs = MulticolorGaussSeidel(poisson32)
    x = asdistarray(np.zeros(1024))
    with pytest.raises(ValueError, match="direction"):
        gs.sweep(x, np.ones(1024), direction="up")
    for bad in (np.ones(1023), np.ones((1024, 2))):
        with pytest.raises(ValueError):
            gs.sweep(x, bad)
    with pytest.raises(ValueError):
        gs.matvec(np.ones(5))


def test_world_size_above_one_raises(monkeypatch):
    from sparse import csr_array
    from sparse.linalg import (MulticolorGaussSeidel, greedy_coloring,
                               sgs_preconditioner)
    from sparse.parallel import comm

    A = csr_array(sps.identity(4, format="csr"))
    monkeypatch.setattr(comm, "world_size", lambda: 2)
    for call in (lambda: MulticolorGaussSeidel(A),
                 lambda: greedy_coloring(A),
                 lambda: sgs_preconditioner(A, ordering="multicolor")):
        with pytest.raises(NotImplementedError, match="world size"):
            call()


# -- the preconditioner -----------------------------------------------------------
def test_matvec_is_permuted_sgs(poisson32):
    from sparse import darray
    from sparse.linalg import (LinearOperator, MulticolorGaussSeidel,
                               sgs_preconditioner)
    from sparse.trisolve import _SGSOperator

    assert type(sgs_preconditioner(poisson32)) is _SGSOperator
    M = sgs_preconditioner(poisson32, ordering="multicolor")
    assert isinstance(M, MulticolorGaussSeidel)
    assert isinstance(M, LinearOperator) and M.shape == (1024, 1024)
    S = poisson32.to_scipy_sparse_csr()
    order = M.order.cpu().numpy()
    for shape in [(1024,), (1024, 3)]:
        r = rhs(shape, np.float64)
        ref = sgs_oracle(S, order, r)
        assert np.allclose(np.asarray(M.matvec(r)), ref, **tol(np.float64))
        assert np.allclose(np.asarray(M.rmatvec(r)), ref, **tol(np.float64))
        out = darray.ones(shape)
        assert M.matvec(r, out=out) is out
        assert np.allclose(np.asarray(out), ref, **tol(np.float64))
    A = random_sym(np.complex128)
    M = MulticolorGaussSeidel(to_csr_array(A), seed=9)
    r = rhs((1500,), np.complex128)
    assert np.allclose(np.asarray(M.matvec(r)),
                       sgs_oracle(A, M.order.cpu().numpy(), r),
                       **tol(np.complex128))
    rd = darray.asdistarray(r.copy())  # out may alias r
    assert M.matvec(rd, out=rd) is rd
    assert np.allclose(np.asarray(rd),
                       sgs_oracle(A, M.order.cpu().numpy(), r),
                       **tol(np.complex128))


def test_multicolor_sgs_preconditioned_cg():
    """Multicolour-SGS CG on poisson2d(64, 64) converges to the tolerance in
    strictly fewer iterations than plain CG (scipy with the same
    preconditioner: 78 against 164)."""
    from sparse import gallery
    from sparse.linalg import cg, sgs_preconditioner

    A = gallery.poisson2d(64, 64)
    S = A.to_scipy_sparse_csr()
    b = np.ones(4096)

    def iterations(M):
        count = [0]

        def cb(_x):
            count[0] += 1

        x, info = cg(A, b, tol=1e-6, conv_test_iters=1, M=M, callback=cb)
        assert info == 0
        r = b - S @ np.asarray(x)
        # the recurrence residual met 1e-6 |b|; the true one differs from it
        # by rounding only
        assert np.linalg.norm(r) <= 1.001e-6 * np.linalg.norm(b)
        return count[0]

    plain = iterations(None)
    mc = iterations(sgs_preconditioner(A, ordering="multicolor"))
    print(f"CG iterations: plain {plain}, multicolour SGS {mc}")
    assert mc < plain


# -- the AMG example --------------------------------------------------------------
def _amg(*a):
    r = subprocess.run([sys.executable, os.path.join(EX, "amg.py"), *a],
                       capture_output=True, timeout=420)
    assert r.returncode == 0, \
        r.stdout.decode()[-1500:] + r.stderr.decode()[-1500:]
    out = r.stdout.decode()
    assert "info=0" in out, out
    return int(out.split("iters=")[1].split()[0])


def test_amg_gauss_seidel_smoother():
    gs = _amg("-n", "65536", "-maxiter", "100", "-smoother", "gs")
    jacobi = _amg("-n", "65536", "-maxiter", "100", "-smoother", "jacobi")
    print(f"AMG-CG iterations: jacobi {jacobi}, gs {gs}")
    assert gs <= jacobi
