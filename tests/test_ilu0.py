"""ILU(0) factorisation and preconditioner vs a plain-Python IKJ reference
(host path).

Inputs and oracle: utils/ilu0_cases.py.  The GPU twin of this file is
test_ilu0_gpu.py.
"""
import numpy as np
import pytest
import scipy.sparse as sps

from utils.common import types
from utils.ilu0_cases import (case, case_names, case_ref, check_factor,
                              check_schedule, convection_diffusion, ilu0_ref,
                              ref_solve, to_scipy, tridiagonal)
from utils.trisolve_cases import rhs, tol


@pytest.fixture(scope="module")
def poisson32():
    from sparse import gallery

    return gallery.poisson2d(32, 32)


def _ilu0(A):
    from sparse import csr_array
    from sparse.linalg import ilu0

    return ilu0(csr_array(A))


# -- 1. defining property -------------------------------------------------------
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("name", case_names)
def test_defining_property(name, dt):
    A = case(name, dt)
    fac = _ilu0(A)
    assert fac.shape == A.shape and fac.dtype == np.dtype(dt)
    check_factor(fac, A, exact=(name == "blocks"))


@pytest.mark.parametrize("dt", types)
def test_tridiagonal_is_exact(dt):
    A = tridiagonal(200, dt)
    check_factor(_ilu0(A), A, F=ilu0_ref(A).astype(dt), exact=True)


def test_poisson(poisson32):
    from sparse.linalg import ilu0

    A = to_scipy(poisson32)
    fac = ilu0(poisson32)
    assert fac.schedule == [("chain", 0, 63)]
    check_factor(fac, A, F=ilu0_ref(A))


# -- 2. reference -----------------------------------------------------------------
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("name", ["coupled", "band", "arrow"])
def test_matches_reference(name, dt):
    A = case(name, dt)
    check_factor(_ilu0(A), A, F=case_ref(name, dt))


def test_numpy_fallback_agrees():
    from sparse.ilu import _ilu0_numpy

    for name in ("coupled", "nonsym"):
        A = case(name, np.complex128)
        v = A.data.copy()
        dp = np.flatnonzero(A.indices == np.repeat(np.arange(A.shape[0]),
                                                   np.diff(A.indptr)))
        bad = _ilu0_numpy(A.indptr.astype(np.int64), A.indices, v, dp)
        assert bad == A.shape[0]
        assert np.allclose(v, case_ref(name, np.complex128).data,
                           **tol(np.complex128))
    one = np.ones(4)
    assert _ilu0_numpy(np.array([0, 2, 4]), np.array([0, 1, 0, 1]), one,
                       np.array([0, 3])) == 1


def test_stored_zeros_are_part_of_the_pattern():
    """A stored zero takes fill that an absent entry would not."""
    dense = np.array([[4.0, 1.0, 2.0], [1.0, 5.0, 0.0], [2.0, 1.0, 6.0]])
    absent = sps.csr_matrix(dense)
    stored = sps.csr_matrix((np.array([4.0, 1, 2, 1, 5, 0, 2, 1, 6]),
                             np.tile(np.arange(3), 3), np.arange(0, 10, 3)),
                            shape=(3, 3))
    Ua = to_scipy(_ilu0(absent).U).toarray()
    fs = _ilu0(stored)
    assert fs.nnz == 9 and to_scipy(fs.U).nnz == 6
    Us = to_scipy(fs.U).toarray()
    assert Ua[1, 2] == 0.0 and np.isclose(Us[1, 2], -0.5)
    # with the position stored the pattern is full: the exact LU
    assert np.allclose(to_scipy(fs.L).toarray() @ Us, dense, rtol=1e-14)


# -- 3. schedule ------------------------------------------------------------------
@pytest.mark.parametrize("name", case_names)
def test_schedule(name):
    fac = _ilu0(case(name))
    check_schedule(fac, name)
    # the factorisation and the L solver share one level analysis
    assert fac.schedule == fac._Ls.schedule
    assert fac._sched.shape == fac._Ls._sched.shape


def test_level_pass_runs_once(monkeypatch):
    """One lower and one upper level pass per ilu0() call."""
    from sparse import kernels, trisolve

    calls = []

    def counting(real):
        def wrapped(indptr, indices, lower):
            calls.append(bool(lower))
            return real(indptr, indices, lower)
        return wrapped

    # the extension's pass and its numpy stand-in: whichever is in use
    monkeypatch.setattr(kernels, "trsv_levels", counting(kernels.trsv_levels))
    monkeypatch.setattr(trisolve, "_levels_numpy",
                        counting(trisolve._levels_numpy))
    fac = _ilu0(case("band"))
    assert sorted(calls) == [False, True]
    fac.refactor(_csr(case("band")))
    assert len(calls) == 2


def _csr(A):
    from sparse import csr_array

    return csr_array(A)


# -- 4. solve ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", types)
def test_solve_matches_scipy(dt):
    from sparse import DistArray

    fac = _ilu0(case("coupled", dt))
    F = case_ref("coupled", dt)
    n = F.shape[0]
    for shape in [(n,), (n, 3), (n, 33)]:
        r = rhs(shape, dt)
        z = fac.solve(r)
        assert isinstance(z, DistArray)
        assert z.shape == shape and z.dtype == np.dtype(dt)
        assert np.allclose(np.asarray(z), ref_solve(F, r), **tol(dt))


def test_solve_out_may_alias_r():
    from sparse import asdistarray, darray
    from sparse.linalg import LinearOperator

    fac = _ilu0(case("band"))
    F = case_ref("band")
    assert isinstance(fac, LinearOperator)
    for shape in [(1500,), (1500, 3)]:
        r = rhs(shape, np.float64)
        ref = ref_solve(F, r)
        rd = asdistarray(r.copy())
        assert fac.solve(rd, out=rd) is rd
        assert np.allclose(np.asarray(rd), ref, **tol(np.float64))
        out = darray.zeros(shape)
        assert fac.matvec(r, out=out) is out
        assert np.allclose(np.asarray(out), ref, **tol(np.float64))
    with pytest.raises(ValueError):
        fac.solve(np.ones(7))
    with pytest.raises(NotImplementedError):
        fac.rmatvec(np.ones(1500))


def test_solve_dtype_promotes():
    """A float32 factor with a float64 (or complex) r solves in the promoted
    dtype; the factor keeps float32 accuracy."""
    fac = _ilu0(case("band", np.float32))
    F = case_ref("band", np.float32)
    for rdt in (np.float64, np.complex128):
        r = rhs((1500,), rdt)
        z = fac.solve(r)
        assert z.dtype == np.dtype(rdt)
        assert np.allclose(np.asarray(z), ref_solve(F, r), **tol(np.float32))


# -- 5. refactor --------------------------------------------------------------------
def test_refactor():
    A = case("coupled")
    fac = _ilu0(A)
    L0, U0 = to_scipy(fac.L), to_scipy(fac.U)
    keep = (fac._Ls, fac._Us, fac._Ls._order, fac._Ls._level_ptr,
            fac._Us._order, fac._sched, fac._diag_ptr)
    assert fac.refactor(_csr(2.0 * A)) is fac
    L1, U1 = to_scipy(fac.L), to_scipy(fac.U)
    assert np.allclose(L1.data, L0.data, **tol(np.float64))
    assert np.allclose(U1.data, 2.0 * U0.data, **tol(np.float64))
    now = (fac._Ls, fac._Us, fac._Ls._order, fac._Ls._level_ptr,
           fac._Us._order, fac._sched, fac._diag_ptr)
    assert all(a is b for a, b in zip(keep, now))
    # the solvers apply the new factors
    r = rhs((A.shape[0],), np.float64)
    assert np.allclose(np.asarray(fac.solve(r)),
                       ref_solve(case_ref("coupled"), r) / 2.0,
                       **tol(np.float64))


def test_refactor_structure_mismatch():
    fac = _ilu0(case("band"))
    with pytest.raises(ValueError):
        fac.refactor(_csr(case("nonsym")))          # same shape, other pattern
    with pytest.raises(ValueError):
        fac.refactor(_csr(tridiagonal(200)))        # other shape
    with pytest.raises(ValueError):
        fac.refactor(_csr(case("band", np.float32)))  # other dtype


# -- 6. errors ----------------------------------------------------------------------
def test_errors():
    from sparse import csr_array
    from sparse.linalg import ilu0

    missing = sps.csr_matrix(np.array([[1.0, 0, 0], [2.0, 0, 1.0], [0, 1, 3]]))
    with pytest.raises(np.linalg.LinAlgError, match="diagonal"):
        ilu0(csr_array(missing))
    with pytest.raises(np.linalg.LinAlgError, match="row 1"):
        ilu0(csr_array(sps.csr_matrix(np.ones((2, 2)))))
    with pytest.raises(ValueError):
        ilu0(csr_array(sps.random(4, 5, 0.5, random_state=0, format="csr")))
    ok = csr_array(sps.csr_matrix(np.array([[2.0, 1.0], [1.0, 2.0]])))
    swapped = ok._indices.clone()
    swapped[:2] = swapped[:2].flip(0)
    with pytest.raises(ValueError, match="sorted"):
        ilu0(csr_array.from_local(ok._indptr, swapped, ok._values,
                                  ok.partition, ok.shape))
    dup = ok._indices.clone()
    dup[0] = 1
    with pytest.raises(ValueError, match="duplicate"):
        ilu0(csr_array.from_local(ok._indptr, dup, ok._values, ok.partition,
                                  ok.shape))


def test_world_size_above_one_raises(monkeypatch):
    from sparse import csr_array
    from sparse.linalg import ilu0
    from sparse.parallel import comm

    A = csr_array(sps.identity(4, format="csr"))
    monkeypatch.setattr(comm, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size"):
        ilu0(A)


def test_tiny():
    from sparse import csr_array
    from sparse.linalg import ilu0

    f0 = ilu0(csr_array((0, 0)))
    assert f0.schedule == [] and f0.nnz == 0 and f0.shape == (0, 0)
    assert np.asarray(f0.solve(np.zeros(0))).shape == (0,)
    assert to_scipy(f0.L).shape == (0, 0)
    f1 = ilu0(csr_array(sps.csr_matrix(np.array([[4.0]]))))
    assert f1.schedule == [("chain", 0, 1)]
    assert to_scipy(f1.L).toarray() == [[1.0]]
    assert to_scipy(f1.U).toarray() == [[4.0]]
    assert np.allclose(np.asarray(f1.solve(np.array([2.0]))), [0.5])
    A = np.array([[4.0, 1.0, 0.0], [2.0, 5.0, 1.0], [0.0, 3.0, 6.0]])
    f3 = ilu0(csr_array(sps.csr_matrix(A)))
    assert np.allclose(to_scipy(f3.L).toarray(),
                       [[1, 0, 0], [0.5, 1, 0], [0, 2 / 3, 1]], rtol=1e-15)
    assert np.allclose(to_scipy(f3.U).toarray(),
                       [[4, 1, 0], [0, 4.5, 1], [0, 0, 16 / 3]], rtol=1e-15)
    assert np.allclose(np.asarray(f3.solve(A @ np.array([1.0, 2.0, 3.0]))),
                       [1.0, 2.0, 3.0], rtol=1e-14)


def test_other_input_kinds():
    """Anything _as_csr accepts: scipy matrices and other formats."""
    from sparse import csc_array
    from sparse.linalg import ilu0

    A = case("band")
    F = case_ref("band")
    for M in (A, csc_array(A.tocsc())):
        fac = ilu0(M)
        assert np.allclose(to_scipy(fac.U).data, sps.triu(F).tocsr().data,
                           **tol(np.float64))


# -- 7. preconditioning -------------------------------------------------------------
def _count(solver, A, S, b, M):
    count = [0]

    def cb(_x):
        count[0] += 1

    x, info = solver(A, b, tol=1e-8, conv_test_iters=1, M=M, callback=cb)
    assert info == 0
    r = b - S @ np.asarray(x)
    assert np.linalg.norm(r) <= 1e-7 * np.linalg.norm(b)
    return count[0]


def test_ilu0_preconditioned_cg(poisson32):
    """CPU measurement behind the bounds: plain 58, SGS 33, ILU(0) 28."""
    from sparse.linalg import cg, ilu0, sgs_preconditioner

    S = to_scipy(poisson32)
    b = np.ones(1024)
    plain = _count(cg, poisson32, S, b, None)
    sgs = _count(cg, poisson32, S, b, sgs_preconditioner(poisson32))
    ilu = _count(cg, poisson32, S, b, ilu0(poisson32))
    print(f"CG iterations: plain {plain}, SGS {sgs}, ILU(0) {ilu}")
    assert ilu <= 0.6 * plain and ilu <= sgs


def test_ilu0_preconditioned_bicgstab():
    """CPU measurement behind the bound: plain 60 callbacks, ILU(0) 13."""
    from sparse import csr_array
    from sparse.linalg import bicgstab, ilu0

    S = convection_diffusion(32, 40.0, 20.0)
    A = csr_array(S)
    b = np.ones(1024)
    plain = _count(bicgstab, A, S, b, None)
    ilu = _count(bicgstab, A, S, b, ilu0(A))
    print(f"BiCGSTAB callbacks: plain {plain}, ILU(0) {ilu}")
    assert ilu <= 0.5 * plain
