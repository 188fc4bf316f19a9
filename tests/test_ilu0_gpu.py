"""ILU(0) factorisation kernels (ilu0.hip) vs the plain-Python reference —
all @gpu.

Same inputs, oracle and checks as test_ilu0.py (utils/ilu0_cases.py); here
the factorisation runs the level-scheduled kernels and every result has to
live on the device.
"""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

from utils.common import types
from utils.ilu0_cases import (case, case_names, case_ref, check_factor,
                              check_schedule, convection_diffusion, ilu0_ref,
                              ref_solve, to_scipy, tridiagonal)
from utils.trisolve_cases import rhs, tol

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _require_ext():
    if torch.cuda.is_available():
        from sparse.kernels import require

        require()


def _device_csr(A, idx="int32"):
    """csr_array of scipy A on the GPU with int32 or int64 column indices."""
    from sparse import csr_array

    Ad = csr_array(A)
    assert Ad._values.is_cuda and Ad._indices.dtype == torch.int32
    if idx == "int64":
        Ad = csr_array.from_local(Ad._indptr, Ad._indices.to(torch.int64),
                                  Ad._values, Ad.partition, Ad.shape)
    return Ad


def _ilu0(A, idx="int32"):
    from sparse.linalg import ilu0

    fac = ilu0(_device_csr(A, idx))
    assert fac._fvals.is_cuda and fac._diag_ptr.is_cuda
    assert fac.L._values.is_cuda and fac.U._values.is_cuda
    assert fac._Ls._values.is_cuda and fac._Us._values.is_cuda
    return fac


# -- 1. defining property, 3. schedule ------------------------------------------
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("name", case_names)
def test_defining_property_gpu(name, dt):
    A = case(name, dt)
    fac = _ilu0(A)
    assert fac.shape == A.shape and fac.dtype == np.dtype(dt)
    check_schedule(fac, name)
    check_factor(fac, A, exact=(name == "blocks"))


@pytest.mark.parametrize("dt", types)
def test_tridiagonal_is_exact_gpu(dt):
    A = tridiagonal(200, dt)
    check_factor(_ilu0(A), A, F=ilu0_ref(A).astype(dt), exact=True)


def test_poisson_gpu():
    from sparse import gallery
    from sparse.linalg import ilu0

    Ad = gallery.poisson2d(32, 32)
    assert Ad._values.is_cuda
    A = to_scipy(Ad)
    fac = ilu0(Ad)
    assert fac.schedule == [("chain", 0, 63)]
    assert fac.U._values.is_cuda
    check_factor(fac, A, F=ilu0_ref(A))


def test_a_is_not_modified_gpu():
    A = case("coupled")
    Ad = _device_csr(A)
    before = Ad._values.clone()
    from sparse.linalg import ilu0

    fac = ilu0(Ad)
    assert torch.equal(Ad._values, before)
    assert fac._fvals.data_ptr() != Ad._values.data_ptr()
    assert not any(k[0] == "ilu0" for k in Ad._plan_cache)


# -- 2. reference -----------------------------------------------------------------
@pytest.mark.parametrize("idx", ["int32", "int64"])
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("name", ["coupled", "band", "arrow"])
def test_matches_reference_gpu(name, dt, idx):
    A = case(name, dt)
    check_factor(_ilu0(A, idx), A, F=case_ref(name, dt))


def test_stored_zeros_are_part_of_the_pattern_gpu():
    dense = np.array([[4.0, 1.0, 2.0], [1.0, 5.0, 0.0], [2.0, 1.0, 6.0]])
    stored = sps.csr_matrix((np.array([4.0, 1, 2, 1, 5, 0, 2, 1, 6]),
                             np.tile(np.arange(3), 3), np.arange(0, 10, 3)),
                            shape=(3, 3))
    fs = _ilu0(stored)
    assert fs.nnz == 9
    Us = to_scipy(fs.U).toarray()
    assert np.isclose(Us[1, 2], -0.5)
    assert np.allclose(to_scipy(fs.L).toarray() @ Us, dense, rtol=1e-14)


# -- 4. solve ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", types)
def test_solve_matches_scipy_gpu(dt):
    fac = _ilu0(case("coupled", dt))
    F = case_ref("coupled", dt)
    n = F.shape[0]
    for shape in [(n,), (n, 3), (n, 33)]:
        r = rhs(shape, dt)
        z = fac.solve(r)
        assert z.local.is_cuda and z.shape == shape
        assert z.dtype == np.dtype(dt)
        assert np.allclose(np.asarray(z), ref_solve(F, r), **tol(dt))


def test_solve_out_may_alias_r_gpu():
    from sparse import asdistarray

    fac = _ilu0(case("band"))
    F = case_ref("band")
    for shape in [(1500,), (1500, 3)]:
        r = rhs(shape, np.float64)
        rd = asdistarray(r.copy())
        assert rd.local.is_cuda
        ptr = rd.local.data_ptr()
        assert fac.solve(rd, out=rd) is rd and rd.local.data_ptr() == ptr
        assert np.allclose(np.asarray(rd), ref_solve(F, r), **tol(np.float64))


def test_solve_dtype_promotes_gpu():
    fac = _ilu0(case("band", np.float32))
    F = case_ref("band", np.float32)
    for rdt in (np.float64, np.complex128):
        r = rhs((1500,), rdt)
        z = fac.solve(r)
        assert z.local.is_cuda and z.dtype == np.dtype(rdt)
        assert np.allclose(np.asarray(z), ref_solve(F, r), **tol(np.float32))


def test_non_default_stream_gpu():
    """Factorisation and solve enqueue on the current stream."""
    from sparse import asdistarray
    from sparse.linalg import ilu0

    A = case("arrow")
    F = case_ref("arrow")
    Ad = _device_csr(A)
    r = rhs((A.shape[0],), np.float64)
    rd = asdistarray(r)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fac = ilu0(Ad)
        z = fac.solve(rd)
    side.synchronize()
    check_factor(fac, A, F=F)
    assert np.allclose(np.asarray(z), ref_solve(F, r), **tol(np.float64))


# -- 5. refactor --------------------------------------------------------------------
def test_refactor_gpu():
    A = case("coupled")
    fac = _ilu0(A)
    L0, U0 = to_scipy(fac.L), to_scipy(fac.U)
    keep = (fac._Ls, fac._Us, fac._Ls._order, fac._Ls._level_ptr,
            fac._Us._order, fac._sched, fac._diag_ptr)
    assert fac.refactor(_device_csr(2.0 * A)) is fac
    assert fac.L._values.is_cuda
    L1, U1 = to_scipy(fac.L), to_scipy(fac.U)
    assert np.allclose(L1.data, L0.data, **tol(np.float64))
    assert np.allclose(U1.data, 2.0 * U0.data, **tol(np.float64))
    now = (fac._Ls, fac._Us, fac._Ls._order, fac._Ls._level_ptr,
           fac._Us._order, fac._sched, fac._diag_ptr)
    assert all(a is b for a, b in zip(keep, now))
    r = rhs((A.shape[0],), np.float64)
    assert np.allclose(np.asarray(fac.solve(r)),
                       ref_solve(case_ref("coupled"), r) / 2.0,
                       **tol(np.float64))
    with pytest.raises(ValueError):
        fac.refactor(_device_csr(case("blocks")))  # same shape, other pattern
    with pytest.raises(ValueError):
        fac.refactor(_device_csr(tridiagonal(200)))


# -- 6. errors ----------------------------------------------------------------------
def test_errors_gpu():
    from sparse import csr_array
    from sparse.linalg import ilu0

    missing = sps.csr_matrix(np.array([[1.0, 0, 0], [2.0, 0, 1.0], [0, 1, 3]]))
    with pytest.raises(np.linalg.LinAlgError, match="diagonal"):
        ilu0(_device_csr(missing))
    with pytest.raises(np.linalg.LinAlgError, match="row 1"):
        ilu0(_device_csr(sps.csr_matrix(np.ones((2, 2)))))
    with pytest.raises(ValueError):
        ilu0(csr_array(sps.random(4, 5, 0.5, random_state=0, format="csr")))
    ok = _device_csr(sps.csr_matrix(np.array([[2.0, 1.0], [1.0, 2.0]])))
    swapped = ok._indices.clone()
    swapped[:2] = swapped[:2].flip(0)
    with pytest.raises(ValueError, match="sorted"):
        ilu0(csr_array.from_local(ok._indptr, swapped, ok._values,
                                  ok.partition, ok.shape))


def test_tiny_gpu():
    from sparse import csr_array
    from sparse.linalg import ilu0

    f0 = ilu0(csr_array((0, 0)))
    assert f0.schedule == [] and f0.nnz == 0
    assert np.asarray(f0.solve(np.zeros(0))).shape == (0,)
    f1 = _ilu0(sps.csr_matrix(np.array([[4.0]])))
    assert f1.schedule == [("chain", 0, 1)]
    assert to_scipy(f1.U).toarray() == [[4.0]]
    assert np.allclose(np.asarray(f1.solve(np.array([2.0]))), [0.5])
    A = np.array([[4.0, 1.0, 0.0], [2.0, 5.0, 1.0], [0.0, 3.0, 6.0]])
    f3 = _ilu0(sps.csr_matrix(A))
    assert np.allclose(to_scipy(f3.L).toarray(),
                       [[1, 0, 0], [0.5, 1, 0], [0, 2 / 3, 1]], rtol=1e-15)
    assert np.allclose(to_scipy(f3.U).toarray(),
                       [[4, 1, 0], [0, 4.5, 1], [0, 0, 16 / 3]], rtol=1e-15)


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


def test_ilu0_preconditioned_cg_gpu():
    """Same bounds as the host test (measured there: 58 / 33 / 28)."""
    from sparse import gallery
    from sparse.linalg import cg, ilu0, sgs_preconditioner

    A = gallery.poisson2d(32, 32)
    assert A._values.is_cuda
    S = to_scipy(A)
    b = np.ones(1024)
    plain = _count(cg, A, S, b, None)
    sgs = _count(cg, A, S, b, sgs_preconditioner(A))
    ilu = _count(cg, A, S, b, ilu0(A))
    print(f"CG iterations on the GPU: plain {plain}, SGS {sgs}, ILU(0) {ilu}")
    assert ilu <= 0.6 * plain and ilu <= sgs


def test_ilu0_preconditioned_bicgstab_gpu():
    """Same bound as the host test (measured there: 60 / 13)."""
    from sparse.linalg import bicgstab, ilu0

    S = convection_diffusion(32, 40.0, 20.0)
    A = _device_csr(S)
    b = np.ones(1024)
    plain = _count(bicgstab, A, S, b, None)
    ilu = _count(bicgstab, A, S, b, ilu0(A))
    print(f"BiCGSTAB callbacks on the GPU: plain {plain}, ILU(0) {ilu}")
    assert ilu <= 0.5 * plain
