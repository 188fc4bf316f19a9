"""FSAI preconditioner vs the plain numpy oracle (host path).

Inputs, oracle and checks: utils/fsai_cases.py.  The GPU twin of this file is
test_fsai_gpu.py.
"""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

from utils.common import types
from utils.fsai_cases import (apply_ref, case, case_names, case_ref,
                              check_fsai, lower_pattern, row_lengths, to_scipy)
from utils.trisolve_cases import rhs, tol


def _csr(A, idx="int32"):
    """csr_array of scipy A with int32 or int64 column indices."""
    from sparse import csr_array

    Ad = csr_array(A)
    if idx == "int64":
        Ad = csr_array.from_local(Ad._indptr, Ad._indices.to(torch.int64),
                                  Ad._values, Ad.partition, Ad.shape)
    return Ad


def _fsai(A, idx="int32", **kw):
    from sparse.linalg import fsai

    if kw.get("pattern") is not None:
        kw["pattern"] = _csr(kw["pattern"], idx)
    return fsai(_csr(A, idx), **kw)


# -- 1. defining properties, 2. reference -----------------------------------------
@pytest.mark.parametrize("idx", ["int32", "int64"])
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("name", case_names)
def test_properties_and_reference(name, dt, idx):
    A = case(name, dt)
    P, ref = case_ref(name, dt)
    fac = _fsai(A, idx)
    assert fac.G._indices.dtype == getattr(torch, idx)
    check_fsai(fac, A, P, ref=ref, exact=(name == "blocks"))


def test_cases_reach_every_bucket_cut():
    """stair and arrow hold a row at, and a row one past, every cut."""
    from sparse.fsai import FSAI_CUTS, FSAI_LDS_ROW, FSAI_MAX_ROW

    assert FSAI_MAX_ROW >= 1024 and FSAI_LDS_ROW in FSAI_CUTS
    assert list(FSAI_CUTS) == sorted(set(FSAI_CUTS))
    have = row_lengths()
    for cut in FSAI_CUTS:
        assert cut in have and cut + 1 in have, cut
    assert max(have) > FSAI_LDS_ROW
    fac = _fsai(case("stair"))
    lengths = np.diff(lower_pattern(case("stair")).indptr)
    lo, want = 0, []
    for cut in FSAI_CUTS:
        want.append((cut, int(((lengths > lo) & (lengths <= cut)).sum())))
        lo = cut
    want.append((0, int((lengths > lo).sum())))
    assert fac.row_classes == want


# -- 3. triangle -------------------------------------------------------------------
@pytest.mark.parametrize("dt", types)
def test_only_the_lower_triangle_is_read(dt):
    A = case("band", dt)
    G = to_scipy(_fsai(A).G)
    low = sps.tril(A).tocsr()
    low.sort_indices()
    Gl = to_scipy(_fsai(low).G)
    assert np.array_equal(G.indices, Gl.indices)
    assert np.array_equal(G.data, Gl.data)


def test_a_wrong_upper_triangle_is_ignored():
    A = case("band", np.complex128)
    junk = sps.random(A.shape[0], A.shape[0], 0.004, random_state=3)
    B = (A + sps.triu(junk, 1) * (2.0 - 3.0j)).tocsr()
    B.sort_indices()
    assert abs(B - B.conj().T).max() > 1.0
    G = to_scipy(_fsai(A).G)
    Gb = to_scipy(_fsai(B).G)
    assert np.array_equal(G.indices, Gb.indices)
    assert np.array_equal(G.data, Gb.data)


def test_a_is_not_modified():
    from sparse.linalg import fsai

    Ad = _csr(case("band"))
    before = Ad._values.clone()
    fac = fsai(Ad)
    assert torch.equal(Ad._values, before)
    assert fac.G._values.data_ptr() != Ad._values.data_ptr()
    assert not any(k[0] == "fsai" for k in Ad._plan_cache)


# -- 4. patterns -------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.complex64])
def test_power_2_on_the_stencil(dt):
    A = case("stencil", dt)
    P, ref = case_ref("stencil", dt, 2)
    AA = sps.tril(A @ A).tocsr()
    AA.sort_indices()
    assert np.array_equal(P.indptr, AA.indptr)
    assert np.array_equal(P.indices, AA.indices)
    assert np.diff(P.indptr).max() == 7
    fac = _fsai(A, power=2)
    assert fac.max_row == 7
    check_fsai(fac, A, P, ref=ref)


def test_pattern_argument_gets_its_diagonal():
    A = case("band")
    n = A.shape[0]
    pat = sps.random(n, n, 0.004, random_state=9, format="csr")
    pat = (pat + sps.diags((np.arange(n) % 3 == 0).astype(float))).tocsr()
    assert 0 < (pat.diagonal() != 0).sum() < n
    P = lower_pattern(pat)
    assert np.all(P.diagonal() == 1.0)
    fac = _fsai(A, pattern=pat)
    check_fsai(fac, A, P)
    with pytest.raises(ValueError):
        _fsai(A, pattern=pat, power=2)
    with pytest.raises(ValueError):
        _fsai(A, pattern=sps.identity(n + 1, format="csr"))
    with pytest.raises(ValueError):
        _fsai(A, power=0)


def test_row_longer_than_the_limit():
    from sparse import fsai as mod

    n = mod.FSAI_MAX_ROW + 8
    last = sps.csr_matrix((np.ones(n), (np.full(n, n - 1), np.arange(n))),
                          shape=(n, n))
    A = (sps.identity(n) * float(n) + sps.tril(last, -1)).tocsr()
    with pytest.raises(ValueError, match=rf"row {n - 1} .* {n} entries"):
        _fsai(A)


# -- 5. apply ----------------------------------------------------------------------
@pytest.mark.parametrize("dt", types)
def test_solve_matches_scipy(dt):
    A = case("band", dt)
    fac = _fsai(A)
    G = to_scipy(fac.G)
    n = A.shape[0]
    for shape in [(n,), (n, 3), (n, 33)]:
        r = rhs(shape, dt)
        z = fac.solve(r)
        assert z.shape == shape and z.dtype == np.dtype(dt)
        assert np.allclose(np.asarray(z), apply_ref(G, r), **tol(dt))
        assert np.allclose(np.asarray(fac.matvec(r)), np.asarray(z))
        assert np.allclose(np.asarray(fac.rmatvec(r)), np.asarray(z))


def test_solve_out_may_alias_r():
    from sparse import asdistarray

    fac = _fsai(case("band"))
    G = to_scipy(fac.G)
    for shape in [(1500,), (1500, 3)]:
        r = rhs(shape, np.float64)
        rd = asdistarray(r.copy())
        ptr = rd.local.data_ptr()
        assert fac.solve(rd, out=rd) is rd and rd.local.data_ptr() == ptr
        assert np.allclose(np.asarray(rd), apply_ref(G, r),
                           **tol(np.float64))
        tmp = dict(fac._tmp)
        fac.solve(rd, out=rd)  # the G r buffer is kept per shape and dtype
        assert fac._tmp.keys() == tmp.keys()
        assert all(fac._tmp[k] is v for k, v in tmp.items())


@pytest.mark.parametrize("dt", [np.float64, np.complex128])
def test_operator_is_hermitian_positive_definite(dt):
    fac = _fsai(case("wide", dt))
    n = fac.shape[0]
    r, s = rhs((n,), dt, seed=1), rhs((n,), dt, seed=2)
    Mr, Ms = np.asarray(fac.solve(r)), np.asarray(fac.solve(s))
    rMr = np.vdot(r, Mr)
    assert rMr.real > 0 and abs(rMr.imag) <= 1e-12 * rMr.real
    assert np.isclose(np.vdot(s, Mr), np.conj(np.vdot(r, Ms)), rtol=1e-10)


# -- 6. refactor -------------------------------------------------------------------
def test_refactor():
    A = case("band")
    fac = _fsai(A)
    G0 = to_scipy(fac.G)
    r = rhs((A.shape[0],), np.float64)
    z0 = np.asarray(fac.solve(r))  # builds whatever SpMV mirrors G gets
    keep = (fac.G, fac.GH, fac.G._indptr, fac.G._indices, fac.GH._indptr,
            fac.GH._indices, fac.G._values, fac.GH._values, fac._perm)
    assert fac.refactor(_csr(2.0 * A)) is fac
    now = (fac.G, fac.GH, fac.G._indptr, fac.G._indices, fac.GH._indptr,
           fac.GH._indices, fac.G._values, fac.GH._values, fac._perm)
    assert all(a is b for a, b in zip(keep, now))
    G1 = to_scipy(fac.G)
    assert np.allclose(G1.data, G0.data / np.sqrt(2.0), **tol(np.float64))
    check_fsai(fac, (2.0 * A).tocsr(), lower_pattern(A))
    assert np.allclose(np.asarray(fac.solve(r)), z0 / 2.0, **tol(np.float64))
    with pytest.raises(ValueError):
        fac.refactor(_csr(case("band", np.float32)))
    other = (A + sps.diags(np.ones(A.shape[0] - 40), -40)).tocsr()
    with pytest.raises(ValueError):
        fac.refactor(_csr(other))  # same shape, other pattern
    with pytest.raises(ValueError):
        fac.refactor(_csr(case("stair")))


# -- 7. errors ---------------------------------------------------------------------
def test_errors():
    from sparse import csr_array

    with pytest.raises(np.linalg.LinAlgError, match="row 1"):
        _fsai(sps.csr_matrix(np.array([[1.0, 2.0], [2.0, 1.0]])))
    missing = sps.csr_matrix(np.array([[1.0, 0, 0], [0.5, 0, 0.5],
                                       [0, 0.5, 3]]))
    with pytest.raises(np.linalg.LinAlgError, match="row 1"):
        _fsai(missing)
    with pytest.raises(ValueError):
        _fsai(csr_array(sps.random(4, 5, 0.5, random_state=0, format="csr")))
    fac = _fsai(case("band"))
    bad = case("band").copy()
    bad.data[bad.indptr[700]: bad.indptr[701]] *= -1.0
    with pytest.raises(np.linalg.LinAlgError, match="row 700"):
        fac.refactor(_csr(bad))
    fac.refactor(_csr(case("band")))  # usable again
    check_fsai(fac, case("band"), lower_pattern(case("band")))


def test_tiny():
    from sparse import csr_array
    from sparse.linalg import fsai

    f0 = fsai(csr_array((0, 0)))
    assert f0.nnz == 0 and f0.max_row == 0 and f0.row_classes == []
    assert np.asarray(f0.solve(np.zeros(0))).shape == (0,)
    f1 = _fsai(sps.csr_matrix(np.array([[4.0]])))
    assert to_scipy(f1.G).toarray() == [[0.5]]
    assert np.allclose(np.asarray(f1.solve(np.array([2.0]))), [0.5])
    A = np.array([[4.0, 2.0], [2.0, 5.0]])
    f2 = _fsai(sps.csr_matrix(A))  # the full lower pattern: G = C^-1
    C = np.linalg.cholesky(A)
    assert np.allclose(to_scipy(f2.G).toarray(), np.linalg.inv(C), rtol=1e-14)
    assert np.allclose(np.asarray(f2.solve(np.array([1.0, 3.0]))),
                       np.linalg.solve(A, [1.0, 3.0]), rtol=1e-14)


# -- 8. preconditioning ------------------------------------------------------------
def _count(solver, A, S, b, M):
    count = [0]

    def cb(_x):
        count[0] += 1

    x, info = solver(A, b, tol=1e-8, conv_test_iters=1, M=M, callback=cb)
    assert info == 0
    r = b - S @ np.asarray(x)
    assert np.linalg.norm(r) <= 1e-7 * np.linalg.norm(b)
    return count[0]


def test_fsai_preconditioned_cg():
    """Measured on the host path: 58 / 43 / 34 / 26."""
    from sparse import gallery
    from sparse.linalg import cg, fsai

    A = gallery.poisson2d(32, 32)
    S = to_scipy(A)
    b = np.ones(1024)
    plain = _count(cg, A, S, b, None)
    p1 = _count(cg, A, S, b, fsai(A))
    p2 = _count(cg, A, S, b, fsai(A, power=2))
    p3 = _count(cg, A, S, b, fsai(A, power=3))
    print(f"CG iterations: plain {plain}, FSAI power 1 / 2 / 3: "
          f"{p1} / {p2} / {p3}")
    assert p1 <= 0.8 * plain
    assert p2 <= 0.65 * plain and p2 <= p1
    assert p3 <= p2


def test_fsai_preconditioned_bicgstab():
    """Converges (info 0, residual checked against scipy in _count)."""
    from sparse import gallery
    from sparse.linalg import bicgstab, fsai

    A = gallery.poisson2d(32, 32)
    S = to_scipy(A)
    b = np.ones(1024)
    plain = _count(bicgstab, A, S, b, None)
    pre = _count(bicgstab, A, S, b, fsai(A, power=2))
    print(f"BiCGSTAB callbacks: plain {plain}, FSAI power 2 {pre}")
