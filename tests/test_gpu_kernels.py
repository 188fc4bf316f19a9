"""HIP kernel numerics vs CPU fp64/scipy oracle — all @gpu.

Each test builds the operands on CPU (scipy/torch reference), moves them to
cuda:0 through the sparse API, and compares.  The GPU path requires the
in-tree HIP extension (sparse.kernels.require()); these tests fail — not
skip — if it is missing on a GPU box.
"""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

from utils.common import types
from utils.sample import sample_csr, sample_dense, spd_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _require_ext():
    if torch.cuda.is_available():
        from sparse.kernels import require

        require()


def tol(dt):
    if np.dtype(dt) in (np.float32, np.complex64):
        return dict(rtol=2e-4, atol=2e-5)
    return dict(rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("shape", [(64, 80), (500, 300), (1000, 1000)])
def test_spmv_gpu(dt, shape):
    from sparse import csr_array

    s = sample_csr(*shape, 0.05, seed=1, dtype=dt)
    x = sample_dense(shape[1], seed=2, dtype=dt)
    A = csr_array(s)
    assert A._values.is_cuda
    y = A @ x
    assert np.allclose(np.asarray(y), s @ x, **tol(dt))


def test_spmv_long_row_carry_gpu():
    # one row with 100k nnz spans many 2048-nnz blocks: exercises the carry path
    from sparse import csr_array

    rng = np.random.default_rng(3)
    n = 200_000
    cols = np.unique(rng.integers(0, n, 100_000))
    rows = np.zeros(len(cols), dtype=np.int64)
    extra_r = np.arange(1, 50)
    extra_c = rng.integers(0, n, 49)
    data = np.concatenate([rng.random(len(cols)), rng.random(49)])
    i = np.concatenate([rows, extra_r])
    j = np.concatenate([cols, extra_c])
    s = sps.csr_matrix((data, (i, j)), shape=(50, n))
    x = rng.random(n)
    A = csr_array(s)
    assert np.allclose(np.asarray(A @ x), s @ x, rtol=1e-10, atol=1e-9)


@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("k", [3, 8, 33])
def test_spmm_gpu(dt, k):
    """k<=32 takes the small-k lane-tiled kernel; k=33 the wide kernel."""
    from sparse import csr_array

    s = sample_csr(300, 200, 0.05, seed=4, dtype=dt)
    B = sample_dense((200, k), seed=5, dtype=dt)
    assert np.allclose(np.asarray(csr_array(s) @ B), s @ B, **tol(dt))


def test_ell_ranged_split_gpu():
    """Ranged ELL SpMV/dot (the ws>1 interior/boundary overlap split):
    three range launches must reproduce the full kernel exactly, and
    ell_interior must return a valid even interior run."""
    import scipy.sparse as sps

    from sparse import csr_array, kernels

    n = 5000
    rng = np.random.default_rng(51)
    W = 6
    rows = np.repeat(np.arange(n), W)
    cols = (rows + rng.integers(-30, 31, n * W)) % n
    s = sps.csr_matrix((rng.random(n * W), (rows, cols)), shape=(n, n))
    s.sum_duplicates()
    A = csr_array(s)
    ell = A._ell()
    assert ell is not None and ell.rmin is not None
    x = torch.as_tensor(rng.random(n), device="cuda")
    pieces = (x[:0], x, x[:0])
    y_full = torch.empty(n, dtype=torch.float64, device="cuda")
    kernels.ell_spmv(ell, pieces, y_full, 0)
    # split at an arbitrary even cut pair
    a, b = 1024, 3072
    y_split = torch.empty(n, dtype=torch.float64, device="cuda")
    kernels.ell_spmv(ell, pieces, y_split, 0, a, b)
    kernels.ell_spmv(ell, pieces, y_split, 0, 0, a)
    kernels.ell_spmv(ell, pieces, y_split, 0, b, -1)
    assert torch.equal(y_full, y_split)
    p = torch.as_tensor(rng.random(n), device="cuda")
    q1 = torch.empty_like(y_full)
    d_full = kernels.ell_spmv_dot(ell, pieces, q1, p, 0)
    q2 = torch.empty_like(y_full)
    d_split = (kernels.ell_spmv_dot(ell, pieces, q2, p, 0, a, b)
               + kernels.ell_spmv_dot(ell, pieces, q2, p, 0, 0, a)
               + kernels.ell_spmv_dot(ell, pieces, q2, p, 0, b, -1))
    assert torch.equal(q1, q2)
    assert torch.allclose(d_full, d_split, rtol=1e-12)
    # interior run over a mid-window piece: valid even bounds, all rows'
    # windows inside
    ia, ib = kernels.ell_interior(ell, 1000, 4000)
    if ib > ia:
        assert ia % 2 == 0 and ib % 2 == 0
        assert bool((ell.rmin[ia:ib] >= 1000).all())
        assert bool((ell.rmax[ia:ib] < 4000).all())


@pytest.mark.parametrize("dt", types)
def test_dense_to_csr_kernel_gpu(dt):
    """Two-phase ballot-compaction dense->CSR kernel (reference
    dense_to_csr.cu parity, VERDICT r1 partial closed): ordered columns,
    all dtypes, wide rows (>64 cols), empty rows, and the csr_array
    constructor path."""
    import scipy.sparse as sps

    from sparse import csr_array
    from sparse.ops import local as L

    rng = np.random.default_rng(41)
    d = rng.random((37, 201))
    d[d < 0.8] = 0.0
    d[5, :] = 0.0  # empty row
    d[6, :] = 1.0  # dense row
    if np.dtype(dt).kind == "c":
        d = d + 1j * (d != 0)
    d = d.astype(dt)
    dd = torch.as_tensor(d, device="cuda")
    lc = L.dense_to_csr(dd)
    ref = sps.csr_matrix(d)
    ref.sort_indices()
    assert (lc.indptr.cpu().numpy() == ref.indptr).all()
    assert (lc.indices.cpu().numpy() == ref.indices).all()
    assert np.allclose(lc.values.cpu().numpy(), ref.data)
    # constructor end-to-end
    A = csr_array(d)
    assert np.allclose(np.asarray(A.todense()), d)


def test_segmented_coo_to_csr_gpu(monkeypatch):
    """The scatter + per-row LDS sort conversion kernel (VERDICT r1 #9;
    opt-in after the measured A/B in profiles/CONV_r02.md): scattered
    input, duplicate (i,j) pairs (summed via fallback), a >1024-nnz row
    (overflow fallback), complex dtype, and tocsc."""
    monkeypatch.setenv("SPARSE_SEGMENTED_CONV", "1")
    import scipy.sparse as sps

    from sparse import coo_array, csr_array

    rng = np.random.default_rng(31)
    n = 400
    s = sps.random(n, n, 0.05, random_state=32, format="coo")
    perm = rng.permutation(s.nnz)
    A = coo_array((s.data[perm], (s.row[perm], s.col[perm])), shape=s.shape)
    ref = s.tocsr()
    ref.sort_indices()
    got = A.tocsr().to_scipy_sparse_csr()
    assert (got.indptr == ref.indptr).all()
    assert (got.indices == ref.indices).all()
    assert np.allclose(got.data, ref.data)
    # duplicates -> summed (scipy semantics), kernel flags + falls back
    i2 = np.array([0, 0, 1, 0, 2]); j2 = np.array([3, 3, 1, 3, 2])
    v2 = np.array([1.0, 2.0, 5.0, 4.0, 6.0])
    got2 = coo_array((v2, (i2, j2)), shape=(4, 4)).tocsr()
    ref2 = sps.coo_matrix((v2, (i2, j2)), shape=(4, 4)).tocsr()
    assert np.allclose(np.asarray(got2.todense()), ref2.toarray())
    # one huge row (> 1024 nnz) -> overflow fallback
    jj = rng.permutation(3000)[:2000]
    big = sps.coo_matrix((rng.random(2000), (np.zeros(2000, int), jj)),
                         shape=(4, 3000))
    gotb = coo_array((big.data, (big.row, big.col)), shape=big.shape).tocsr()
    refb = big.tocsr(); refb.sort_indices()
    gb = gotb.to_scipy_sparse_csr()
    assert (gb.indices == refb.indices).all() and np.allclose(gb.data, refb.data)
    # complex + tocsc
    sc = sps.random(120, 90, 0.08, random_state=33).astype(np.complex128)
    sc.data = sc.data + 1j * rng.random(sc.nnz)
    gc = csr_array(sc.tocsr()).tocsc()
    refc = sc.tocsc()
    assert np.allclose(np.asarray(gc.todense()), refc.toarray())


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("k", [16, 32, 40])
def test_bsr_mfma_spmm_gpu(dt, k):
    """The MFMA 16x16-block SpMM path (profiles/MFMA_r02.md): a banded
    matrix with dense-ish blocks must take the BSR mirror and match
    scipy; white-box asserts the mirror was built and selected."""
    import scipy.sparse as sps

    from sparse import csr_array, kernels

    n = 512
    # tridiagonal band: 46/256 on the diagonal blocks + 1/256 corner
    # blocks -> overall fill ~6.4%, inside the k<=32 win region
    s = sps.diags([np.ones(n - 1), 4 * np.ones(n), np.ones(n - 1)],
                  [-1, 0, 1], format="csr").astype(dt)
    A = csr_array(s)
    B = sample_dense((n, k), seed=9, dtype=dt)
    out = np.asarray(A @ B)
    bm = A._bsr()
    assert bm is not None and 0.05 < bm.fill < 0.08
    assert kernels.bsr_profitable(bm, k) == (k <= 32)
    assert np.allclose(out, s @ B, **tol(dt))
    # fully dense 16x16 blocks (fill 1.0): profitable at every k
    sd = sps.kron(sps.diags([np.ones(7)], [0]),
                  np.arange(256).reshape(16, 16) * 0.01 + 1).tocsr().astype(dt)
    Ad = csr_array(sd)
    Bd = sample_dense((sd.shape[1], k), seed=12, dtype=dt)
    outd = np.asarray(Ad @ Bd)
    bmd = Ad._bsr()
    assert bmd is not None and bmd.fill == 1.0
    assert kernels.bsr_profitable(bmd, k)
    assert np.allclose(outd, sd @ Bd, **tol(dt))
    # scattered matrix: mirror must refuse (fill too low), fallback path
    s2 = sample_csr(300, 400, 0.01, seed=10, dtype=dt)
    A2 = csr_array(s2)
    B2 = sample_dense((400, k), seed=11, dtype=dt)
    assert np.allclose(np.asarray(A2 @ B2), s2 @ B2, **tol(dt))


@pytest.mark.parametrize("dt", [np.float64, np.complex128])
def test_rspmm_gpu(dt):
    from sparse import csr_array

    s = sample_csr(150, 120, 0.08, seed=6, dtype=dt)
    A = sample_dense((7, 150), seed=7, dtype=dt)
    assert np.allclose(np.asarray(A @ csr_array(s)), A @ s, **tol(dt))


@pytest.mark.parametrize("dt", types)
def test_add_gpu(dt):
    from sparse import csr_array

    a = sample_csr(400, 300, 0.03, seed=8, dtype=dt)
    b = sample_csr(400, 300, 0.03, seed=9, dtype=dt)
    c = csr_array(a) + csr_array(b)
    assert np.allclose(np.asarray(c.todense()), (a + b).toarray(), **tol(dt))


@pytest.mark.parametrize("dt", types)
def test_elem_mult_gpu(dt):
    from sparse import csr_array

    a = sample_csr(300, 300, 0.05, seed=10, dtype=dt)
    b = sample_csr(300, 300, 0.05, seed=11, dtype=dt)
    c = csr_array(a).multiply(csr_array(b))
    assert np.allclose(np.asarray(c.todense()), a.multiply(b).toarray(), **tol(dt))


@pytest.mark.parametrize("dt", [np.float64, np.complex128])
def test_mult_dense_gpu(dt):
    from sparse import csr_array

    a = sample_csr(120, 90, 0.1, seed=12, dtype=dt)
    d = sample_dense((120, 90), seed=13, dtype=dt)
    c = csr_array(a).multiply(d)
    assert np.allclose(np.asarray(c.todense()), a.multiply(d).toarray(), **tol(dt))


@pytest.mark.parametrize("dt", types)
def test_spgemm_gpu(dt):
    from sparse import csr_array

    a = sample_csr(200, 150, 0.05, seed=14, dtype=dt)
    b = sample_csr(150, 180, 0.05, seed=15, dtype=dt)
    c = csr_array(a) @ csr_array(b)
    assert np.allclose(np.asarray(c.todense()), (a @ b).toarray(), **tol(dt))


def test_spgemm_dense_row_fallback_gpu():
    # a row whose product has > 1024 distinct columns must take the ESC path
    from sparse import csr_array

    rng = np.random.default_rng(16)
    n = 3000
    a = sps.random(50, 40, 0.2, random_state=17).tocsr()
    a[0, :] = 1.0  # dense row -> C row 0 hits most of B's columns
    a = a.tocsr()
    b = sps.random(40, n, 0.2, random_state=18).tocsr()
    c = csr_array(a) @ csr_array(b)
    assert c.nnz == (a @ b).nnz
    assert np.allclose(np.asarray(c.todense()), (a @ b).toarray(), rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("dt", [np.float64])
def test_sddmm_gpu(dt):
    from sparse import csr_array

    s = sample_csr(90, 110, 0.1, seed=19, dtype=dt)
    C = sample_dense((90, 8), seed=20, dtype=dt)
    D = sample_dense((8, 110), seed=21, dtype=dt)
    out = csr_array(s).sddmm(C, D)
    assert np.allclose(np.asarray(out.todense()), s.multiply(C @ D).toarray(), **tol(dt))


@pytest.mark.parametrize("dt", types)
def test_csc_spmv_gpu(dt):
    from sparse import csc_array

    s = sample_csr(130, 170, 0.06, seed=22, dtype=dt)
    x = sample_dense(170, seed=23, dtype=dt)
    A = csc_array(s.tocsc())
    assert np.allclose(np.asarray(A @ x), s @ x, **tol(dt))


def test_conversions_gpu():
    from sparse import csr_array

    s = sample_csr(200, 160, 0.05, seed=24)
    A = csr_array(s)
    assert np.allclose(np.asarray(A.todense()), s.toarray())
    assert np.allclose(np.asarray(A.tocsc().todense()), s.toarray())
    assert np.allclose(np.asarray(A.tocoo().tocsr().todense()), s.toarray())
    assert np.allclose(np.asarray(A.diagonal()), s.diagonal())


def test_axpby_gpu():
    from sparse import darray
    from sparse.linalg import cg_axpby

    n = 10000
    y = darray.random((n,), seed=25)
    x = darray.random((n,), seed=26)
    a = torch.tensor(3.0, device="cuda", dtype=torch.float64)
    b = torch.tensor(2.0, device="cuda", dtype=torch.float64)
    y0 = np.asarray(y).copy()
    x0 = np.asarray(x)
    cg_axpby(y, x, a, b, isalpha=True, negate=False)
    assert np.allclose(np.asarray(y), y0 + 1.5 * x0)
    cg_axpby(y, x, a, b, isalpha=True, negate=True)
    assert np.allclose(np.asarray(y), y0)
    cg_axpby(y, x, a, b, isalpha=False, negate=False)
    assert np.allclose(np.asarray(y), x0 + 1.5 * y0)


def test_cg_gpu():
    from sparse import csr_array, linalg

    n = 300
    s = spd_csr(n, seed=27)
    rng = np.random.default_rng(28)
    b = rng.random(n)
    x, info = linalg.cg(csr_array(s), b, tol=1e-10, conv_test_iters=10)
    assert info == 0
    assert np.allclose(s @ np.asarray(x), b, atol=1e-6)


def test_cg_poisson_gpu():
    from sparse import darray, gallery, linalg

    A = gallery.poisson2d(128)
    n = A.shape[0]
    b = darray.ones((n,), dtype=np.float64)
    x, info = linalg.cg(A, b, tol=1e-8, maxiter=2000, conv_test_iters=25)
    r = b - A.dot(x)
    assert float(r.norm().item()) < 1e-6 * float(b.norm().item())


def test_cdist_gpu():
    from sparse import spatial

    XA = sample_dense((100, 7), seed=29)
    XB = sample_dense((80, 7), seed=30)
    from scipy.spatial.distance import cdist as sp_cdist

    assert np.allclose(np.asarray(spatial.cdist(XA, XB)), sp_cdist(XA, XB),
                       atol=1e-8)


def test_tropical_spmv_gpu():
    from sparse import csr_array
    from sparse.darray import DistArray

    rng = np.random.default_rng(31)
    s = sample_csr(60, 60, 0.2, seed=32)
    x = rng.integers(0, 100, size=(60, 3)).astype(np.int64)
    A = csr_array(s)
    y = A.tropical_spmv(x)
    yn = np.asarray(y)
    sc = s.tocoo()
    expect = np.zeros((60, 3), dtype=np.int64)
    for r in range(60):
        cols = sc.col[sc.row == r]
        if len(cols):
            cand = sorted((tuple(x[c]) for c in cols), reverse=True)[0]
            expect[r] = cand
    assert np.array_equal(yn, expect)


def test_native_extension_is_loaded():
    """The driver checks loaded .so files; make sure ours is in-process."""
    from sparse import kernels

    assert kernels.ext() is not None
    import subprocess

    maps = open("/proc/self/maps").read()
    assert "sparse_hip.so" in maps


def test_spmv_dot_fused_gpu():
    from sparse import csr_array, darray

    s = sample_csr(5000, 5000, 0.002, seed=33)
    A = csr_array(s)
    p = darray.random((5000,), seed=34)
    q = darray.zeros((5000,))
    pq = A.spmv_dot(p, q)
    qref = s @ np.asarray(p)
    assert np.allclose(np.asarray(q), qref, rtol=1e-10)
    assert np.isclose(float(pq.item()), float(np.asarray(p) @ qref), rtol=1e-10)


@pytest.mark.parametrize("n", [50000, 3_000_001])
@pytest.mark.parametrize("ndt", [np.float64, np.float32])
def test_axpby_norm2_gpu(n, ndt):
    """n=3M+1 regression: a capped launch grid once left elements beyond
    512K untouched (silent corruption in the fused CG loop); odd n also
    exercises the scalar tail."""
    from sparse import darray
    from sparse.linalg import _axpby_norm2

    y = darray.random((n,), seed=35, dtype=ndt)
    x = darray.random((n,), seed=36, dtype=ndt)
    y0 = np.asarray(y).copy()
    x0 = np.asarray(x)
    tdt = torch.float64 if ndt == np.float64 else torch.float32
    a = torch.tensor(2.0, device="cuda", dtype=tdt)
    b = torch.tensor(4.0, device="cuda", dtype=tdt)
    rz = _axpby_norm2(y, x, a, b, negate=True)
    expect = (y0 - 0.5 * x0).astype(ndt)
    rt = 1e-12 if ndt == np.float64 else 1e-5
    assert np.allclose(np.asarray(y), expect, rtol=rt)
    assert np.isclose(float(rz.item()),
                      float(expect.astype(np.float64) @ expect), rtol=1e-3
                      if ndt == np.float32 else 1e-10)


def test_ell_spmv_three_piece_split():
    """Exercise the halo (3-piece x) addressing path of the ELL kernel with
    an artificial split — the multi-GPU layout with ws=1 data."""
    from sparse import darray, gallery, kernels

    A = gallery.banded(4000, ndiags=7)
    x = darray.random((4000,), seed=41)
    ell = A._ell()
    assert ell is not None
    plan = A._xplan(x.partition)
    xw = plan.gather(x.local)
    ref = torch.empty(4000, dtype=torch.float64, device="cuda")
    kernels.ell_spmv(ell, (xw[:0], xw, xw[:0]), ref, plan.lo)
    n = xw.numel()
    for cut1, cut2 in [(0, n), (100, n - 137), (1, 2), (n // 2, n // 2)]:
        out = torch.empty(4000, dtype=torch.float64, device="cuda")
        pieces = (xw[:cut1].clone(), xw[cut1:cut2].clone(), xw[cut2:].clone())
        kernels.ell_spmv(ell, pieces, out, plan.lo)
        assert torch.allclose(out, ref), (cut1, cut2)
    # fused dot variant
    q = torch.empty(4000, dtype=torch.float64, device="cuda")
    d = kernels.ell_spmv_dot(ell, (xw[:50].clone(), xw[50:n - 60].clone(),
                                   xw[n - 60:].clone()), q, x.local, plan.lo)
    assert torch.allclose(q, ref)
    assert np.isclose(float(d.item()), float(torch.dot(x.local, ref).item()))


@pytest.mark.parametrize("dt", [np.float32, np.complex128])
def test_ell_spmv_dtypes_gpu(dt):
    """ELL fast path across dtypes (banded => ELL-eligible)."""
    from sparse import csr_array, gallery

    A = gallery.banded(3000, ndiags=9, dtype=np.float64)
    if np.dtype(dt) != np.float64:
        A = A.astype(dt)
    x = sample_dense(3000, seed=50, dtype=dt)
    assert A._ell() is not None
    y = A @ x
    sref = A.to_scipy_sparse_csr()
    assert np.allclose(np.asarray(y), sref @ x, rtol=1e-4 if dt == np.float32 else 1e-10)


def test_solve_ivp_gpu():
    """solve_ivp on GPU DistArrays (exercises the rk_calc_dy kernel)."""
    from sparse import asdistarray, integrate

    y0 = np.linspace(1.0, 2.0, 5000)

    def f(t, y):
        return y * (-0.3)

    res = integrate.solve_ivp(f, (0, 2.0), y0, method="RK45", rtol=1e-8,
                              atol=1e-10)
    assert res.success
    assert np.allclose(res.y[:, -1], y0 * np.exp(-0.6), rtol=1e-6)


def test_profiling_ranges_gpu():
    from sparse import csr_array, profiling

    s = sample_csr(200, 200, 0.05, seed=51)
    A = csr_array(s)
    x = sample_dense(200, seed=52)
    with profiling.profile() as prof:
        from sparse import linalg

        linalg.cg(A.T @ A + csr_array(5 * np.eye(200)), x, tol=1e-6, maxiter=50)
    keys = [e.key for e in prof.key_averages()]
    assert any("sparse::" in k for k in keys), keys[:10]


def test_jacobi_smooth_gpu():
    from sparse import darray, gallery

    A = gallery.poisson2d(64)
    n = A.shape[0]
    x = darray.random((n,), seed=60)
    b = darray.random((n,), seed=61)
    d = A.diagonal()
    dinv = darray.DistArray.from_local(1.0 / d.local, d.partition, d.shape)
    out = A.jacobi_smooth(x, b, dinv, 0.7)
    r = b - A.dot(x)
    expect = np.asarray(x) + 0.7 * np.asarray(dinv) * np.asarray(r)
    assert np.allclose(np.asarray(out), expect, rtol=1e-12)


def test_cg_complex_gpu():
    """Hermitian positive-definite complex CG (eager GPU path: complex axpby
    kernels + vdot)."""
    from sparse import csr_array, linalg

    n = 120
    s = sample_csr(n, n, 0.2, seed=70, dtype=np.complex128)
    H = (s + s.conj().T + 2 * n * sps.eye(n)).tocsr()
    rng = np.random.default_rng(71)
    b = rng.random(n) + 1j * rng.random(n)
    x, info = linalg.cg(csr_array(H), b, tol=1e-10, maxiter=500, conv_test_iters=5)
    assert info == 0
    assert np.allclose(H @ np.asarray(x), b, atol=1e-6)


def test_dia_fast_path_gpu():
    """Banded matrices take the device-DIA path (no index stream): the
    mirror must build, and SpMV / fused-dot / Jacobi must match the CSR
    reference numerics."""
    from sparse import csr_array, darray, gallery, kernels

    n = 5000
    A = gallery.banded(n, ndiags=9)
    dm = A._dia()
    assert dm is not None, "banded matrix should be DIA-eligible"
    x = darray.random((n,), seed=61)
    sref = A.to_scipy_sparse_csr()
    # plain SpMV through the public path (dispatches to DIA)
    y = A @ x
    assert np.allclose(np.asarray(y), sref @ np.asarray(x), rtol=1e-12)
    # fused dot
    q = darray.zeros((n,), dtype=np.float64)
    d = A.spmv_dot(x, q)
    assert np.allclose(np.asarray(q), sref @ np.asarray(x), rtol=1e-12)
    assert np.isclose(float(d), float(np.asarray(x) @ (sref @ np.asarray(x))),
                      rtol=1e-10)
    # weighted Jacobi: out = x + w*dinv*(b - A x)
    b = darray.random((n,), seed=62)
    dinv = darray.DistArray.from_local(
        torch.as_tensor(1.0 / sref.diagonal(), device="cuda"),
        x.partition, x.gshape)
    out = A.jacobi_smooth(x, b, dinv, 0.7)
    expect = np.asarray(x) + 0.7 * (1.0 / sref.diagonal()) * (
        np.asarray(b) - sref @ np.asarray(x))
    assert np.allclose(np.asarray(out), expect, rtol=1e-12)


def test_dia_three_piece_split():
    """Halo (3-piece x) addressing of the DIA kernel with artificial
    splits, as in the ELL test above."""
    from sparse import darray, gallery, kernels

    n = 4000
    A = gallery.banded(n, ndiags=7)
    dm = A._dia()
    assert dm is not None
    x = darray.random((n,), seed=63)
    plan = A._xplan(x.partition)
    xw = plan.gather(x.local)
    wsize = plan.hi - plan.lo
    ref = torch.empty(n, dtype=torch.float64, device="cuda")
    kernels.dia_spmv(dm, (xw[:0], xw, xw[:0]), ref, plan.lo, wsize)
    m = xw.numel()
    for cut1, cut2 in [(0, m), (100, m - 137), (1, 2), (m // 2, m // 2)]:
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        pieces = (xw[:cut1].clone(), xw[cut1:cut2].clone(), xw[cut2:].clone())
        kernels.dia_spmv(dm, pieces, out, plan.lo, wsize)
        assert torch.allclose(out, ref), (cut1, cut2)
    d = kernels.dia_spmv_dot(
        dm, (xw[:50].clone(), xw[50:m - 60].clone(), xw[m - 60:].clone()),
        torch.empty(n, dtype=torch.float64, device="cuda"), x.local,
        plan.lo, wsize)
    assert np.isclose(float(d.item()), float(torch.dot(x.local, ref).item()))


def test_dia_rejects_scattered():
    """Scattered-column matrices must NOT build a DIA mirror (too many
    distinct diagonals) and fall back to ELL/CSR."""
    from utils.sample import sample_csr
    from sparse import csr_array

    s = sample_csr(2000, 2000, density=0.003, seed=64)
    A = csr_array(s)
    assert A._dia() is None
    x = sample_dense(2000, seed=65)
    assert np.allclose(np.asarray(A @ x), s @ x, rtol=1e-12)


def test_cg_xr_norm2_gpu():
    """K2 numerics: x += (a/b)p, r -= (a/b)q, returns sum(r_new^2).
    Odd n exercises the scalar tail; n>512K guards the grid-cap regression."""
    from sparse import darray, kernels

    kernels.require()
    for n in (70001, 1_500_000):
        x = darray.random((n,), seed=70)
        p = darray.random((n,), seed=71)
        r = darray.random((n,), seed=72)
        q = darray.random((n,), seed=73)
        x0, p0 = np.asarray(x).copy(), np.asarray(p)
        r0, q0 = np.asarray(r).copy(), np.asarray(q)
        a = torch.tensor(3.0, device="cuda", dtype=torch.float64)
        b = torch.tensor(2.0, device="cuda", dtype=torch.float64)
        rz = kernels.cg_xr_norm2(x.local, p.local, r.local, q.local, a, b)
        xe, re = x0 + 1.5 * p0, r0 - 1.5 * q0
        assert np.allclose(np.asarray(x), xe, rtol=1e-12)
        assert np.allclose(np.asarray(r), re, rtol=1e-12)
        assert np.isclose(float(rz.item()), float(re @ re), rtol=1e-10)


def test_spmv_bpdot_gpu():
    """K1 numerics: p_new = r + beta*p, q = A@p_new, returns p_new.q —
    against a plain torch/scipy fp64 reference."""
    from sparse import darray, gallery

    n = 4000
    A = gallery.banded(n, ndiags=9)
    assert A._dia() is not None
    sref = A.to_scipy_sparse_csr()
    r = darray.random((n,), seed=80)
    p_old = darray.random((n,), seed=81)
    p_new = darray.zeros((n,))
    q = darray.zeros((n,))
    bn = torch.tensor(0.7, device="cuda", dtype=torch.float64)
    bd = torch.tensor(2.0, device="cuda", dtype=torch.float64)
    pq = A.spmv_bpdot(r, p_old, p_new, q, bn, bd)
    pe = np.asarray(r) + 0.35 * np.asarray(p_old)
    qe = sref @ pe
    assert np.allclose(np.asarray(p_new), pe, rtol=1e-12)
    assert np.allclose(np.asarray(q), qe, rtol=1e-12)
    assert np.isclose(float(pq.item()), float(pe @ qe), rtol=1e-10)


def test_cg_two_kernel_matches_eager_gpu():
    """The 2-kernel DIA CG loop must converge to the same solution as the
    generic path (CSR fallback) on the same banded SPD system."""
    from sparse import csr_array, gallery, linalg

    A = gallery.poisson2d(96)
    n = A.shape[0]
    rng = np.random.default_rng(82)
    b = rng.random(n)
    assert A._dia() is not None
    x2, info2 = linalg.cg(A, b, tol=1e-10, maxiter=3000, conv_test_iters=20)
    A2 = gallery.poisson2d(96)
    A2._dia_cache = "no"
    A2._ell_cache = "no"
    x4, info4 = linalg.cg(A2, b, tol=1e-10, maxiter=3000, conv_test_iters=20)
    assert info2 == 0 and info4 == 0
    s = A.to_scipy_sparse_csr()
    assert np.allclose(s @ np.asarray(x2), b, atol=1e-7)
    assert np.allclose(np.asarray(x2), np.asarray(x4), atol=1e-6)


def test_spgemm_2d_local_gpu():
    """2-D grid SpGEMM's local pipeline (CSC block -> CSR conversion,
    binned SpGEMM, COO shuffle/rebuild) on cuda tensors at ws=1."""
    from sparse import csc_array, csr_array

    a = sample_csr(120, 90, 0.1, seed=90)
    b = sample_csr(90, 70, 0.1, seed=91).tocsc()
    A = csr_array(a)
    B = csc_array(b)
    C = A._spgemm_2d(B)
    ref = (a @ b).tocsr()
    assert np.allclose(np.asarray(C.todense()), ref.toarray(), rtol=1e-10)


def test_precise_plan_gpu():
    """PreciseGatherPlan remap/gather on cuda tensors (ws=1 direct use)."""
    from sparse import csr_array
    from sparse.parallel.gather import PreciseGatherPlan
    from sparse.parallel.partition import RowPartition

    s = sample_csr(50, 300, 0.03, seed=92)
    A = csr_array(s)
    plan = PreciseGatherPlan(A._indices, RowPartition.single(300))
    x = torch.rand(300, dtype=torch.float64, device="cuda")
    xw = plan.gather(x)
    assert xw.numel() == plan.hi
    remapped = plan.remap(A._indices)
    assert int(remapped.max()) < plan.hi
    # y via compact window == direct SpMV
    got = torch.zeros(50, dtype=torch.float64, device="cuda")
    for r in range(50):
        sl = slice(int(A._indptr[r]), int(A._indptr[r + 1]))
        got[r] = (A._values[sl] * xw[remapped[sl].long()]).sum()
    ref = s @ x.cpu().numpy()
    assert np.allclose(got.cpu().numpy(), ref, rtol=1e-10)


def test_dia_residual_gpu():
    """Fused r = b - A@x on the DIA path vs the eager reference."""
    from sparse import darray, gallery

    n = 5000
    A = gallery.banded(n, ndiags=9)
    assert A._dia() is not None
    x = darray.random((n,), seed=95)
    b = darray.random((n,), seed=96)
    r = A.residual(x, b)
    sref = A.to_scipy_sparse_csr()
    expect = np.asarray(b) - sref @ np.asarray(x)
    assert np.allclose(np.asarray(r), expect, rtol=1e-12)
    # scattered matrix takes the fallback path
    s = sample_csr(800, 800, 0.01, seed=97)
    from sparse import csr_array

    A2 = csr_array(s)
    assert A2._dia() is None
    x2 = darray.random((800,), seed=98)
    b2 = darray.random((800,), seed=99)
    r2 = A2.residual(x2, b2)
    assert np.allclose(np.asarray(r2), np.asarray(b2) - s @ np.asarray(x2),
                       rtol=1e-10)


def test_solvers_gpu():
    """Non-CG solvers end-to-end on the GPU (gmres/bicgstab/lsqr/eigsh run
    through DistArray torch ops + HIP SpMV)."""
    from sparse import csr_array, linalg

    n = 60
    rng = np.random.default_rng(101)
    s = (sps.random(n, n, 0.25, random_state=102) + n * sps.eye(n)).tocsr()
    b = rng.random(n)
    x, _ = linalg.gmres(csr_array(s), b, tol=1e-10, restart=20, maxiter=300)
    assert np.allclose(s @ np.asarray(x), b, atol=1e-5)
    x, _ = linalg.bicgstab(csr_array(s), b, tol=1e-10, maxiter=400,
                           conv_test_iters=2)
    assert np.allclose(s @ np.asarray(x), b, atol=1e-5)
    spd = spd_csr(n, seed=103)
    w, V = linalg.eigsh(csr_array(spd), k=3, which="LA")
    ws_ = np.linalg.eigvalsh(spd.toarray())
    assert np.allclose(np.sort(w), ws_[-3:], atol=1e-4)
    m = 50
    srect = sps.random(m, 20, 0.4, random_state=104).tocsr()
    brect = rng.random(m)
    r = linalg.lsqr(csr_array(srect), brect, atol=1e-12, btol=1e-12,
                    iter_lim=200)
    xref = sps.linalg.lsqr(srect, brect, atol=1e-12, btol=1e-12,
                           iter_lim=200)[0]
    assert np.allclose(np.asarray(r[0]), xref, atol=1e-5)


def test_integrate_banded_gpu():
    """solve_ivp with a sparse banded RHS operator on GPU (SpMV inside the
    RK stages)."""
    from sparse import asdistarray, gallery, integrate

    n = 2000
    A = gallery.banded(n, ndiags=5)
    A = A * (-0.01)
    y0 = np.linspace(1.0, 2.0, n)

    def f(t, y):
        return A.dot(asdistarray(y))

    res = integrate.solve_ivp(f, (0, 1.0), y0, method="RK45", rtol=1e-8,
                              atol=1e-10)
    assert res.success


def test_spgemm_checked_bin_gpu(monkeypatch):
    """Rows with product upper bound > 1024 but few distinct columns take
    the checked 4096-entry bin; true overflows (uniques > 2048) reroute
    to the (row-batched) ESC fallback."""
    from sparse import csr_array, kernels

    rng = np.random.default_rng(47)
    # checked-bin case: ~30K products/row, <= 1500 uniques
    a = sps.random(40, 2000, 0.5, random_state=48).tocsr()
    b = sps.random(2000, 1500, 0.01, random_state=49).tocsr()
    C = csr_array(a) @ csr_array(b)
    ref = (a @ b).tocsr()
    assert C.nnz == ref.nnz
    assert np.allclose(np.asarray(C.todense()), ref.toarray(), rtol=1e-10)
    # overflow case: uniques ~ 5000 > 2048 -> ESC, with tiny forced batches
    monkeypatch.setattr(kernels, "_ESC_LIMIT", 4000)
    b2 = sps.random(2000, 5000, 0.02, random_state=50).tocsr()
    C2 = csr_array(a) @ csr_array(b2)
    ref2 = (a @ b2).tocsr()
    assert C2.nnz == ref2.nnz
    assert np.allclose(np.asarray(C2.todense()), ref2.toarray(), rtol=1e-10)
    # complex stays on ESC (checked bin is 8-byte values only)
    ac = csr_array(a.astype(np.complex128))
    bc = csr_array(b.astype(np.complex128))
    Cc = ac @ bc
    refc = (a.astype(np.complex128) @ b.astype(np.complex128)).tocsr()
    assert np.allclose(np.asarray(Cc.todense()), refc.toarray(), rtol=1e-10)


# -- row-pair DIA/ELL family: pinned behaviour -------------------------------
# Sizes: a one-row tail thread in a second block (513, 1025), an exact block
# multiple (512) and odd m with mp = m + 1 (511, 513, 1025).
_PIN_SIZES = [511, 512, 513, 1025]
_PIN_DIA_OPS = ["dia_spmv", "dia_spmv_dot", "dia_residual", "dia_jacobi",
                "dia_spmv_bpdot"]
_PIN_ELL_OPS = ["ell_spmv", "ell_spmv_dot", "ell_jacobi"]
_PIN_RANGED_OPS = ["dia_spmv", "dia_spmv_dot", "dia_residual", "dia_jacobi",
                   "ell_spmv", "ell_spmv_dot"]
_PIN_OMEGA = 0.7
_PIN_CACHE = {}


class _Pin:
    """One pinned problem: a scipy matrix with distinct values on every
    diagonal (DIA) or a row-uniform scattered matrix (ELL), its mirror,
    seeded vectors and the scipy references of all eight ops."""

    def __init__(self, kind, m, dt):
        from sparse import csr_array

        rng = np.random.default_rng(7000 + m)
        if kind == "dia":
            offs = (-37, -2, 0, 1, 40)
            s = sps.diags([0.5 + rng.random(m - abs(o)) for o in offs], offs,
                          shape=(m, m), format="csr")
        else:
            W = 8
            rows = np.repeat(np.arange(m), W)
            near = (rows + rng.integers(-40, 41, m * W)) % m
            far = rng.integers(0, m, m * W)
            cols = np.where(rng.random(m * W) < 0.08, far, near)
            s = sps.csr_matrix((0.5 + rng.random(m * W), (rows, cols)),
                               shape=(m, m))
            s.sum_duplicates()
        self.s = s = s.astype(dt)
        self.m, self.dt = m, np.dtype(dt)
        self.A = A = csr_array(s)
        if kind == "dia":
            self.mir = A._dia()
            assert self.mir is not None
        else:
            assert A._dia() is None
            self.mir = A._ell()
            assert self.mir is not None
        self.lo, self.hi = A._col_window()
        self.w = self.hi - self.lo

        def vec():
            v = rng.random(m)
            if self.dt.kind == "c":
                v = v + 1j * rng.random(m)
            return v.astype(dt)

        self.np = {k: vec() for k in ("x", "p", "b", "dinv", "r", "pold")}
        # rows sum at most 8 entries * 1.5 * |x| < 16: with b >= 16 the
        # residual and the Jacobi update add same-signed terms only, so
        # the relative tolerances below are not eaten by cancellation
        self.np["b"] = (self.np["b"] + 16).astype(dt)
        self.t = {k: torch.as_tensor(v, device="cuda")
                  for k, v in self.np.items()}
        tdt = self.t["x"].dtype
        self.bn = torch.tensor(0.7, device="cuda", dtype=tdt)
        self.bd = torch.tensor(2.0, device="cuda", dtype=tdt)
        # references in fp64 / complex128 from the rounded inputs
        wide = np.complex128 if self.dt.kind == "c" else np.float64
        n = {k: v.astype(wide) for k, v in self.np.items()}
        s = s.astype(wide)
        Ax = s @ n["x"]
        pn = n["r"] + 0.35 * n["pold"]
        jac = n["x"] + _PIN_OMEGA * n["dinv"] * (n["b"] - Ax)
        self.ref = {
            "spmv": ([Ax], None),
            "spmv_dot": ([Ax], n["p"] @ Ax),
            "residual": ([n["b"] - Ax], None),
            "jacobi": ([jac], None),
            "spmv_bpdot": ([pn, s @ pn], pn @ (s @ pn)),
        }

    def pieces(self, name, cut):
        xw = self.t[name][self.lo:self.hi]
        if cut is None:
            return xw[:0], xw, xw[:0]
        c1, c2 = cut
        return xw[:c1].clone(), xw[c1:c2].clone(), xw[c2:].clone()

    def new_out(self, op):
        # NaN-filled: a row no thread wrote fails every comparison
        k = 2 if op == "dia_spmv_bpdot" else 1
        return [torch.full((self.m,), float("nan"), dtype=self.t["x"].dtype,
                           device="cuda") for _ in range(k)]

    def run(self, op, cut=None, rows=(0, -1), out=None):
        """Run one kernel wrapper; returns (output vectors, dot or None)."""
        from sparse import kernels as K

        out = self.new_out(op) if out is None else out
        t, mir, lo, w = self.t, self.mir, self.lo, self.w
        px = self.pieces("x", cut)
        dot = None
        if op == "dia_spmv":
            K.dia_spmv(mir, px, out[0], lo, w, *rows)
        elif op == "dia_spmv_dot":
            dot = K.dia_spmv_dot(mir, px, out[0], t["p"], lo, w, *rows)
        elif op == "dia_residual":
            K.dia_residual(mir, px, t["b"], out[0], lo, w, *rows)
        elif op == "dia_jacobi":
            K.dia_jacobi(mir, px, t["x"], t["b"], t["dinv"], _PIN_OMEGA,
                         out[0], lo, w, *rows)
        elif op == "dia_spmv_bpdot":
            assert rows == (0, -1)
            dot = K.dia_spmv_bpdot(mir, self.pieces("r", cut),
                                   self.pieces("pold", cut), out[0], out[1],
                                   self.bn, self.bd, lo, w)
        elif op == "ell_spmv":
            K.ell_spmv(mir, px, out[0], lo, *rows)
        elif op == "ell_spmv_dot":
            dot = K.ell_spmv_dot(mir, px, out[0], t["p"], lo, *rows)
        elif op == "ell_jacobi":
            assert rows == (0, -1)
            K.ell_jacobi(mir, px, t["x"], t["b"], t["dinv"], _PIN_OMEGA,
                         out[0], lo)
        else:
            raise AssertionError(op)
        return out, dot


def _pin(op, m, dt=np.float64):
    key = (op[:3], m, np.dtype(dt))
    if key not in _PIN_CACHE:
        _PIN_CACHE[key] = _Pin(*key)
    return _PIN_CACHE[key]


def _pin_cuts(w):
    return [(0, w), (1, 2), (101, w - 137), (w // 2, w // 2)]


def _pin_check_reference_and_cuts(op, m, dt):
    P = _pin(op, m, dt)
    rvecs, rdot = P.ref[op[4:]]
    vrt = 1e-4 if P.dt == np.float32 else (1e-10 if P.dt.kind == "c"
                                           else 1e-12)
    single, sdot = P.run(op)
    for got, want in zip(single, rvecs):
        assert np.allclose(got.cpu().numpy(), want, rtol=vrt), (op, m)
    if rdot is not None:
        assert sdot.dim() == 0
        assert np.isclose(float(sdot.item()), float(rdot), rtol=1e-10)
    for cut in _pin_cuts(P.w):
        three, tdot = P.run(op, cut=cut)
        for got, want in zip(three, single):
            assert torch.equal(got, want), (op, m, cut)
        if rdot is not None:
            assert np.isclose(float(tdot.item()), float(rdot), rtol=1e-10)


@pytest.mark.parametrize("m", _PIN_SIZES)
@pytest.mark.parametrize("op", _PIN_DIA_OPS + _PIN_ELL_OPS)
def test_rowpair_reference_and_window_cuts_gpu(op, m):
    """Every DIA/ELL row-pair op against scipy, and three-piece x windows
    (odd cuts hit the odd-parity and clamped pair loads) bit-equal to the
    single-piece result: the arithmetic per row is identical."""
    _pin_check_reference_and_cuts(op, m, np.float64)


@pytest.mark.parametrize("m", _PIN_SIZES)
@pytest.mark.parametrize("dt", [np.float32, np.complex128])
@pytest.mark.parametrize("op", ["dia_spmv", "dia_jacobi"])
def test_rowpair_dia_dtypes_gpu(op, dt, m):
    """DIA SpMV and Jacobi in fp32 / complex128 (tolerances as in
    test_ell_spmv_dtypes_gpu)."""
    _pin_check_reference_and_cuts(op, m, dt)


@pytest.mark.parametrize("m", _PIN_SIZES)
@pytest.mark.parametrize("op", _PIN_RANGED_OPS)
def test_rowpair_row_ranges_gpu(op, m):
    """[a, b), [0, a), [b, -1) with even a < b into one output reproduce
    the full-range call bit for bit; the split dots sum to the full dot.
    (0, 512) makes the outer ranges empty at m <= 512 and gives a span
    whose half is an exact block multiple."""
    P = _pin(op, m)
    full, fdot = P.run(op)
    for a, b in [(2, 258), (0, 512)]:
        out = P.new_out(op)
        dots = [P.run(op, rows=rows, out=out)[1]
                for rows in [(a, b), (0, a), (b, -1)]]
        assert torch.equal(out[0], full[0]), (op, m, a, b)
        if fdot is not None:
            assert all(d.dim() == 0 for d in dots)
            assert torch.allclose(dots[0] + dots[1] + dots[2], fdot,
                                  rtol=1e-12, atol=0), (op, m, a, b)
