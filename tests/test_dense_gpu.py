"""Edge checks of the kernels that multiply a sparse matrix by a dense operand
(spmv.hip's nnz-split SpMV and fused dot, spmm.hip's two CSR SpMM kernels,
the MFMA BSR SpMM and rSpMM, conv.hip's CSC column-split SpMV / SpMM)
against the plain long-double references of utils/dense_cases.py — all @gpu.

The inputs sit against the kernels' constants (2048 nnz and 256 threads per
SpMV block, the lane tiles of the SpMM kernels, the 16 x 16 blocks); every
tolerance is the derived (n + 2) eps S of dense_cases, never a measured one.
Every output buffer the caller can pass is pre-filled with NaN, and rows
without entries must come out exactly zero.  The ops layer is called with
hand-built LocalCSRs so the tests choose index dtype and offsets.  No case
is skipped or filtered; a route assertion that does not hold is a failure.
"""
import numpy as np
import pytest
import torch

from utils.common import types
from utils import dense_cases as dc

pytestmark = pytest.mark.gpu

_IDX = [torch.int32, torch.int64]
_REAL = [np.float32, np.float64]
_CACHE = {}


@pytest.fixture(autouse=True, scope="module")
def _require_ext():
    if torch.cuda.is_available():
        from sparse.kernels import require

        require()


def _cached(key, make):
    """References are computed once per module and never modified."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _tdt(dt):
    return torch.from_numpy(np.zeros(0, dtype=dt)).dtype


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _local(M, idt):
    from sparse.ops.local import LocalCSR

    return LocalCSR(_dev(M.indptr), _dev(M.indices).to(idt), _dev(M.values),
                    M.nrows, M.ncols)


def _nan(shape, dt):
    return torch.full(shape, float("nan"), dtype=_tdt(dt), device="cuda")


class _Worst:
    """Largest |got - ref| / tolerance seen by one test."""

    def __init__(self):
        self.ratio, self.where = 0.0, ""

    def check(self, got, values, tol, what):
        assert got.is_cuda and tuple(got.shape) == values.shape, what
        err = np.abs(got.detach().cpu().numpy().astype(values.dtype) - values)
        assert np.all(err <= tol), \
            f"{what}: {int(np.sum(~(err <= tol)))} of {err.size} off, " \
            f"worst at flat index {int(np.argmax(err - tol))}"
        pos = tol > 0
        if np.any(pos):
            r = float(np.max(err[pos] / tol[pos]))
            if r > self.ratio:
                self.ratio, self.where = r, what
        return err

    def report(self):
        print(f"max |got - ref| / tolerance: {self.ratio:.3f} ({self.where})")


# -- SpMV -------------------------------------------------------------------------
# columns from 2^33 on do not exist in int32: "wide" runs with int64 only
_SPMV_RUNS = [("base", torch.int32), ("base", torch.int64),
              ("col_lo", torch.int32), ("col_lo", torch.int64),
              ("wide", torch.int64)]
_SPMV_IDS = [f"{v}-i{torch.iinfo(i).bits}" for v, i in _SPMV_RUNS]
BETA = -0.5


@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("variant,idt", _SPMV_RUNS, ids=_SPMV_IDS)
def test_spmv_boundary_set(variant, idt, dt):
    """nnz 1 .. 26625 over 1 .. 14 blocks: rows ending / starting exactly on
    a block boundary, crossing one, spanning three blocks (two carries),
    empty rows on a boundary, trailing empty rows behind a full last block,
    more than 256 owned rows per block; beta = 0 into a NaN-filled y and
    beta = -0.5 onto y0."""
    from sparse.ops import local as ops

    w = _Worst()
    for nnz in dc.SPMV_NNZS:
        M, lo = dc.spmv_boundary_csr(dt, nnz, variant)
        x, y0, _ = dc.spmv_vectors(dt, nnz, M.nrows)
        ref = _cached(("spmv", dt, nnz, variant),
                      lambda: dc.ref_spmv(M, x, lo))
        A, xd = _local(M, idt), _dev(x)
        y = _nan((M.nrows,), dt)
        out = ops.spmv(A, xd, lo, y, 0.0)
        assert out.data_ptr() == y.data_ptr() and y.dtype == _tdt(dt)
        w.check(y, ref.values, dc.dense_tol(ref, dt),
                f"nnz {nnz} beta 0")
        assert torch.all(y[_dev(ref.n == 0)] == 0)   # exactly, not NaN
        y = _dev(y0)
        ops.spmv(A, xd, lo, y, BETA)
        by = BETA * y0.astype(ref.values.dtype)
        w.check(y, ref.values + by, dc.dense_tol(ref, dt, extra=np.abs(by)),
                f"nnz {nnz} beta {BETA}")
    w.report()


@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", types)
def test_spmv_without_entries(dt, idt):
    """nnz = 0: the memset (beta = 0) and scale_kernel over two blocks."""
    from sparse.ops import local as ops
    from utils.spout_cases import empty_csr

    M = empty_csr(300, 40, dt)
    x, y0, _ = dc.spmv_vectors(dt, 0, M.nrows)
    A, xd = _local(M, idt), _dev(x[:40])
    y = _nan((M.nrows,), dt)
    ops.spmv(A, xd, 0, y, 0.0)
    assert torch.all(y == 0)
    y = _dev(y0)
    ops.spmv(A, xd, 0, y, BETA)
    # a scaling by -0.5 is exact
    assert np.array_equal(y.cpu().numpy(), (BETA * y0).astype(dt))


@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", _REAL)
@pytest.mark.parametrize("nnz", dc.SPMV_DOT_NNZS)
def test_spmv_fused_dot(nnz, dt, idt):
    """q = A x and dot_out += p . q with dot_out starting at 3: all operands
    positive, so a dropped carry or block partial shifts the dot by at least
    100x the tolerance (test_dense_cases.py)."""
    from sparse import kernels

    w = _Worst()
    for variant in ("base", "col_lo"):
        M, lo = dc.spmv_boundary_csr(dt, nnz, variant, positive=True)
        x, _, p = dc.spmv_vectors(dt, nnz, M.nrows, positive=True)
        ref = _cached(("dot", dt, nnz, variant),
                      lambda: dc.ref_spmv(M, x, lo))
        q = _nan((M.nrows,), dt)
        dot = torch.full((), 3.0, dtype=_tdt(dt), device="cuda")
        kernels.spmv_dot(_local(M, idt), _dev(x), q, _dev(p), dot, lo)
        w.check(q, ref.values, dc.dense_tol(ref, dt), f"q, {variant}")
        assert torch.all(q[_dev(ref.n == 0)] == 0)
        want = np.longdouble(3.0) + np.sum(p.astype(np.longdouble) * ref.values)
        tol = dc.dot_tol(ref, p, 3.0, -(-nnz // dc.SPMV_NNZ_PER_BLOCK), dt)
        w.check(dot, np.asarray(want), np.asarray(tol), f"dot, {variant}")
    w.report()


# -- SpMM -------------------------------------------------------------------------
@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("m", dc.SPMM_MS)
def test_spmm_lane_tiles(m, dt, idt):
    """k = 1 .. 32 through the lane-tiled kernel (64 .. 2 rows per wave) and
    k = 33 .. 129 through the 64-lanes-per-row kernel (second column tile at
    k > 64), m around the rows per block, col_lo 0 and 1000, into a
    NaN-filled C."""
    from sparse.ops import local as ops

    w = _Worst()
    for lo in (0, dc.COL_LO):
        M = dc.spmm_csr(dt, m, lo)
        A = _local(M, idt)
        empty = _dev(np.diff(M.indptr) == 0)
        for k in dc.SPMM_SMALL_KS + dc.SPMM_WIDE_KS:
            B = dc.rand_dense(100 + k, (dc.SPMM_WINDOW, k), dt)
            ref = _cached(("spmm", dt, m, lo, k),
                          lambda: dc.ref_spmm(M, B, lo))
            C = _nan((m, k), dt)
            out = ops.spmm(A, _dev(B), lo, C)
            assert out.data_ptr() == C.data_ptr()
            w.check(C, ref.values, dc.dense_tol(ref, dt),
                    f"col_lo {lo} k {k}")
            assert torch.all(C[empty] == 0)
    w.report()


def test_spmm_wide_kernel_many_rows():
    """m = 262145 at k = 33: the rows ride grid.y and (m + 3) / 4 = 65537
    exceeds the 65535 HIP guarantees.  The launch is checked: a rejected one
    raises instead of leaving C as it was."""
    from sparse.ops import local as ops

    M, B = dc.spmm_large()
    C = _nan((M.nrows, 33), np.float64)
    out = ops.spmm(_local(M, torch.int32), _dev(B), 0, C)
    torch.cuda.synchronize()
    assert out.data_ptr() == C.data_ptr()
    got = C.cpu().numpy()
    assert not np.isnan(got).any()
    eps = np.longdouble(dc.real_eps(np.float64))
    worst = 0.0
    for s in range(0, M.nrows, 1 << 15):     # long double, a slab at a time
        e = min(s + (1 << 15), M.nrows)
        ref = (M.values[s:e].astype(np.longdouble)[:, None]
               * B[M.indices[s:e]].astype(np.longdouble))
        err, tol = np.abs(got[s:e] - ref), 3 * eps * np.abs(ref)   # n = 1
        assert np.all(err <= tol), f"rows {s}..{e}"
        worst = max(worst, float(np.max(err / tol)))
    print(f"max |got - ref| / tolerance: {worst:.3f}")


# -- BSR (MFMA) -------------------------------------------------------------------
@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", _REAL)
@pytest.mark.parametrize("m", dc.BSR_MS)
def test_bsr_mfma_kernel(m, dt, idt):
    """build_bsr + bsr_spmm on a window that starts block-aligned at column
    16 (first stored column 21) and ends ragged at 53: rows past m, window
    rows past n, an empty block row, ragged k tiles, asymmetric blocks (the
    fp32 and fp64 D-row maps differ)."""
    from sparse import kernels
    from sparse.ops import local as ops

    w = _Worst()
    M = dc.bsr_case(dt, m)
    lo16, hi16 = dc.bsr_window(M)
    A = _local(M, idt)
    bm = kernels.build_bsr(A, min_fill=0.0)
    assert bm is not None and bm.nbrows == -(-m // dc.BSR) and bm.m == m
    blocks = dc.bsr_blocks(M)
    assert bm.bcol.numel() == len(blocks)
    assert abs(bm.fill - M.nnz / (256.0 * len(blocks))) < 1e-12
    skip = dc.bsr_empty_block_row(m)
    if skip is not None:
        bp = bm.bptr.cpu().numpy()
        assert bp[skip] == bp[skip + 1]
    empty = _dev(np.diff(M.indptr) == 0)
    for k in dc.BSR_KS:
        Bw = dc.rand_dense(200 + k, (hi16 - lo16, k), dt)
        ref = _cached(("bsr", dt, m, k), lambda: dc.ref_spmm(M, Bw, lo16))
        tol = dc.dense_tol(ref, dt)
        # the window is the head of a buffer whose further rows, up to the
        # end of the last 16-row block, hold NaN: a read past the window
        # (rows 37 .. 47, which only the row < nwin guard keeps out) would
        # turn 0 * NaN into the result, inside the allocation
        buf = _nan((-(-M.ncols // dc.BSR) * dc.BSR - lo16, k), dt)   # 48
        buf[: hi16 - lo16] = _dev(Bw)
        Bd = buf[: hi16 - lo16]
        assert Bd.is_contiguous() and Bd.data_ptr() == buf.data_ptr()
        C = _nan((m, k), dt)
        kernels.bsr_spmm(bm, Bd, C, lo16)
        w.check(C, ref.values, tol, f"bsr k {k}")
        assert torch.all(C[empty] == 0)
        C2 = ops.spmm(A, Bd, lo16, _nan((m, k), dt))
        w.check(C2, ref.values, tol, f"spmm k {k}")
        assert np.all(np.abs((C - C2).cpu().numpy()) <= 2 * tol)
    w.report()


@pytest.mark.parametrize("dt", _REAL)
@pytest.mark.parametrize("m", dc.BSR_MS)
def test_bsr_route_through_csr_array(m, dt, monkeypatch):
    """csr_array @ B and dot(out=) take the MFMA route at every k >= 16 and
    hand it the block-aligned window from column 16 on.  m = 1 cannot fill a
    block to 5 % (one row is 16 of 256 positions): there the route must NOT
    be taken."""
    import scipy.sparse as sps

    from sparse import csr_array, kernels
    from sparse.darray import asdistarray

    M = dc.bsr_case(dt, m)
    lo16, hi16 = dc.bsr_window(M)
    A = csr_array(sps.csr_matrix((M.values, M.indices, M.indptr),
                                 shape=(m, M.ncols)))
    assert A._values.is_cuda and A._values.dtype == _tdt(dt)
    calls = []
    inner = kernels.bsr_spmm

    def rec(bm, Bw, C, col_lo):
        calls.append((int(col_lo), tuple(Bw.shape), tuple(C.shape)))
        return inner(bm, Bw, C, col_lo)

    monkeypatch.setattr(kernels, "bsr_spmm", rec)
    w = _Worst()
    empty = _dev(np.diff(M.indptr) == 0)
    for k in dc.BSR_KS:
        Bw = dc.rand_dense(200 + k, (hi16 - lo16, k), dt)
        ref = _cached(("bsr", dt, m, k), lambda: dc.ref_spmm(M, Bw, lo16))
        B = np.zeros((M.ncols, k), dtype=dt)
        B[:lo16] = np.nan       # rows the window must not touch
        B[lo16:hi16] = Bw
        del calls[:]
        got = A @ B
        out = asdistarray(np.full((m, k), np.nan, dtype=dt))
        ret = A.dot(B, out=out)
        assert ret is out
        want = [] if m == 1 else [(lo16, (hi16 - lo16, k), (m, k))] * 2
        assert calls == want and lo16 == 16
        for C in (got.local, out.local):
            assert C.dtype == _tdt(dt)
            w.check(C, ref.values, dc.dense_tol(ref, dt), f"k {k}")
            assert torch.all(C[empty] == 0)
    w.report()


# -- rSpMM --------------------------------------------------------------------------
@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("side", dc.SPARSE_SIDES)
def test_rspmm_extents_and_hot_column(side, dt, idt):
    """C = A_dense @ B_csr, one wave per entry of B with lanes striding over
    kd = 1 .. 130: empty rows of B under the row search, columns nothing
    lands on, and one column that takes an atomic from every non-empty row
    (more than 500 at side = 600)."""
    from sparse.ops import local as ops

    w = _Worst()
    M = dc.rspmm_case(dt, side)
    Bl = _local(M, idt)
    for kd in dc.EXTENTS:
        A = dc.rand_dense(300 + kd, (kd, side), dt)
        ref = _cached(("rspmm", dt, side, kd), lambda: dc.ref_rspmm(A, M))
        C = ops.rspmm(_dev(A), Bl)
        assert C.dtype == _tdt(dt)
        w.check(C, ref.values, dc.dense_tol(ref, dt),
                f"kd {kd}")
        assert torch.all(C[:, _dev(ref.n[0] == 0)] == 0)
    w.report()


# -- CSC column split ---------------------------------------------------------------
@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("side", dc.SPARSE_SIDES)
def test_csc_spmv_spmm_row_window(side, dt, idt):
    """Partial y / C over the row window [rlo, rlo + 300), rlo 0 and 1000:
    empty columns, rows nothing lands on, one row that takes an atomic from
    every non-empty column, k = 1 .. 130 over the lane stride."""
    from sparse.ops import local as ops

    w = _Worst()
    for rlo in dc.CSC_RLOS:
        rhi = rlo + dc.OTHER_SIDE
        M = dc.csc_case(dt, side, rlo)
        colptr, rowidx = _dev(M.indptr), _dev(M.indices).to(idt)
        vals = _dev(M.values)
        x = dc.rand_dense(400, (side,), dt)
        ref = _cached(("cscv", dt, side, rlo),
                      lambda: dc.ref_csc(M, x, rlo, rhi))
        y = ops.csc_spmv(colptr, rowidx, vals, _dev(x), rlo, rhi)
        w.check(y, ref.values, dc.dense_tol(ref, dt), f"spmv rlo {rlo}")
        assert torch.all(y[_dev(ref.n == 0)] == 0)
        for k in dc.EXTENTS:
            X = dc.rand_dense(400 + k, (side, k), dt)
            ref = _cached(("cscm", dt, side, rlo, k),
                          lambda: dc.ref_csc(M, X, rlo, rhi))
            C = ops.csc_spmm(colptr, rowidx, vals, _dev(X), rlo, rhi)
            w.check(C, ref.values,
                    dc.dense_tol(ref, dt),
                    f"spmm rlo {rlo} k {k}")
            assert torch.all(C[_dev(ref.n[:, 0] == 0)] == 0)
    w.report()


# -- non-canonical constructor input --------------------------------------------------
@pytest.mark.parametrize("kind", dc.NONCANON_KINDS)
def test_noncanonical_input_routes(kind, monkeypatch):
    """The API-level checks of test_dense_cases.py on the GPU, where the
    banded input runs on its DIA mirror and the block input through the
    MFMA route at k = 16 (the two mirrors that kept only the last of a
    set of duplicates)."""
    from sparse import csc_array, csr_array, kernels

    calls = []
    inner = kernels.bsr_spmm

    def rec(bm, Bw, C, col_lo):
        calls.append(tuple(Bw.shape))
        return inner(bm, Bw, C, col_lo)

    monkeypatch.setattr(kernels, "bsr_spmm", rec)
    built = dc.check_noncanonical(kind, csr_array, csc_array)
    assert len(built) == 2 and all(A._values.is_cuda for A in built)
    if kind == "banded":
        assert all(A._dia() is not None for A in built)
    if kind == "blocks":
        assert calls == [(64, 16)] * 2
