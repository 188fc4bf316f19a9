"""Structure-exact checks of the kernels that produce a new sparse structure
(spgemm.hip, the add / multiply merges of elemwise.hip, mult_dense, sddmm)
against the plain long-double references of utils/spout_cases.py — all @gpu.

Every sparse result must have the reference's indptr and indices exactly
(hence sorted, duplicate-free rows, and entries kept when values cancel);
values are held to derived bounds, never to measured ones.  The ops layer is
called with hand-built LocalCSRs so the tests choose index dtype and offsets.
Nothing here densifies a sparse operand (B has up to 2^33 columns).
"""
import numpy as np
import pytest
import torch

from utils.common import types
from utils import spout_cases as sc

pytestmark = pytest.mark.gpu

_IDX = [torch.int32, torch.int64]
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


def _host(t, dt):
    return t.detach().cpu().numpy().astype(sc.wide(dt))


def _check_structure(C, indptr, indices, idt, dt):
    assert C.indptr.is_cuda and C.indices.is_cuda and C.values.is_cuda
    assert C.indptr.dtype == torch.int64
    assert C.indices.dtype == idt
    assert C.values.dtype == _tdt(dt)
    assert C.nnz == len(indices) == C.indices.numel()
    assert np.array_equal(C.indptr.cpu().numpy(), indptr)
    assert np.array_equal(C.indices.cpu().numpy(), indices)


def _same_structure(C, C2):
    assert torch.equal(C.indptr, C2.indptr)
    assert torch.equal(C.indices, C2.indices)


def _check_spgemm(C, ref, cases, idt, dt):
    _check_structure(C, ref.indptr, ref.indices, idt, dt)
    err = np.abs(_host(C.values, dt) - ref.values)
    tol = sc.spgemm_tol(ref, dt)
    if len(err):
        print(f"max |got - ref| / tolerance: {float((err / tol).max()):.3f}")
    assert np.all(err <= tol)
    got = C.values.cpu().numpy()
    for i, c in enumerate(cases):
        if c.kind == "cancel":  # +v b and -v b: exactly zero, and kept
            assert ref.indptr[i + 1] - ref.indptr[i] == c.distinct
            assert np.all(got[ref.indptr[i]: ref.indptr[i + 1]] == 0)


def _record_fallbacks(monkeypatch):
    """Recording pass-throughs around the two fallbacks of spgemm_csr."""
    from sparse import kernels

    calls = {"dense": [], "esc": []}
    dense, esc = kernels._spgemm_dense_rows, kernels._spgemm_esc

    def rec_dense(A, B, a_col_lo, vdt):
        out = dense(A, B, a_col_lo, vdt)
        calls["dense"].append((A.indices.cpu().numpy().astype(np.int64),
                               out is not None))
        return out

    def rec_esc(A, B, a_col_lo, vdt):
        calls["esc"].append(A.indices.cpu().numpy().astype(np.int64))
        return esc(A, B, a_col_lo, vdt)

    monkeypatch.setattr(kernels, "_spgemm_dense_rows", rec_dense)
    monkeypatch.setattr(kernels, "_spgemm_esc", rec_esc)
    return calls


def _rerouted_rows(s, ref, dt):
    ub, distinct = sc.row_ub(s), np.diff(ref.indptr)
    return [i for i in range(s.A.nrows)
            if sc.expected_table(int(ub[i]), int(distinct[i]),
                                 np.dtype(dt).itemsize) == "reroute"]


def _a_entries(s, rows):
    return (np.concatenate([s.A.indices[s.A.indptr[i]: s.A.indptr[i + 1]]
                            for i in rows]) if rows else np.zeros(0, np.int64))


# -- SpGEMM ---------------------------------------------------------------------
# columns up to 2^33 do not exist in int32: "wide" runs with int64 only
_SPGEMM_RUNS = [("base", torch.int32), ("base", torch.int64),
                ("col_lo", torch.int32), ("col_lo", torch.int64),
                ("wide", torch.int64)]


@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("variant,idt", _SPGEMM_RUNS,
                         ids=[f"{v}-i{torch.iinfo(i).bits}"
                              for v, i in _SPGEMM_RUNS])
def test_spgemm_boundary_set(variant, idt, dt, monkeypatch):
    """Every table size at both sides of its cut, A-row lengths around the
    lane tile, partly filled last blocks, all-new / heavily accumulated /
    all-colliding columns, the checked table at 2048 / 2049 / 4097 distinct
    columns, empty and cancelling rows; with a non-zero a_col_lo; with
    columns up to 2^33 (int64).  Routing: exactly the rows the cuts name
    leave the LDS tables."""
    from sparse.ops import local as ops

    s = sc.spgemm_set(dt, variant)
    ref = sc.spgemm_ref(dt, variant)
    A, B = _local(s.A, idt), _local(s.B, idt)
    calls = _record_fallbacks(monkeypatch)
    C = ops.spgemm(A, B, s.a_col_lo)
    assert (C.nrows, C.ncols) == (s.A.nrows, s.B.ncols)
    _check_spgemm(C, ref, s.cases, idt, dt)
    # white box: which rows left the LDS tables
    rer = _rerouted_rows(s, ref, dt)
    distinct = np.diff(ref.indptr)
    if np.dtype(dt).itemsize == 16:
        assert rer == [i for i, c in enumerate(s.cases) if c.ub > 1024]
    elif variant == "wide":
        assert [int(distinct[i]) for i in rer] == [2049]
    else:
        assert [int(distinct[i]) for i in rer] == [2049, 4097]
    assert len(calls["dense"]) == 1
    sub_ix, took_dense = calls["dense"][0]
    assert np.array_equal(sub_ix, _a_entries(s, rer))
    if variant == "wide":  # a 2^33-wide dense workspace is over the budget
        assert not took_dense and len(calls["esc"]) == 1
        assert np.array_equal(calls["esc"][0], _a_entries(s, rer))
    else:
        assert took_dense and calls["esc"] == []
    _same_structure(C, ops.spgemm(A, B, s.a_col_lo))


@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("mode", ["dense", "esc", "batched"])
def test_spgemm_rerouted_rows_three_ways(mode, dt, idt, monkeypatch):
    """The rows with more than 1024 products through the dense-workspace
    fallback, expand-sort-reduce, and batched expand-sort-reduce."""
    from sparse import kernels
    from sparse.ops import local as ops

    s = sc.spgemm_set(dt, "base")
    rows = [i for i, c in enumerate(s.cases) if c.ub > 1024]
    sub = sc.SpgemmSet(sc.sub_rows(s.A, rows), s.B, 0,
                       tuple(s.cases[i] for i in rows))
    ref = sc.ref_rows(sc.spgemm_ref(dt, "base"), rows)
    rer = _rerouted_rows(sub, ref, dt)
    assert len(rer) == (4 if np.dtype(dt).itemsize == 16 else 2)
    if mode != "dense":
        monkeypatch.setattr(kernels, "_DENSE_FALLBACK_BUDGET", 0)
    if mode == "batched":
        monkeypatch.setattr(kernels, "_ESC_LIMIT", 3000)
    calls = _record_fallbacks(monkeypatch)
    A, B = _local(sub.A, idt), _local(sub.B, idt)
    C = ops.spgemm(A, B, 0)
    _check_spgemm(C, ref, sub.cases, idt, dt)
    assert len(calls["dense"]) == 1
    assert np.array_equal(calls["dense"][0][0], _a_entries(sub, rer))
    assert calls["dense"][0][1] == (mode == "dense")
    if mode == "dense":
        assert calls["esc"] == []
    elif mode == "esc":
        assert len(calls["esc"]) == 1
    else:  # the outer call plus one per single-row batch
        assert len(calls["esc"]) == 1 + len(rer)
    _same_structure(C, ops.spgemm(A, B, 0))


@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", types)
def test_spgemm_degenerate_operands(dt, idt):
    from sparse.ops import local as ops

    s = sc.spgemm_set(dt, "base")
    B = _local(s.B, idt)
    for A in (sc.empty_csr(5, s.B.nrows, dt), sc.empty_csr(0, s.B.nrows, dt)):
        C = ops.spgemm(_local(A, idt), B, 0)
        _check_structure(C, np.zeros(A.nrows + 1, np.int64),
                         np.zeros(0, np.int64), idt, dt)
    # every A entry references an empty B row
    A = sc.sub_rows(s.A, [i for i, c in enumerate(s.cases) if c.kind == "ub0"])
    C = ops.spgemm(_local(A, idt), _local(sc.empty_csr(s.B.nrows, 9, dt), idt), 0)
    _check_structure(C, np.zeros(2, np.int64), np.zeros(0, np.int64), idt, dt)


# -- add / sub / multiply ---------------------------------------------------------
def _complex(dt):
    return np.issubdtype(np.dtype(dt), np.complexfloating)


def _check_mult(C, A, B, idt, dt, key):
    R = _cached(("mult",) + key, lambda: sc.ref_mult(A, B))
    _check_structure(C, R.indptr, R.indices, idt, dt)
    if _complex(dt):
        err = np.abs(_host(C.values, dt) - R.values)
        assert np.all(err <= 2 * sc.real_eps(dt) * np.abs(R.values))
    else:
        Rd = _cached(("mult_dt",) + key, lambda: sc.ref_mult(A, B, dt=dt))
        assert np.array_equal(C.values.cpu().numpy(), Rd.values)


@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("m", [255, 256, 257])
def test_add_sub_multiply_row_kinds(m, dt, idt):
    """Union / intersection merges over every row kind, one thread per row
    in blocks of 256.  Scalings by 1, -1, 2 and -0.5 are exact, so every
    entry carries one rounding: add is bit-equal to numpy in the same dtype."""
    from sparse.ops import local as ops

    A, B = sc.elem_pair(dt, m)
    Ad, Bd = _local(A, idt), _local(B, idt)
    for alpha, beta in sc.ADD_SCALARS:
        R = _cached(("add", dt, m, alpha, beta),
                    lambda: sc.ref_add(A, B, alpha, beta, dt=dt))
        C = ops.add(Ad, Bd, alpha, beta)
        _check_structure(C, R.indptr, R.indices, idt, dt)
        assert np.array_equal(C.values.cpu().numpy(), R.values)
        _same_structure(C, ops.add(Ad, Bd, alpha, beta))
    C = ops.elem_mult(Ad, Bd)
    _check_mult(C, A, B, idt, dt, (dt, m))
    _same_structure(C, ops.elem_mult(Ad, Bd))
    # kept zeros: B = -A rows under add, every one still present
    R = _CACHE[("add", dt, m, 1.0, 1.0)]
    neg = [i for i in range(m) if sc.elem_kind(i) == "negated"]
    assert neg and all(
        R.indptr[i + 1] > R.indptr[i]
        and np.all(R.values[R.indptr[i]: R.indptr[i + 1]] == 0) for i in neg)


@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", types)
def test_add_multiply_empty_operands(dt, idt):
    """An operand without entries, and a pair without rows."""
    from sparse.ops import local as ops

    A, _ = sc.elem_pair(dt, 255)
    Z = sc.empty_csr(A.nrows, A.ncols, dt)
    E = sc.empty_csr(0, A.ncols, dt)
    for X, Y in ((A, Z), (Z, A), (Z, Z), (E, E)):
        Xd, Yd = _local(X, idt), _local(Y, idt)
        R = sc.ref_add(X, Y, 2.0, -0.5, dt=dt)
        C = ops.add(Xd, Yd, 2.0, -0.5)
        _check_structure(C, R.indptr, R.indices, idt, dt)
        assert np.array_equal(C.values.cpu().numpy(), R.values)
        C = ops.elem_mult(Xd, Yd)
        _check_structure(C, np.zeros(X.nrows + 1, np.int64),
                         np.zeros(0, np.int64), idt, dt)


# -- mult_dense / sddmm -------------------------------------------------------------
@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("nnz", [255, 256, 257])
def test_mult_dense_row_search(nnz, dt, idt):
    """One thread per entry finds its row by upper_bound in indptr: runs of
    empty rows at the start, middle and end; nnz around the block size."""
    from sparse.ops import local as ops

    for col_lo in (0, 1000):  # here only a wider matrix
        M = sc.rowsearch_csr(dt, nnz, col_lo)
        D = sc.rand_dense(11 + nnz, (M.nrows, M.ncols), dt)
        out = ops.mult_dense(_local(M, idt), _dev(D))
        assert out.dtype == _tdt(dt) and out.shape == (nnz,)
        if _complex(dt):
            R = _cached(("md", dt, nnz, col_lo),
                        lambda: sc.ref_mult_dense(M, D))
            err = np.abs(_host(out, dt) - R)
            assert np.all(err <= 2 * sc.real_eps(dt) * np.abs(R))
        else:
            R = _cached(("md", dt, nnz, col_lo),
                        lambda: sc.ref_mult_dense(M, D, dt=dt))
            assert np.array_equal(out.cpu().numpy(), R)
    Z = sc.empty_csr(7, 5, dt)
    out = ops.mult_dense(_local(Z, idt), _dev(sc.rand_dense(1, (7, 5), dt)))
    assert out.numel() == 0


@pytest.mark.parametrize("idt", _IDX, ids=["i32", "i64"])
@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("nnz", [255, 256, 257])
def test_sddmm_row_search_and_col_lo(nnz, dt, idt):
    """As above for SDDMM, with D being only the column block
    [col_lo, col_lo + width) of the operand."""
    from sparse.ops import local as ops

    for col_lo in (0, 1000):
        M = sc.rowsearch_csr(dt, nnz, col_lo)
        Md = _local(M, idt)
        absv = np.abs(M.values.astype(sc.wide(dt)))
        for kd in (1, 8, 33):
            C = sc.rand_dense(21 + kd, (M.nrows, kd), dt)
            D = sc.rand_dense(31 + kd, (kd, sc.ROWSEARCH_WIDTH), dt)
            R, T = _cached(("sddmm", dt, nnz, col_lo, kd),
                           lambda: sc.ref_sddmm(M, C, D, col_lo))
            out = ops.sddmm(Md, _dev(C), _dev(D), col_lo)
            assert out.dtype == _tdt(dt) and out.shape == (nnz,)
            err = np.abs(_host(out, dt) - R)
            tol = (kd + 2) * sc.real_eps(dt) * absv * T
            assert np.all(err <= tol)
            # sensitivity: one term of the dot product is at least 0.25
            assert np.all(tol < 0.1 * 0.25 * absv)


# -- the same through the csr_array API (float64) -----------------------------------
def _api_check(C, indptr, indices):
    S = C.to_scipy_sparse_csr()
    assert C._values.is_cuda and S.data.dtype == np.float64
    assert S.nnz == C.nnz == len(indices)
    assert np.array_equal(S.indptr, indptr)
    assert np.array_equal(S.indices, indices)
    return S.data


def test_csr_array_matmul_passes_col_lo(monkeypatch):
    """A @ B where A's smallest column is 1000: _spgemm gathers B's rows
    from 1000 on and passes a_col_lo = 1000 itself."""
    import scipy.sparse as sps

    from sparse import csr_array, kernels

    dt = np.float64
    s, ref = sc.spgemm_set(dt, "col_lo"), sc.spgemm_ref(dt, "col_lo")
    lo = s.a_col_lo
    a = sps.csr_matrix((s.A.values, s.A.indices, s.A.indptr),
                       shape=(s.A.nrows, s.A.ncols))
    b = sps.csr_matrix((s.B.values, s.B.indices, s.B.indptr + 0),
                       shape=(s.B.nrows, s.B.ncols))
    b = sps.vstack([sps.csr_matrix((lo, s.B.ncols), dtype=dt), b]).tocsr()
    assert b.nnz == s.B.nnz
    seen = []
    inner = kernels.spgemm_csr

    def rec(A, B, a_col_lo, vdt):
        seen.append(int(a_col_lo))
        return inner(A, B, a_col_lo, vdt)

    monkeypatch.setattr(kernels, "spgemm_csr", rec)
    C = csr_array(a) @ csr_array(b)
    assert seen == [lo] and lo == 1000
    assert C.shape == (s.A.nrows, s.B.ncols)
    got = _api_check(C, ref.indptr, ref.indices)
    err = np.abs(got.astype(np.longdouble) - ref.values)
    assert np.all(err <= sc.spgemm_tol(ref, dt))
    for i, c in enumerate(s.cases):
        if c.kind == "cancel":
            assert np.all(got[ref.indptr[i]: ref.indptr[i + 1]] == 0)


def test_csr_array_add_sub_multiply():
    import scipy.sparse as sps

    from sparse import csr_array

    dt, m = np.float64, 257
    A, B = sc.elem_pair(dt, m)
    a = csr_array(sps.csr_matrix((A.values, A.indices, A.indptr),
                                 shape=(A.nrows, A.ncols)))
    b = csr_array(sps.csr_matrix((B.values, B.indices, B.indptr),
                                 shape=(B.nrows, B.ncols)))
    for C, beta in ((a + b, 1.0), (a - b, -1.0)):
        R = _cached(("add", dt, m, 1.0, beta),
                    lambda: sc.ref_add(A, B, 1.0, beta, dt=dt))
        assert np.array_equal(_api_check(C, R.indptr, R.indices), R.values)
    R = _cached(("mult_dt", dt, m), lambda: sc.ref_mult(A, B, dt=dt))
    assert np.array_equal(_api_check(a.multiply(b), R.indptr, R.indices),
                          R.values)
