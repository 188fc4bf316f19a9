"""CPU checks of utils/spout_cases.py: the generated SpGEMM / elementwise /
row-search inputs meet the preconditions test_spout_gpu.py relies on, the
tolerance is tight enough to see one wrong term, and the plain references
agree with scipy wherever scipy keeps the entry.
"""
import numpy as np
import pytest
import scipy.sparse as sps

from utils.common import types
from utils import spout_cases as sc


def _scipy(M, col_lo=0, dt=None):
    v = M.values if dt is None else M.values.astype(dt)
    return sps.csr_matrix((v, M.indices - col_lo, M.indptr),
                          shape=(M.nrows, M.ncols - col_lo))


def _down(dt):
    """The widest dtype scipy multiplies in."""
    return (np.complex128 if np.issubdtype(np.dtype(dt), np.complexfloating)
            else np.float64)


# -- preconditions ------------------------------------------------------------
def test_case_counts():
    cases = sc.spgemm_case_list()
    kinds = [c.kind for c in cases]
    assert kinds.count("bin") == 129  # 43 (ub, na) pairs x 3 column pools
    assert kinds.count("checked") == 4 and kinds.count("cancel") == 2
    s = sc.spgemm_set(np.float64)
    assert s.A.nrows == len(cases) == 137
    for ub in sc.UBS:
        got = {(c.na, c.stride) for c in cases if c.kind == "bin" and c.ub == ub}
        assert got == {(na, st) for na in sc.NAS if na <= ub
                       for st in (1, 4096)}
    # the stride-4096 pool of the 1024-product rows sets the width, ~4.2 M
    assert s.B.ncols == 1023 * 4096 + 1


@pytest.mark.parametrize("variant", ["base", "col_lo", "wide"])
@pytest.mark.parametrize("dt", types)
def test_spgemm_preconditions(dt, variant):
    """ub, A-row length and distinct count of every row, recomputed from the
    arrays, are what the case asked for."""
    s = sc.spgemm_set(dt, variant)
    ref = sc.spgemm_ref(dt, variant)
    assert s.A.values.dtype == s.B.values.dtype == np.dtype(dt)
    assert s.a_col_lo == (sc.A_COL_LO if variant == "col_lo" else 0)
    if s.a_col_lo:
        assert s.A.indices.min() == s.a_col_lo
    ub = sc.row_ub(s)
    na = np.diff(s.A.indptr)
    distinct = np.diff(ref.indptr)
    assert ub.tolist() == [c.ub for c in s.cases]
    assert na.tolist() == [c.na for c in s.cases]
    assert distinct.tolist() == [c.distinct for c in s.cases]
    assert np.all(ref.n >= 1) and ref.n.sum() == ub.sum()
    sc.check_csr(sc.Csr(ref.indptr, ref.indices, ref.values, s.A.nrows,
                        s.B.ncols))
    mag = np.abs(np.concatenate([s.A.values, s.B.values]).astype(sc.wide(dt)))
    e = 4 * sc.real_eps(dt)
    assert mag.min() >= 0.5 * (1 - e) and mag.max() <= 2 * (1 + e)
    for i, c in enumerate(s.cases):
        cols = ref.indices[ref.indptr[i]: ref.indptr[i + 1]]
        if c.stride == 4096:
            assert np.all(cols % 4096 == 0)  # every key hashes to slot 0
        if c.kind == "cancel":
            assert np.all(ref.values[ref.indptr[i]: ref.indptr[i + 1]] == 0)
            assert np.all(ref.n[ref.indptr[i]: ref.indptr[i + 1]] == 2)
    if variant == "wide":
        assert ref.indices.max() >= (1 << 33) - (1 << 28)
        assert s.B.ncols > (1 << 33) - (1 << 28)


def test_col_lo_variant_is_the_same_product():
    a, b = sc.spgemm_ref(np.float64, "base"), sc.spgemm_ref(np.float64, "col_lo")
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    sa, sb = sc.spgemm_set(np.float64, "base"), sc.spgemm_set(np.float64, "col_lo")
    assert np.array_equal(sa.A.indices + sc.A_COL_LO, sb.A.indices)
    assert np.array_equal(sa.B.indices, sb.B.indices)


@pytest.mark.parametrize("variant", ["base", "wide"])
def test_spgemm_routing_and_partial_blocks(variant):
    """Which table the cuts (32 / 128 / 512 / 1024 products, 2048 distinct
    columns) send each row to; both sides of every cut are present; the last
    block of every launch is partly filled."""
    s = sc.spgemm_set(np.float64, variant)
    ub = sc.row_ub(s)
    distinct = np.diff(sc.spgemm_ref(np.float64, variant).indptr)
    for itemsize in (4, 8, 16):
        tables = [sc.expected_table(int(u), int(d), itemsize)
                  for u, d in zip(ub, distinct)]
        for (cut, table, rpb), nxt in zip(sc.BIN_CUTS, (256, 1024, 2048, None)):
            rows = [i for i, t in enumerate(tables) if t == table]
            assert max(ub[rows]) == cut  # a row sits on the upper edge ...
            if nxt:                      # ... and one just past it
                assert min(ub[[i for i, t in enumerate(tables) if t == nxt]]
                           ) == cut + 1
            assert len(rows) % rpb != 0, (table, len(rows))
            # the table load reaches exactly one half at the upper edge
            assert max(distinct[rows]) == table // 2
        big = [i for i in range(len(ub)) if ub[i] > 1024]
        routed = {int(distinct[i]): tables[i] for i in big}
        if itemsize == 16:
            assert set(routed.values()) == {"reroute"}
        elif variant == "base":
            assert routed == {1025: 4096, 2048: 4096, 2049: "reroute",
                              4097: "reroute"}
            assert min(ub[big]) == 1025
        else:
            assert routed == {2049: "reroute"}
    lens = {int(n) for n in np.diff(s.A.indptr)}
    assert lens >= ({1, 17, 65} if variant == "wide" else set(sc.NAS))


# -- sensitivity ---------------------------------------------------------------
@pytest.mark.parametrize("variant", ["base", "wide"])
def test_spgemm_tolerance_sees_one_wrong_term(variant):
    """float32, the worst case: the tolerance of every entry is below a tenth
    of the smallest product that contributes to it, so a dropped, doubled or
    wrong-signed term always fails."""
    ref = sc.spgemm_ref(np.float32, variant)
    tol = sc.spgemm_tol(ref, np.float32)
    ratio = tol / ref.pmin
    print(f"worst tolerance / smallest contributing product: "
          f"{float(ratio.max()):.4f}; smallest product {float(ref.pmin.min()):.4f}")
    assert np.all(tol < 0.1 * ref.pmin)
    assert ref.pmin.min() >= 0.25 * (1 - 1e-6)


# -- cross-check against scipy ------------------------------------------------
@pytest.mark.parametrize("variant", ["base", "col_lo"])
@pytest.mark.parametrize("dt", types)
def test_ref_spgemm_vs_scipy(dt, variant):
    s = sc.spgemm_set(dt, variant)
    ref = sc.spgemm_ref(dt, variant)
    w = _down(dt)
    C = (_scipy(s.A, s.a_col_lo, w)[:, : s.B.nrows] @ _scipy(s.B, 0, w)).tocsr()
    C.sort_indices()
    tol = sc.spgemm_tol(ref, w)  # scipy accumulates in double
    for i, c in enumerate(s.cases):
        r0, r1 = ref.indptr[i], ref.indptr[i + 1]
        got_c = C.indices[C.indptr[i]: C.indptr[i + 1]]
        got_v = C.data[C.indptr[i]: C.indptr[i + 1]]
        if c.kind == "cancel":
            # the stated exception: scipy drops what the reference keeps
            assert len(got_c) == 0 and r1 - r0 == c.distinct > 0
            continue
        assert np.array_equal(got_c, ref.indices[r0:r1])
        err = np.abs(got_v.astype(sc.wide(dt)) - ref.values[r0:r1])
        assert np.all(err <= tol[r0:r1])


def test_scipy_drops_cancelled_entries():
    a = sps.csr_matrix(np.array([[1.0, -1.0]]))
    b = sps.csr_matrix(np.array([[2.0, 3.0], [2.0, 3.0]]))
    assert (a @ b).nnz == 0 and (a + (-a)).nnz == 0
    r = sc.ref_spgemm(a.indptr.astype(np.int64), a.indices.astype(np.int64),
                      a.data, b.indptr.astype(np.int64),
                      b.indices.astype(np.int64), b.data)
    assert r.indptr.tolist() == [0, 2] and r.indices.tolist() == [0, 1]
    assert np.all(r.values == 0) and r.n.tolist() == [2, 2]
    assert r.S.tolist() == [4.0, 6.0]


@pytest.mark.parametrize("m", [255, 256, 257])
def test_elem_pair_rows(m):
    A, B = sc.elem_pair(np.float64, m)
    assert A.nrows == B.nrows == m and A.ncols == B.ncols == sc.ELEM_NCOLS
    kinds = {sc.elem_kind(i) for i in range(m)}
    assert kinds == set(sc.ELEM_KINDS) | {"long"}
    la, lb = np.diff(A.indptr), np.diff(B.indptr)
    r = sc.ELEM_LONG_ROW
    assert la[r] >= 3000 and lb[r] >= 3000
    assert la[r - 1] == lb[r - 1] == la[r + 1] == lb[r + 1] == 0
    for i in range(m):
        ca = set(A.indices[A.indptr[i]: A.indptr[i + 1]].tolist())
        cb = set(B.indices[B.indptr[i]: B.indptr[i + 1]].tolist())
        k = sc.elem_kind(i)
        if k == "both_empty":
            assert not ca and not cb
        elif k == "a_empty":
            assert not ca and cb
        elif k == "b_empty":
            assert ca and not cb
        elif k in ("identical", "negated"):
            assert ca == cb and ca
        elif k == "interleaved":
            assert not (ca & cb) and {c + 1 for c in ca} == cb
        elif k == "a_in_b":
            assert ca < cb
        elif k == "b_in_a":
            assert cb < ca
        elif k == "edges":
            assert {0, A.ncols - 1} <= ca & cb
        if k == "negated":
            s, e = A.indptr[i], A.indptr[i + 1]
            assert np.array_equal(B.values[B.indptr[i]: B.indptr[i + 1]],
                                  -A.values[s:e])


@pytest.mark.parametrize("dt", types)
def test_ref_elementwise_vs_scipy(dt):
    """Rows without exact cancellation: same structure as scipy, values
    within one rounding of the working dtype; "negated" rows are the stated
    exception for add."""
    A, B = sc.elem_pair(dt, 257)
    w = _down(dt)
    a, b = _scipy(A, dt=w), _scipy(B, dt=w)
    eps = sc.real_eps(w)
    neg = [i for i in range(A.nrows) if sc.elem_kind(i) == "negated"]
    for (alpha, beta) in sc.ADD_SCALARS:
        R = sc.ref_add(A, B, alpha, beta)
        sc.check_csr(R)
        S = (alpha * a + beta * b).tocsr()
        S.sort_indices()
        for i in range(A.nrows):
            r0, r1 = R.indptr[i], R.indptr[i + 1]
            gc = S.indices[S.indptr[i]: S.indptr[i + 1]]
            gv = S.data[S.indptr[i]: S.indptr[i + 1]]
            if (alpha, beta) == (1.0, 1.0) and i in neg:
                assert len(gc) == 0 and r1 - r0 > 0
                assert np.all(R.values[r0:r1] == 0)
                continue
            assert np.array_equal(gc, R.indices[r0:r1])
            err = np.abs(gv.astype(sc.wide(dt)) - R.values[r0:r1])
            assert np.all(err <= eps * np.abs(R.values[r0:r1]))
    assert neg
    R = sc.ref_mult(A, B)
    sc.check_csr(R)
    S = a.multiply(b).tocsr()
    S.sort_indices()
    assert np.array_equal(S.indptr, R.indptr)
    assert np.array_equal(S.indices, R.indices)
    err = np.abs(S.data.astype(sc.wide(dt)) - R.values)
    assert np.all(err <= 2 * eps * np.abs(R.values))
    # the same expression in the working dtype is what a one-rounding
    # kernel returns; it is within one rounding of the long double value
    Rd = sc.ref_add(A, B, 2.0, -0.5, dt=dt)
    Rw = sc.ref_add(A, B, 2.0, -0.5)
    assert Rd.values.dtype == np.dtype(dt)
    assert np.array_equal(Rd.indices, Rw.indices)
    err = np.abs(Rd.values.astype(sc.wide(dt)) - Rw.values)
    assert np.all(err <= sc.real_eps(dt) * np.abs(Rw.values))


def test_ref_add_all_empty_and_no_rows():
    A, _ = sc.elem_pair(np.float64, 255)
    Z = sc.empty_csr(A.nrows, A.ncols, np.float64)
    R = sc.ref_add(A, Z, 2.0, -0.5)
    assert np.array_equal(R.indptr, A.indptr)
    assert np.array_equal(R.indices, A.indices)
    assert np.array_equal(R.values, 2 * A.values.astype(np.longdouble))
    assert sc.ref_mult(A, Z).nnz == 0 and sc.ref_mult(Z, A).nnz == 0
    E = sc.empty_csr(0, 10, np.float64)
    assert sc.ref_add(E, E).indptr.tolist() == [0]
    assert sc.ref_mult(E, E).indptr.tolist() == [0]


@pytest.mark.parametrize("nnz", [255, 256, 257])
@pytest.mark.parametrize("col_lo", [0, 1000])
def test_rowsearch_cases(nnz, col_lo):
    M = sc.rowsearch_csr(np.float64, nnz, col_lo)
    lens = np.diff(M.indptr)
    assert M.nnz == nnz and M.nrows == sc.ROWSEARCH_M
    assert np.all(lens[list(sc.ROWSEARCH_EMPTY)] == 0)
    assert lens[0] == 0 and lens[-1] == 0 and lens[30] == 0
    assert np.all(np.delete(lens, sc.ROWSEARCH_EMPTY) >= 1)
    assert len(set(lens.tolist())) > 3
    assert M.indices.min() >= col_lo and M.indices.max() < col_lo + 50


@pytest.mark.parametrize("dt", types)
def test_ref_rowsearch_vs_numpy(dt):
    """mult_dense / sddmm references against a dense numpy evaluation in
    double."""
    w = _down(dt)
    col_lo, kd = 1000, 8
    M = sc.rowsearch_csr(dt, 257, col_lo)
    rows = np.repeat(np.arange(M.nrows), np.diff(M.indptr))
    Dm = sc.rand_dense(1, (M.nrows, M.ncols), dt)
    got = sc.ref_mult_dense(M, Dm)
    want = M.values.astype(w) * Dm.astype(w)[rows, M.indices]
    assert np.all(np.abs(got - want.astype(sc.wide(dt)))
                  <= 2 * sc.real_eps(w) * np.abs(got))
    C = sc.rand_dense(2, (M.nrows, kd), dt)
    D = sc.rand_dense(3, (kd, sc.ROWSEARCH_WIDTH), dt)
    got, T = sc.ref_sddmm(M, C, D, col_lo)
    full = C.astype(w) @ D.astype(w)
    want = M.values.astype(w) * full[rows, M.indices - col_lo]
    bound = (kd + 2) * sc.real_eps(w) * np.abs(M.values.astype(w)) * T
    assert np.all(np.abs(got - want.astype(sc.wide(dt))) <= bound)
    assert np.all(T >= kd * 0.25 * (1 - 1e-6)) and np.all(T <= kd * 4 * (1 + 1e-6))
