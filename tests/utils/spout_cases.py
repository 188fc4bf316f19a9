"""Inputs and plain references for the kernels that produce a new sparse
structure: SpGEMM, add / multiply row merges, mult_dense and SDDMM.  Shared by
test_spout_cases.py (CPU checks of this file) and test_spout_gpu.py.

numpy only; nothing here imports the code under test.

Structure contract of the references: an entry exists as soon as one operand
term touches it, whatever its value (union for add, intersection for
multiply, every touched column for SpGEMM).  scipy drops entries whose value
comes out exactly zero, so it cannot be the structural oracle.

Inputs are drawn in the target dtype (exactly representable) and cast UP to
long double for the references; results are compared by casting them up too.
Values have magnitude in [0.5, 2] with random sign (random phase if complex).
"""
import functools
from typing import NamedTuple

import numpy as np

INT = np.int64

# the SpGEMM routing the cases are placed against: product upper bound ub ->
# LDS table size, rows per block
BIN_CUTS = ((32, 64, 16), (128, 256, 4), (512, 1024, 4), (1024, 2048, 2))
CHECKED_TABLE = 4096      # rows with ub > 1024 try this table ...
CHECKED_DISTINCT = 2048   # ... which accepts at most this many columns

UBS = (32, 33, 128, 129, 512, 513, 1024)
NAS = (1, 15, 16, 17, 63, 64, 65)
CHECKED_NA = 65
CHECKED_DISTINCTS = (2048, 2049, 4097)
A_COL_LO = 1000


def wide(dt):
    return (np.clongdouble if np.issubdtype(np.dtype(dt), np.complexfloating)
            else np.longdouble)


def real_eps(dt):
    return float(np.finfo(np.dtype(dt)).eps)


def rand_values(rng, n, dt):
    """n values of dtype dt, magnitude in [0.5, 2], random sign / phase."""
    dt = np.dtype(dt)
    mag = rng.uniform(0.5, 2.0, n)
    if np.issubdtype(dt, np.complexfloating):
        v = mag * np.exp(2j * np.pi * rng.random(n))
    else:
        v = mag * rng.choice([-1.0, 1.0], n)
    return v.astype(dt)


class Csr(NamedTuple):
    indptr: np.ndarray   # int64, nrows + 1
    indices: np.ndarray  # int64, sorted and duplicate-free within a row
    values: np.ndarray
    nrows: int
    ncols: int

    @property
    def nnz(self):
        return int(self.indptr[-1])


def csr_from_rows(rows, ncols, dt):
    """Csr from a list of (cols, vals) per row (cols sorted)."""
    ip = np.zeros(len(rows) + 1, dtype=INT)
    for i, (c, _) in enumerate(rows):
        ip[i + 1] = ip[i] + len(c)
    ix = (np.concatenate([np.asarray(c, dtype=INT) for c, _ in rows])
          if rows else np.zeros(0, INT))
    vs = (np.concatenate([np.asarray(v, dtype=dt) for _, v in rows])
          if rows else np.zeros(0, dt))
    return Csr(ip, ix.astype(INT), vs.astype(dt), len(rows), int(ncols))


def check_csr(M):
    """indptr consistent, columns in range, strictly increasing per row."""
    ip, ix = M.indptr, M.indices
    assert ip[0] == 0 and len(ip) == M.nrows + 1 and np.all(np.diff(ip) >= 0)
    assert ip[-1] == len(ix) == len(M.values)
    if len(ix):
        assert ix.min() >= 0 and ix.max() < M.ncols
        inner = np.ones(len(ix), dtype=bool)
        inner[ip[:-1][ip[:-1] < len(ix)]] = False  # first entry of each row
        assert np.all((np.diff(ix) > 0) | ~inner[1:])


# -- references ---------------------------------------------------------------
class SpgemmRef(NamedTuple):
    indptr: np.ndarray
    indices: np.ndarray
    values: np.ndarray   # long double / complex long double
    n: np.ndarray        # products landing on the entry
    S: np.ndarray        # sum of |a| |b| over those products
    pmin: np.ndarray     # smallest |a| |b| among them


def ref_spgemm(aip, aix, av, bip, bix, bv, a_col_lo=0):
    """C = A @ B by rows with one dict per row, accumulated in long double.
    B's row k is global row a_col_lo + k.  Entries are kept whatever their
    value."""
    w = wide(np.result_type(av.dtype, bv.dtype))
    avw, bvw = av.astype(w), bv.astype(w)
    aab, bab = np.abs(avw), np.abs(bvw)
    aip, bip = aip.tolist(), bip.tolist()
    aix, bix = aix.tolist(), bix.tolist()
    m = len(aip) - 1
    indptr = np.zeros(m + 1, dtype=INT)
    cols, vals, ns, Ss, pm = [], [], [], [], []
    for i in range(m):
        acc = {}
        for p in range(aip[i], aip[i + 1]):
            k = aix[p] - a_col_lo
            a, aa = avw[p], aab[p]
            for q in range(bip[k], bip[k + 1]):
                prod, mag = a * bvw[q], aa * bab[q]
                e = acc.get(bix[q])
                if e is None:
                    acc[bix[q]] = [prod, 1, mag, mag]
                else:
                    e[0] += prod
                    e[1] += 1
                    e[2] += mag
                    if mag < e[3]:
                        e[3] = mag
        for c in sorted(acc):
            e = acc[c]
            cols.append(c)
            vals.append(e[0])
            ns.append(e[1])
            Ss.append(e[2])
            pm.append(e[3])
        indptr[i + 1] = len(cols)
    return SpgemmRef(indptr, np.array(cols, dtype=INT), np.array(vals, dtype=w),
                     np.array(ns, dtype=INT), np.array(Ss, dtype=np.longdouble),
                     np.array(pm, dtype=np.longdouble))


def _row_dict(M, i, v):
    s, e = int(M.indptr[i]), int(M.indptr[i + 1])
    return dict(zip(M.indices[s:e].tolist(), v[s:e]))


def _calc_dtype(A, B, dt):
    return np.dtype(wide(np.result_type(A.values.dtype, B.values.dtype))
                    if dt is None else dt)


def ref_add(A, B, alpha=1.0, beta=1.0, dt=None):
    """alpha A + beta B on the UNION pattern.  Computed in long double, or,
    with dt given, as the same expression in dt (one rounding per entry when
    the scalings are exact)."""
    w = _calc_dtype(A, B, dt).type
    av, bv = A.values.astype(w), B.values.astype(w)
    al, be = w(alpha), w(beta)
    rows = []
    for i in range(A.nrows):
        da, db = _row_dict(A, i, av), _row_dict(B, i, bv)
        cols = sorted(set(da) | set(db))
        out = []
        for c in cols:
            if c in da and c in db:
                out.append(al * da[c] + be * db[c])
            elif c in da:
                out.append(al * da[c])
            else:
                out.append(be * db[c])
        rows.append((cols, out))
    return csr_from_rows(rows, A.ncols, w)


def ref_mult(A, B, dt=None):
    """A .* B on the INTERSECTION pattern (long double, or dt)."""
    w = _calc_dtype(A, B, dt).type
    av, bv = A.values.astype(w), B.values.astype(w)
    rows = []
    for i in range(A.nrows):
        da, db = _row_dict(A, i, av), _row_dict(B, i, bv)
        cols = sorted(set(da) & set(db))
        rows.append((cols, [da[c] * db[c] for c in cols]))
    return csr_from_rows(rows, A.ncols, w)


def ref_mult_dense(A, D, dt=None):
    """values[p at (i, j)] * D[i, j] on A's pattern (long double, or dt)."""
    w = np.dtype(wide(np.result_type(A.values.dtype, D.dtype))
                 if dt is None else dt).type
    av, Dw = A.values.astype(w), D.astype(w)
    out = np.zeros(A.nnz, dtype=w)
    for i in range(A.nrows):
        for p in range(int(A.indptr[i]), int(A.indptr[i + 1])):
            out[p] = av[p] * Dw[i, int(A.indices[p])]
    return out


def ref_sddmm(A, C, D, col_lo=0):
    """values[p at (i, j)] * (C[i, :] @ D[:, j - col_lo]) on A's pattern in
    long double; D is the column block [col_lo, col_lo + D.shape[1]).  Also
    returns T[p] = sum_t |C[i, t]| |D[t, j - col_lo]|."""
    w = wide(np.result_type(A.values.dtype, C.dtype, D.dtype))
    av, Cw, Dw = A.values.astype(w), C.astype(w), D.astype(w)
    Ca, Da = np.abs(Cw), np.abs(Dw)
    out = np.zeros(A.nnz, dtype=w)
    T = np.zeros(A.nnz, dtype=np.longdouble)
    kd = C.shape[1]
    for i in range(A.nrows):
        for p in range(int(A.indptr[i]), int(A.indptr[i + 1])):
            j = int(A.indices[p]) - col_lo
            acc, t_acc = w(0), np.longdouble(0)
            for t in range(kd):
                acc += Cw[i, t] * Dw[t, j]
                t_acc += Ca[i, t] * Da[t, j]
            out[p] = av[p] * acc
            T[p] = t_acc
    return out, T


# -- SpGEMM boundary set ------------------------------------------------------
class SpgemmCase(NamedTuple):
    kind: str      # "bin" | "checked" | "empty" | "ub0" | "cancel"
    ub: int        # products of the row = sum of the touched B-row lengths
    na: int        # A-row length
    distinct: int  # columns of the C row
    stride: int    # spacing of the column pool
    base: int = 0  # first column of the pool


def spgemm_case_list(variant="base"):
    """One case per row of A, in row order."""
    cases = []
    if variant == "wide":
        # int64 only: pool columns spread up to 2^33 (odd stride, so the
        # keys scatter over the table)
        for ub in UBS:
            for na in (1, 17, 65):
                if na <= ub:
                    cases.append(SpgemmCase("bin", ub, na, ub,
                                            ((1 << 33) // ub) | 1))
        d = 2049
        cases.append(SpgemmCase("checked", d + 700, CHECKED_NA, d,
                                ((1 << 33) // d) | 1))
    else:
        k = 0
        for ub in UBS:
            for na in NAS:
                if na > ub:
                    continue
                heavy = max(-(-ub // na), min(ub, 7))
                for distinct, stride in ((ub, 1), (heavy, 1), (ub, 4096)):
                    # stride-1 pools start anywhere; stride-4096 pools hold
                    # multiples of 4096 only (all hash to slot 0)
                    base = 0 if stride != 1 else 37 * k
                    cases.append(SpgemmCase("bin", ub, na, distinct, stride,
                                            base))
                    k += 1
        for d in CHECKED_DISTINCTS:
            cases.append(SpgemmCase("checked", d + 700, CHECKED_NA, d, 1))
        # the first product count past the last cut
        cases.append(SpgemmCase("checked", 1025, CHECKED_NA, 1025, 1))
    cases.append(SpgemmCase("empty", 0, 0, 0, 1))
    cases.append(SpgemmCase("ub0", 0, 3, 0, 1))
    # +v / -v against two identical B rows: small (64-entry table) and large
    # (2048-entry table)
    cases.append(SpgemmCase("cancel", 10, 2, 5, 1, 11))
    cases.append(SpgemmCase("cancel", 600, 2, 300, 1, 123))
    return cases


class SpgemmSet(NamedTuple):
    A: Csr             # column ids already shifted by a_col_lo
    B: Csr
    a_col_lo: int
    cases: tuple


@functools.lru_cache(maxsize=None)
def spgemm_set(dt, variant="base"):
    """The boundary set for value dtype dt.  variant: "base", "col_lo" (A's
    column ids shifted up by A_COL_LO, same B) or "wide" (columns up to
    2^33).  Built once; do not modify."""
    dt = np.dtype(dt)
    cases = spgemm_case_list("wide" if variant == "wide" else "base")
    rng = np.random.default_rng(20240 + dt.num)
    a_rows, b_rows = [], []
    ncols = 1
    for cs in cases:
        k0 = len(b_rows)
        if cs.kind in ("empty",):
            a_rows.append(([], []))
            continue
        if cs.kind == "ub0":
            b_rows += [([], [])] * cs.na
            a_rows.append((list(range(k0, k0 + cs.na)),
                           rand_values(rng, cs.na, dt)))
            continue
        if cs.kind == "cancel":
            cols = cs.base + cs.stride * np.arange(cs.distinct)
            bv = rand_values(rng, cs.distinct, dt)
            b_rows += [(cols, bv), (cols.copy(), bv.copy())]
            v = rand_values(rng, 1, dt)
            a_rows.append(([k0, k0 + 1], np.array([v[0], -v[0]], dtype=dt)))
            ncols = max(ncols, int(cols[-1]) + 1)
            continue
        # the B-row lengths split ub evenly; the pool is walked cyclically
        lens = [cs.ub // cs.na + (1 if j < cs.ub % cs.na else 0)
                for j in range(cs.na)]
        assert max(lens) <= cs.distinct <= cs.ub
        walk = cs.base + cs.stride * (np.arange(cs.ub) % cs.distinct)
        ncols = max(ncols, int(walk.max()) + 1)
        s = 0
        for ln in lens:
            b_rows.append((np.sort(walk[s: s + ln]), rand_values(rng, ln, dt)))
            s += ln
        a_rows.append((list(range(k0, k0 + cs.na)),
                       rand_values(rng, cs.na, dt)))
    lo = A_COL_LO if variant == "col_lo" else 0
    B = csr_from_rows(b_rows, ncols, dt)
    A = csr_from_rows([(np.asarray(c, dtype=INT) + lo, v) for c, v in a_rows],
                      B.nrows + lo, dt)
    check_csr(A)
    check_csr(B)
    return SpgemmSet(A, B, lo, tuple(cases))


@functools.lru_cache(maxsize=None)
def spgemm_ref(dt, variant="base"):
    """ref_spgemm of spgemm_set(dt, variant), computed once."""
    s = spgemm_set(dt, variant)
    return ref_spgemm(s.A.indptr, s.A.indices, s.A.values, s.B.indptr,
                      s.B.indices, s.B.values, s.a_col_lo)


def row_ub(s):
    """Product upper bound of each A row, recomputed from the arrays."""
    blen = np.diff(s.B.indptr)
    per = np.concatenate([[0], np.cumsum(blen[s.A.indices - s.a_col_lo])])
    return per[s.A.indptr[1:]] - per[s.A.indptr[:-1]]


def expected_table(ub, distinct, itemsize):
    """Where the wrapper's cuts send a row: the LDS table size, or
    "reroute" (dense-workspace / expand-sort-reduce fallback)."""
    for cut, table, _ in BIN_CUTS:
        if ub <= cut:
            return table
    if itemsize <= 8 and distinct <= CHECKED_DISTINCT:
        return CHECKED_TABLE
    return "reroute"


def sub_rows(M, rows):
    """The Csr made of the given rows of M."""
    return csr_from_rows(
        [(M.indices[M.indptr[i]: M.indptr[i + 1]],
          M.values[M.indptr[i]: M.indptr[i + 1]]) for i in rows],
        M.ncols, M.values.dtype)


def ref_rows(ref, rows):
    """The SpgemmRef restricted to the given rows."""
    seg = [np.arange(ref.indptr[i], ref.indptr[i + 1]) for i in rows]
    pos = np.concatenate(seg) if seg else np.zeros(0, INT)
    ip = np.concatenate([[0], np.cumsum([len(x) for x in seg])]).astype(INT)
    return SpgemmRef(ip, *(f[pos] for f in ref[1:]))


def spgemm_tol(ref, dt):
    """(n + 2) eps S per entry: n roundings of products and sums in any
    atomic order plus the complex-product factor; at most about 4x the
    rigorous gamma_n bound."""
    return (ref.n + 2) * np.longdouble(real_eps(dt)) * ref.S


# -- elementwise set ----------------------------------------------------------
ELEM_NCOLS = 6000
ELEM_LONG_ROW = 101   # >= 3000 entries, rows 100 and 102 are empty
ELEM_KINDS = ("both_empty", "a_empty", "b_empty", "identical", "interleaved",
              "a_in_b", "b_in_a", "edges", "negated")


def elem_kind(i):
    if i in (ELEM_LONG_ROW - 1, ELEM_LONG_ROW + 1):
        return "both_empty"
    if i == ELEM_LONG_ROW:
        return "long"
    return ELEM_KINDS[i % len(ELEM_KINDS)]


@functools.lru_cache(maxsize=None)
def elem_pair(dt, m=257):
    """(A, B) of m rows holding every row kind of ELEM_KINDS plus one long
    row between two empty ones.  Built once; do not modify."""
    dt = np.dtype(dt)
    n = ELEM_NCOLS
    rng = np.random.default_rng(7700 + dt.num)  # same rows for every m
    ra, rb = [], []

    def pick(k):
        return np.sort(rng.choice(n, k, replace=False))

    for i in range(m):
        kind = elem_kind(i)
        ca = cb = np.zeros(0, INT)
        if kind == "a_empty":
            cb = pick(40)
        elif kind == "b_empty":
            ca = pick(40)
        elif kind == "identical":
            ca = cb = pick(23)
        elif kind == "interleaved":
            c = pick(30) // 2 * 2
            c = np.unique(c)
            ca, cb = c, c + 1
        elif kind == "a_in_b":
            cb = pick(31)
            ca = cb[::3]
        elif kind == "b_in_a":
            ca = pick(31)
            cb = ca[1::2]
        elif kind == "edges":
            ca = np.unique(np.concatenate([[0, n - 1], pick(9)]))
            cb = np.unique(np.concatenate([[0], pick(5), [n - 1]]))
        elif kind == "negated":
            ca = cb = pick(17)
        elif kind == "long":
            ca = pick(3000)
            cb = np.unique(np.concatenate([ca[::2], pick(2600)]))
        va, vb = rand_values(rng, len(ca), dt), rand_values(rng, len(cb), dt)
        if kind == "negated":
            vb = -va
        ra.append((ca, va))
        rb.append((cb, vb))
    A, B = csr_from_rows(ra, n, dt), csr_from_rows(rb, n, dt)
    check_csr(A)
    check_csr(B)
    return A, B


def empty_csr(nrows, ncols, dt):
    return csr_from_rows([([], [])] * nrows, ncols, np.dtype(dt))


ADD_SCALARS = ((1.0, 1.0), (1.0, -1.0), (2.0, -0.5))


# -- row-search set (mult_dense, sddmm) ---------------------------------------
ROWSEARCH_M = 60
ROWSEARCH_EMPTY = tuple(range(0, 7)) + tuple(range(25, 35)) + tuple(range(52, 60))
ROWSEARCH_WIDTH = 50


@functools.lru_cache(maxsize=None)
def rowsearch_csr(dt, nnz, col_lo=0):
    """60 x (col_lo + 50) matrix with nnz entries, all in columns
    [col_lo, col_lo + 50); runs of empty rows at the start, in the middle
    and at the end, uneven lengths elsewhere.  Built once; do not modify."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(9100 + dt.num + nnz)
    full = [i for i in range(ROWSEARCH_M) if i not in ROWSEARCH_EMPTY]
    lens = np.ones(len(full), dtype=INT)
    while lens.sum() < nnz:
        j = int(rng.integers(len(full)))
        if lens[j] < ROWSEARCH_WIDTH:
            lens[j] += 1
    rows = [([], [])] * ROWSEARCH_M
    for i, ln in zip(full, lens):
        c = np.sort(rng.choice(ROWSEARCH_WIDTH, int(ln), replace=False))
        rows[i] = (c + col_lo, rand_values(rng, int(ln), dt))
    M = csr_from_rows(rows, col_lo + ROWSEARCH_WIDTH, dt)
    check_csr(M)
    assert M.nnz == nnz
    return M


def rand_dense(seed, shape, dt):
    rng = np.random.default_rng(seed)
    return rand_values(rng, int(np.prod(shape)), dt).reshape(shape)
