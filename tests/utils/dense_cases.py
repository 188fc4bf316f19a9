"""Inputs and plain references for the kernels that multiply a sparse matrix
by a dense operand: the nnz-split CSR SpMV and its fused dot, the two CSR
SpMM kernels, the MFMA BSR SpMM, rSpMM and the CSC column-split SpMV / SpMM;
plus non-canonical constructor inputs.  Shared by test_dense_cases.py (CPU
checks of this file) and test_dense_gpu.py.

numpy only; nothing here imports the code under test (the API-level checks
at the bottom receive the classes under test as arguments).

Inputs are drawn in the target dtype with magnitude in [0.5, 2] and random
sign / phase (spout_cases.rand_values) and cast UP to long double for the
references.  Every reference returns, per output element, the value, S =
sum |a| |b| over its terms and the term count n.

Tolerance (dense_tol): (n + 2) eps(dt) S, as spgemm_tol: n roundings of
products and sums in ANY order (LDS trees, carries and atomics included)
plus the complex-product factor, about 4x the rigorous gamma_n bound.  With
beta != 0 the term beta * y0 counts as one more term of size |beta y0|.

Fused dot (dot_tol): dot = d0 + sum_r p_r q_r where every q_r (or piece of
a row cut by a block boundary) carries at most (n_r + 2) eps S_r and the
m + nblocks + 1 terms are then summed in any order:
    eps * (sum_r p_r (n_r + 2) S_r + (m + nblocks + 2) S_dot),
    S_dot = |d0| + sum_r p_r S_r      (everything positive there).
"""
import functools
from typing import NamedTuple

import numpy as np

from .spout_cases import (INT, Csr, check_csr, csr_from_rows, rand_values,
                          real_eps, wide)

# -- the kernels' constants the cases are placed against ------------------------
SPMV_BLK = 256                 # threads of an spmv_kernel block
SPMV_NNZ_PER_BLOCK = 2048      # nonzeros one block owns
NXCD = 8                       # xcd_swizzle remaps block ids over 8 XCDs
WAVE = 64
SPMM_SMALLK_MAX = WAVE // 2    # k <= 32: lane-tiled kernel, else 64 lanes / row
SPMM_WAVES_PER_BLOCK = 4
SPMM_MAX_GRID_Y = 65535        # rows / 4 of the wide kernel ride grid.y
BSR = 16                       # block edge of the MFMA mirror
BSR_MIN_FILL = 0.05            # build_bsr gives up below this
BSR_FILL_ANY_K = 0.2           # bsr_profitable at every k from here on

SPMV_NNZS = (1, 2047, 2048, 2049, 4096, 26624, 26625)
SPMV_WINDOW = 6000             # columns a boundary matrix touches
COL_LO = 1000
WIDE_LO = 1 << 33              # int64-only variant: columns start here
SPMV_DOT_NNZS = (4096, 6144, 10240)

SPMM_MS = (1, 255, 256, 257)
SPMM_WINDOW = 400
SPMM_SMALL_KS = (1, 2, 3, 16, 17, 31, 32)
SPMM_WIDE_KS = (33, 64, 65, 129)
SPMM_LARGE_M = 4 * SPMM_MAX_GRID_Y + 5   # 262145: grid.y would be 65537

BSR_MS = (1, 15, 16, 17, 33)
BSR_N = 53
BSR_FIRST_COL = 21
BSR_KS = (16, 17, 31, 32, 33, 48)

EXTENTS = (1, 63, 64, 65, 130)           # dense extent of rSpMM / CSC SpMM
# sparse side of rSpMM (rows) / CSC (columns); 600 is there so that 500
# entries can share one output column / row (a row holds a column once)
SPARSE_SIDES = (255, 256, 257, 600)
HOT_MIN = 500
OTHER_SIDE = 300
CSC_RLOS = (0, 1000)


# -- tolerances -----------------------------------------------------------------
class DenseRef(NamedTuple):
    values: np.ndarray   # long double / complex long double
    S: np.ndarray        # long double
    n: np.ndarray        # int64, broadcastable to values


def dense_tol(ref, dt, extra=None):
    """(n + 2) eps S; extra = |beta y0| adds one term of that size."""
    n, S = ref.n, ref.S
    if extra is not None:
        n, S = n + 1, S + extra
    return (n + 2) * np.longdouble(real_eps(dt)) * S


def dot_tol(ref, p, d0, nblocks, dt):
    pw = np.abs(p.astype(np.longdouble))
    s_dot = abs(np.longdouble(d0)) + np.sum(pw * ref.S)
    return np.longdouble(real_eps(dt)) * (
        np.sum(pw * (ref.n + 2) * ref.S)
        + (len(p) + nblocks + 2) * s_dot)


# -- references -----------------------------------------------------------------
def ref_spmv(M, x, col_lo=0):
    """y = M @ x[window] by rows in long double."""
    w = wide(np.result_type(M.values.dtype, x.dtype))
    prod = M.values.astype(w) * x.astype(w)[M.indices - col_lo]
    mag = np.abs(prod).astype(np.longdouble)
    y = np.zeros(M.nrows, dtype=w)
    S = np.zeros(M.nrows, dtype=np.longdouble)
    ip = M.indptr
    for i in range(M.nrows):
        y[i] = prod[ip[i]: ip[i + 1]].sum()
        S[i] = mag[ip[i]: ip[i + 1]].sum()
    return DenseRef(y, S, np.diff(ip).astype(INT))


def _dense_wide(M, col_lo, width, w):
    D = np.zeros((M.nrows, width), dtype=w)
    rows = np.repeat(np.arange(M.nrows), np.diff(M.indptr))
    D[rows, M.indices - col_lo] = M.values.astype(w)
    return D


def ref_spmm(M, B, col_lo=0):
    """C = M @ B (B = window rows [col_lo, col_lo + len(B))) in long double."""
    w = wide(np.result_type(M.values.dtype, B.dtype))
    D = _dense_wide(M, col_lo, B.shape[0], w)
    Bw = B.astype(w)
    S = np.abs(D).astype(np.longdouble) @ np.abs(Bw).astype(np.longdouble)
    return DenseRef(D @ Bw, S, np.diff(M.indptr).astype(INT)[:, None])


def ref_rspmm(A, M):
    """C = A_dense (kd, M.nrows) @ M in long double; n = entries per column."""
    w = wide(np.result_type(M.values.dtype, A.dtype))
    D = _dense_wide(M, 0, M.ncols, w)
    Aw = A.astype(w)
    S = np.abs(Aw).astype(np.longdouble) @ np.abs(D).astype(np.longdouble)
    n = np.bincount(M.indices, minlength=M.ncols).astype(INT)
    return DenseRef(Aw @ D, S, n[None, :])


def ref_csc(M, X, rlo, rhi):
    """Partial result over rows [rlo, rhi) of the CSC matrix whose COLUMNS
    are M's rows (M.indices are global row ids): out[r - rlo] = sum v X[c].
    X is 1-D (SpMV) or (columns, k) (SpMM)."""
    w = wide(np.result_type(M.values.dtype, X.dtype))
    D = _dense_wide(M, rlo, rhi - rlo, w).T        # (rows, columns)
    Xw = X.astype(w)
    S = np.abs(D).astype(np.longdouble) @ np.abs(Xw).astype(np.longdouble)
    n = np.bincount(M.indices - rlo, minlength=rhi - rlo).astype(INT)
    return DenseRef(D @ Xw, S, n if X.ndim == 1 else n[:, None])


# -- plain model of spmv_kernel's block ownership -------------------------------
class SpmvBlock(NamedTuple):
    s: int
    e: int
    ro0: int       # first owned row: lower bound of s in indptr[0..m)
    ro1: int       # one past the last owned row
    carry: tuple   # (row, s, cend) when entries [s, cend) continue row ro0-1


def spmv_block_model(indptr, nnz=None):
    """What each 2048-nnz block of spmv_kernel owns."""
    ip = np.asarray(indptr, dtype=INT)
    m = len(ip) - 1
    nnz = int(ip[-1]) if nnz is None else nnz
    out = []
    for b in range(-(-nnz // SPMV_NNZ_PER_BLOCK)):
        s = b * SPMV_NNZ_PER_BLOCK
        e = min(s + SPMV_NNZ_PER_BLOCK, nnz)
        ro0 = int(np.searchsorted(ip[:m], s, side="left"))
        ro1 = m if e == nnz else int(np.searchsorted(ip[:m], e, side="left"))
        carry = None
        if ro0 > 0:
            cend = min(int(ip[ro0]), e) if ro0 < m else e
            if cend > s:
                carry = (ro0 - 1, s, cend)
        out.append(SpmvBlock(s, e, ro0, ro1, carry))
    return out


def xcd_swizzle(bid, nwg):
    """common.h's block remap, in Python."""
    q, rr = divmod(nwg, NXCD)
    xcd, idx = bid % NXCD, bid // NXCD
    return (xcd * (q + 1) if xcd < rr else rr * (q + 1) + (xcd - rr) * q) + idx


# -- SpMV boundary matrices -----------------------------------------------------
_SHORT = (1, 2, 3)
_LEAD = _GAP = _TRAIL = 3


def spmv_row_lengths(nnz):
    """Row lengths of the boundary matrix, cut off at nnz entries (with B =
    2048):
      3 empty rows | 600 rows of 1..3 entries (to 1200) | 848 (ends AT B)
      | 3 empty rows whose indptr is B | 1000 (starts AT B) | 2048 (crosses
      2B, to 5096) | 5144 (to 5B exactly: blocks 2, 3, 4, a carry in 3 and
      in 4) | 700 rows of 1..3 entries from 5B on | rows of 97 entries and
      empty ones up to 13B exactly | 3 empty rows whose indptr is 13B
      | 1 (starts AT 13B) | 3 empty rows."""
    B = SPMV_NNZ_PER_BLOCK
    master = [0] * _LEAD
    master += [_SHORT[i % 3] for i in range(600)]
    master += [B - 1200]
    master += [0] * _GAP
    master += [1000, 2048, 5 * B - 5096]
    master += [_SHORT[i % 3] for i in range(700)]
    pos = sum(master)
    i = 0
    while pos < 13 * B:
        ln = 0 if i % 5 == 4 else min(97, 13 * B - pos)
        master.append(ln)
        pos += ln
        i += 1
    master += [0] * _GAP + [1]
    lens, pos = [], 0
    for ln in master:
        ln = min(ln, nnz - pos)
        lens.append(ln)
        pos += ln
        if pos == nnz and ln > 0:
            break
    assert pos == nnz
    return lens + [0] * _TRAIL


@functools.lru_cache(maxsize=None)
def spmv_boundary_csr(dt, nnz, variant="base", positive=False):
    """The boundary matrix with nnz entries.  variant: "base" (columns in
    [0, 6000)), "col_lo" (first column 1000) or "wide" (int64 only: columns
    offset by 2^33).  Returns (Csr, col_lo): x is the window of SPMV_WINDOW
    entries from col_lo on.  positive: all values positive (fused dot).
    Built once; do not modify."""
    dt = np.dtype(dt)
    lo = {"base": 0, "col_lo": COL_LO, "wide": WIDE_LO}[variant]
    rng = np.random.default_rng(4100 + dt.num + nnz)
    rows = []
    for ln in spmv_row_lengths(nnz):
        c = np.sort(rng.choice(SPMV_WINDOW, ln, replace=False)).astype(INT)
        v = rand_values(rng, ln, dt)
        rows.append((c + lo, np.abs(v).astype(dt) if positive else v))
    M = csr_from_rows(rows, lo + SPMV_WINDOW, dt)
    check_csr(M)
    assert M.nnz == nnz and (nnz == 0 or M.indices.min() >= lo)
    return M, lo


def spmv_vectors(dt, nnz, m, positive=False):
    """(x window, y0, p) for the boundary matrix of nnz entries, m rows."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(4200 + dt.num + nnz)
    out = [rand_values(rng, SPMV_WINDOW, dt), rand_values(rng, m, dt),
           rand_values(rng, m, dt)]
    return [np.abs(v).astype(dt) if positive else v for v in out]


def dot_shares(M, x, p, col_lo=0):
    """What each carry and each block partial of the fused dot contributes:
    a list of (kind, block, amount) over the non-empty ones, and the dot's
    total (without d0).  Long double, all operands positive."""
    w = np.longdouble
    prod = M.values.astype(w) * x.astype(w)[M.indices - col_lo]
    pw = p.astype(w)
    ip = M.indptr
    shares = []
    for b, blk in enumerate(spmv_block_model(ip)):
        if blk.carry is not None:
            r, s, cend = blk.carry
            shares.append(("carry", b, pw[r] * prod[s:cend].sum()))
        part = w(0)
        for r in range(blk.ro0, blk.ro1):
            part += pw[r] * prod[ip[r]: min(int(ip[r + 1]), blk.e)].sum()
        if blk.ro1 > blk.ro0 and part > 0:
            shares.append(("partial", b, part))
    rows = np.repeat(np.arange(M.nrows), np.diff(ip))
    return shares, np.sum(pw[rows] * prod)


# -- SpMM operands --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spmm_csr(dt, m, col_lo=0):
    """m rows over columns [col_lo, col_lo + 400): empty, single-entry,
    300-entry and short rows; the last row is a 300-entry one (m = 1: the
    only row).  Built once; do not modify."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(5100 + dt.num + m)
    rows = []
    for i in range(m):
        if i == m - 1 or i % 64 == 2:
            ln = 300
        elif i % 7 == 0:
            ln = 0
        elif i % 7 == 1:
            ln = 1
        else:
            ln = int(rng.integers(2, 10))
        c = np.sort(rng.choice(SPMM_WINDOW, ln, replace=False)).astype(INT)
        rows.append((c + col_lo, rand_values(rng, ln, dt)))
    M = csr_from_rows(rows, col_lo + SPMM_WINDOW, dt)
    check_csr(M)
    return M


def rand_dense(seed, shape, dt):
    rng = np.random.default_rng(seed)
    return rand_values(rng, int(np.prod(shape)), dt).reshape(shape)


def spmm_large(dt=np.float64):
    """One entry per row, 64 columns, 262145 rows: (Csr, B (64, 33))."""
    m, n, k = SPMM_LARGE_M, 64, 33
    rng = np.random.default_rng(5200)
    ip = np.arange(m + 1, dtype=INT)
    ix = rng.integers(0, n, m).astype(INT)
    return (Csr(ip, ix, rand_values(rng, m, dt), m, n),
            rand_dense(5201, (n, k), dt))


# -- BSR cases ------------------------------------------------------------------
def bsr_empty_block_row(m):
    """The block row left without a block (None: there is only one)."""
    return 1 if -(-m // BSR) > 1 else None


@functools.lru_cache(maxsize=None)
def bsr_case(dt, m, n=BSR_N, first_col=BSR_FIRST_COL):
    """m x n matrix, every position of columns [first_col, n) stored, so
    the blocks reach the last, partial block column and the window starts
    inside block column first_col // 16; block row 1 (where there is one)
    has no block; at m = 33 block row 2 is row 32 alone and keeps one block
    only (columns 32..47).  Built once; do not modify."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(6100 + dt.num + m)
    skip = bsr_empty_block_row(m)
    rows = []
    for i in range(m):
        if i // BSR == skip:
            c = np.zeros(0, INT)
        elif i // BSR == 2:
            c = np.arange(2 * BSR, 3 * BSR, dtype=INT)
        else:
            c = np.arange(first_col, n, dtype=INT)
        rows.append((c, rand_values(rng, len(c), dt)))
    M = csr_from_rows(rows, n, dt)
    check_csr(M)
    return M


def bsr_blocks(M):
    """{(block row, block column): 16x16 array} of the stored entries."""
    out = {}
    rows = np.repeat(np.arange(M.nrows), np.diff(M.indptr))
    for r, c, v in zip(rows, M.indices, M.values):
        blk = out.setdefault((r // BSR, c // BSR),
                             np.zeros((BSR, BSR), dtype=M.values.dtype))
        blk[r % BSR, c % BSR] = v
    return out


def bsr_window(M):
    """(lo16, hi16) as csr_array._spmm aligns the gathered window."""
    lo, hi = int(M.indices.min()), int(M.indices.max()) + 1
    return lo // BSR * BSR, min(M.ncols, -(-hi // BSR) * BSR)


# -- rSpMM / CSC cases ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hot_csr(dt, side, lo=0):
    """side rows over ids [lo, lo + 300): every seventh row empty, and every
    other row holds the HOT id lo + 150 besides 0..5 more, so one output
    address takes an atomic from every non-empty row; ids lo + 290.. stay
    unused (empty outputs).  Read as CSR rows (rSpMM's B) or as the columns
    of a CSC matrix whose ids are global rows (lo = rlo).  Built once; do
    not modify."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(7100 + dt.num + side)
    hot = 150
    rows = []
    for i in range(side):
        if i % 7 == 3:
            c = np.zeros(0, INT)
        else:
            extra = rng.choice(290, int(rng.integers(0, 6)), replace=False)
            c = np.unique(np.concatenate([[hot], extra])).astype(INT)
        rows.append((c + lo, rand_values(rng, len(c), dt)))
    M = csr_from_rows(rows, lo + OTHER_SIDE, dt)
    check_csr(M)
    return M


def rspmm_case(dt, side):
    """B of C = A_dense @ B: side rows, 300 columns."""
    return hot_csr(dt, side)


def csc_case(dt, side, rlo=0):
    """side columns (as Csr rows) whose ids are the global rows
    [rlo, rlo + 300) of a CSC slab."""
    return hot_csr(dt, side, rlo)


def hot_count(M, lo=0):
    return int(np.sum(M.indices == lo + 150))


# -- non-canonical constructor inputs ---------------------------------------------
NONCANON_KINDS = ("banded", "blocks", "scattered")


@functools.lru_cache(maxsize=None)
def noncanonical(kind):
    """(data, indices, indptr, shape) in float64 with duplicates that add
    up, one cancelling pair per touched row (a stored zero afterwards, at a
    position of its own) and rows in descending column order.  banded: 5
    diagonals of a 300 x 300 matrix; blocks: dense 16 x 16 blocks of a
    64 x 64 matrix; scattered: random 120 x 90."""
    rng = np.random.default_rng(8100 + NONCANON_KINDS.index(kind))
    if kind == "banded":
        m = n = 300
        pat = [[j for j in range(i - 2, i + 3) if 0 <= j < n]
               for i in range(m)]
    elif kind == "blocks":
        m = n = 64
        on = {(0, 0), (0, 2), (1, 1), (2, 0), (2, 3), (3, 3)}
        pat = [[j for j in range(n) if (i // BSR, j // BSR) in on]
               for i in range(m)]
    else:
        m, n = 120, 90
        pat = [sorted(rng.choice(n, int(rng.integers(0, 9)),
                                 replace=False).tolist()) for i in range(m)]
    data, indices, indptr = [], [], [0]
    for i, cols in enumerate(pat):
        ent = []
        for j in cols:
            v = float(rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0]))
            if (i + j) % 3 == 0:       # stored twice, the parts add up
                part = float(rng.uniform(0.5, 2.0))
                ent += [(j, part), (j, v - part)]
            else:
                ent.append((j, v))
        if i % 4 == 1 and cols:        # +w, -w where nothing else is stored
            if kind == "blocks":       # inside a stored block: not possible,
                free = []              # the blocks are dense
            elif kind == "banded":
                free = [j for j in (i + 5, i - 5) if 0 <= j < n]
            else:
                free = [j for j in range(n) if j not in cols]
            if free:
                w = float(rng.uniform(0.5, 2.0))
                ent += [(free[0], w), (free[0], -w)]
        if kind == "blocks" and i % 4 == 1:   # cancel ON a stored entry:
            j = cols[0]                       # the sum stays, as a zero
            ent = [(c, v) for c, v in ent if c != j]
            w = float(rng.uniform(0.5, 2.0))
            ent += [(j, w), (j, -w)]
        ent.sort(key=lambda t: -t[0])         # descending: unsorted rows
        indices += [c for c, _ in ent]
        data += [v for _, v in ent]
        indptr.append(len(indices))
    out = (np.array(data, dtype=np.float64), np.array(indices, dtype=np.int64),
           np.array(indptr, dtype=np.int64))
    for a in out:       # shared by every caller: nobody may write to them
        a.flags.writeable = False
    return out + ((m, n),)


def _strictly_increasing(indptr, indices):
    for i in range(len(indptr) - 1):
        seg = indices[indptr[i]: indptr[i + 1]]
        if len(seg) > 1 and not np.all(np.diff(seg.astype(np.int64)) > 0):
            return False
    return True


def _close(got, ref, scale, nmax):
    """|got - ref| <= (nmax + 2) eps scale, float64; scale = sum |a| |b|."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref)
                  <= (nmax + 2) * real_eps(np.float64) * scale)


def check_noncanonical(kind, csr_array, csc_array):
    """Every API-level assertion on a non-canonical input, against scipy
    built from the same arrays; runs on whichever device the package uses.
    Returns the csr_arrays built (for the route assertions of the caller)."""
    import scipy.sparse as sps

    data, indices, indptr, shape = noncanonical(kind)
    m, n = shape
    raw = sps.csr_matrix((data, indices, indptr), shape=shape)
    assert not _strictly_increasing(indptr, indices)
    keep = [a.copy() for a in (raw.data, raw.indices, raw.indptr)]
    canon = raw.copy()
    canon.sum_duplicates()
    assert canon.nnz < raw.nnz and np.any(canon.data == 0)  # a kept zero
    rng = np.random.default_rng(8200)
    x = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    B = rng.uniform(0.5, 2.0, (n, 16)) * rng.choice([-1.0, 1.0], (n, 16))
    dense = raw.toarray()                      # scipy adds duplicates up
    absA = np.zeros(shape)                     # |parts| summed: the true S
    np.add.at(absA, (np.repeat(np.arange(m), np.diff(indptr)), indices),
              np.abs(data))
    nmax = int(np.diff(indptr).max())
    built = []
    for how in ("triple", "scipy"):
        A = (csr_array((data, indices, indptr), shape=shape)
             if how == "triple" else csr_array(raw))
        built.append(A)
        S = A.to_scipy_sparse_csr()
        assert A.nnz == canon.nnz == S.nnz
        assert _strictly_increasing(S.indptr, S.indices)
        assert np.array_equal(S.indptr, canon.indptr)
        assert np.array_equal(S.indices, canon.indices)
        assert np.array_equal(S.data == 0, canon.data == 0)
        _close(A @ x, raw @ x, absA @ np.abs(x), nmax)
        _close(A @ B, raw @ B, absA @ np.abs(B), nmax)
        _close(A.todense(), dense, absA, nmax)
        dg = np.asarray(A.diagonal())
        assert dg.shape == (min(m, n),)
        assert np.all(np.abs(dg - raw.diagonal())
                      <= (nmax + 2) * real_eps(np.float64)
                      * absA.diagonal())
        T = A.tocsc()
        tc = canon.tocsc()
        tc.sort_indices()
        assert T.nnz == tc.nnz
        assert np.array_equal(np.asarray(T._colptr.cpu()), tc.indptr)
        assert np.array_equal(np.asarray(T._indices.cpu()), tc.indices)
        _close(T.todense(), dense, absA, nmax)
        _close((A + A).todense(), (canon + canon).toarray(), 2 * absA, nmax)
        _close(A.multiply(A).todense(), canon.multiply(canon).toarray(),
               absA * absA, nmax)
    # the same two paths of csc_array, on the transposed arrays
    rawc = sps.csc_matrix((data, indices, indptr), shape=(n, m))
    keepc = [a.copy() for a in (rawc.data, rawc.indices, rawc.indptr)]
    xc = rng.uniform(0.5, 2.0, m)
    for how in ("triple", "scipy"):
        Ac = (csc_array((data, indices, indptr), shape=(n, m))
              if how == "triple" else csc_array(rawc))
        assert Ac.nnz == canon.nnz
        assert np.array_equal(np.asarray(Ac._colptr.cpu()), canon.indptr)
        assert np.array_equal(np.asarray(Ac._indices.cpu()), canon.indices)
        _close(Ac @ xc, rawc @ xc, absA.T @ xc, nmax)
        _close(Ac.todense(), dense.T, absA.T, nmax)
    # the caller's objects and arrays are bit-identical, order included
    for obj, kept in ((raw, keep), (rawc, keepc)):
        for a, b in zip((obj.data, obj.indices, obj.indptr), kept):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert not _strictly_increasing(indptr, indices)
    return built
