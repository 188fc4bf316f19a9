"""CPU checks of utils/dense_cases.py: the generated SpMV / SpMM / BSR /
rSpMM / CSC inputs hit the kernel edges test_dense_gpu.py relies on (by a
plain model of spmv_kernel's block ownership), the references agree with
scipy, a dropped carry or block partial of the fused dot is far above the dot
tolerance, and the API-level checks of non-canonical constructor input pass
on whichever device the package runs on.
"""
import numpy as np
import pytest
import scipy.sparse as sps

from utils.common import types
from utils import dense_cases as dc

B = dc.SPMV_NNZ_PER_BLOCK
_REAL = [np.float32, np.float64]


def _down(dt):
    """The widest dtype scipy multiplies in."""
    return (np.complex128 if np.issubdtype(np.dtype(dt), np.complexfloating)
            else np.float64)


def _scipy(M, col_lo=0, width=None):
    w = M.ncols - col_lo if width is None else width
    return sps.csr_matrix((M.values.astype(_down(M.values.dtype)),
                           M.indices - col_lo, M.indptr), shape=(M.nrows, w))


def _agrees(ref, got, dt):
    """Loose: scipy computes in (at most) double, in its own order."""
    tol = 4 * (np.max(ref.n) + 2) * dc.real_eps(_down(dt)) * ref.S
    assert np.all(np.abs(ref.values - got) <= tol)


# -- SpMV boundary matrices -------------------------------------------------------
def _blocks(nnz):
    M, _ = dc.spmv_boundary_csr(np.float64, nnz)
    return M, dc.spmv_block_model(M.indptr)


def test_spmv_row_lengths_layout():
    for nnz in dc.SPMV_NNZS + dc.SPMV_DOT_NNZS:
        lens = dc.spmv_row_lengths(nnz)
        assert sum(lens) == nnz
        assert lens[:3] == [0, 0, 0] and lens[-3:] == [0, 0, 0]
    lens = dc.spmv_row_lengths(26625)
    ip = np.concatenate([[0], np.cumsum(lens)])
    assert max(lens) >= 5000
    # runs of >= 3 empty rows whose indptr is a multiple of 2048
    for at in (B, 13 * B):
        assert np.sum(ip[:-1] == at) >= 4  # the empty rows + the row after
    assert lens[-4] == 1 and ip[-5] == 13 * B   # a row starting AT 13 B


def test_spmv_model_hits_every_edge():
    counts = []
    for nnz in dc.SPMV_NNZS:
        M, blocks = _blocks(nnz)
        counts.append(len(blocks))
        assert len(blocks) == -(-nnz // B)
        # every row is owned exactly once
        owned = np.concatenate([np.arange(b.ro0, b.ro1) for b in blocks])
        assert np.array_equal(owned, np.arange(M.nrows))
        if nnz >= 2047:   # the row loop strides: a block owns > 256 rows
            assert max(b.ro1 - b.ro0 for b in blocks) > dc.SPMV_BLK
            short = np.diff(M.indptr)[blocks[0].ro0: blocks[0].ro1]
            assert np.sum(short <= 3) >= 600
        if nnz % B == 0:  # last block full, trailing empty rows via ro1 = m
            last = blocks[-1]
            assert last.e - last.s == B and last.e == nnz
            assert last.ro1 == M.nrows
            assert np.all(M.indptr[-4:] == nnz)
    assert counts == [1, 1, 1, 2, 2, 13, 14]
    assert any(c % dc.NXCD for c in counts)
    M, blocks = _blocks(26625)
    ip = M.indptr
    # boundary B: a row ends AT it, empty rows sit on it, a row starts AT it
    assert blocks[1].carry is None and blocks[1].s == B
    r = blocks[1].ro0
    assert np.all(ip[r: r + 4] == B) and ip[r + 4] > B and ip[r - 1] < B
    # boundary 2 B is crossed once; the 5144-entry row spans blocks 2, 3, 4
    assert blocks[2].carry is not None
    long_row = int(np.argmax(np.diff(ip)))
    assert ip[long_row + 1] - ip[long_row] >= 5000
    carried = [b.carry for b in blocks if b.carry and b.carry[0] == long_row]
    assert len(carried) == 2
    assert [c[2] - c[1] for c in carried] == [B, B]      # whole blocks
    assert blocks[3].ro0 == blocks[3].ro1                # owns no row
    assert blocks[5].carry is None                       # it ends AT 5 B
    assert blocks[5].ro1 - blocks[5].ro0 > 2 * dc.SPMV_BLK
    # boundary 13 B: no carry, empty rows on it, one entry behind it
    assert blocks[13].carry is None and blocks[13].e - blocks[13].s == 1
    assert np.sum(ip[:-1] == 13 * B) >= 4
    # nnz = 1 and 2047: a single partly filled block
    assert _blocks(1)[1][0].e == 1 and _blocks(2047)[1][0].e == 2047


def test_xcd_swizzle_is_a_bijection():
    for nwg in (1, 2, 3, 5, 7, 8, 9, 13, 14, 16, 23):
        assert sorted(dc.xcd_swizzle(b, nwg) for b in range(nwg)) == \
            list(range(nwg))


@pytest.mark.parametrize("variant", ["base", "col_lo", "wide"])
def test_spmv_variants(variant):
    M, lo = dc.spmv_boundary_csr(np.float64, 4096, variant)
    assert lo == {"base": 0, "col_lo": 1000, "wide": 1 << 33}[variant]
    assert M.indices.min() >= lo and M.indices.max() < lo + dc.SPMV_WINDOW
    assert M.ncols == lo + dc.SPMV_WINDOW
    base, _ = dc.spmv_boundary_csr(np.float64, 4096)
    assert np.array_equal(M.indptr, base.indptr)
    if variant == "wide":
        assert M.indices.max() > np.iinfo(np.int32).max


@pytest.mark.parametrize("dt", types)
@pytest.mark.parametrize("nnz", [1, 2049, 26625])
def test_ref_spmv_against_scipy(nnz, dt):
    M, lo = dc.spmv_boundary_csr(dt, nnz, "col_lo")
    assert M.values.dtype == np.dtype(dt)
    assert np.all((np.abs(M.values) >= 0.49) & (np.abs(M.values) <= 2.01))
    x, _, _ = dc.spmv_vectors(dt, nnz, M.nrows)
    ref = dc.ref_spmv(M, x, lo)
    _agrees(ref, _scipy(M, lo) @ x.astype(_down(dt)), dt)
    assert np.all(ref.values[ref.n == 0] == 0)
    # sensitivity: one term of a row is >= 0.25; the tolerance is a tenth
    # of that on every row in double, on rows up to 300 entries in single
    # (it grows like n^2 eps; the long rows are seen in double)
    tol = dc.dense_tol(ref, dt)
    seen = ref.n > 0
    if dt in (np.float32, np.complex64):
        seen &= ref.n <= 300
    assert np.all(tol[seen] < 0.1 * 0.25)


@pytest.mark.parametrize("dt", _REAL)
@pytest.mark.parametrize("nnz", dc.SPMV_DOT_NNZS)
def test_dot_share_is_100x_the_tolerance(nnz, dt):
    """All operands positive: a dropped carry or block partial shifts the
    dot by its share of the sum, at least 100x the dot tolerance."""
    M, lo = dc.spmv_boundary_csr(dt, nnz, positive=True)
    x, _, p = dc.spmv_vectors(dt, nnz, M.nrows, positive=True)
    assert np.all(M.values > 0) and np.all(x > 0) and np.all(p > 0)
    ref = dc.ref_spmv(M, x, lo)
    shares, total = dc.dot_shares(M, x, p, lo)
    assert abs(total - np.sum(p.astype(np.longdouble) * ref.values)) \
        <= 1e-15 * total
    nblocks = -(-nnz // B)
    tol = dc.dot_tol(ref, p, 3.0, nblocks, dt)
    kinds = [k for k, _, _ in shares]
    assert kinds.count("partial") >= 2
    assert kinds.count("carry") == {4096: 0, 6144: 1, 10240: 3}[nnz]
    smallest = min(a for _, _, a in shares)
    print(f"smallest share / dot tolerance: {float(smallest / tol):.1f}")
    assert smallest >= 100 * tol


# -- SpMM operands ------------------------------------------------------------------
@pytest.mark.parametrize("m", dc.SPMM_MS)
def test_spmm_operands(m):
    for lo in (0, dc.COL_LO):
        M = dc.spmm_csr(np.float64, m, lo)
        lens = np.diff(M.indptr)
        assert M.nrows == m and lens[-1] == 300
        assert M.indices.min() >= lo and M.ncols == lo + dc.SPMM_WINDOW
        if m > 1:
            assert {0, 1, 300} <= set(lens.tolist())
    # the k lists straddle every lane tile of the two kernels
    assert max(dc.SPMM_SMALL_KS) == dc.SPMM_SMALLK_MAX < min(dc.SPMM_WIDE_KS)
    assert {1, 2, 16, 17, 32} <= set(dc.SPMM_SMALL_KS)
    assert any(k > dc.WAVE for k in dc.SPMM_WIDE_KS)       # second column tile
    # ragged last wave / block: m is no multiple of the rows per block
    for k in dc.SPMM_SMALL_KS:
        kp = 1 << (k - 1).bit_length()
        rows_per_block = dc.SPMM_WAVES_PER_BLOCK * (dc.WAVE // kp)
        assert any(mm % rows_per_block for mm in dc.SPMM_MS)


@pytest.mark.parametrize("dt", types)
def test_ref_spmm_against_scipy(dt):
    M = dc.spmm_csr(dt, 257, dc.COL_LO)
    Bd = dc.rand_dense(1, (dc.SPMM_WINDOW, 17), dt)
    ref = dc.ref_spmm(M, Bd, dc.COL_LO)
    _agrees(ref, _scipy(M, dc.COL_LO) @ Bd.astype(_down(dt)), dt)
    assert np.all(ref.values[np.diff(M.indptr) == 0] == 0)


def test_spmm_large_case():
    M, Bd = dc.spmm_large()
    assert M.nrows == 262145 and Bd.shape == (64, 33)
    assert (M.nrows + 3) // 4 > dc.SPMM_MAX_GRID_Y
    assert np.array_equal(np.diff(M.indptr), np.ones(M.nrows))
    assert M.nrows * 33 * 8 < 72e6   # C is about 70 MB


# -- BSR ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", _REAL)
@pytest.mark.parametrize("m", dc.BSR_MS)
def test_bsr_cases(m, dt):
    M = dc.bsr_case(dt, m)
    assert (M.nrows, M.ncols) == (m, 53) and M.indices.min() == 21
    lo16, hi16 = dc.bsr_window(M)
    assert (lo16, hi16) == (16, 53)          # block-aligned start, ragged end
    assert M.ncols % dc.BSR and M.indices.max() == 52   # last column block
    blocks = dc.bsr_blocks(M)
    nbrows = -(-m // dc.BSR)
    skip = dc.bsr_empty_block_row(m)
    assert skip == (1 if m > 16 else None)
    assert {br for br, _ in blocks} == set(range(nbrows)) - {skip}
    assert max(bc for _, bc in blocks) == 3  # reaches the partial block column
    fill = M.nnz / (256.0 * len(blocks))
    if m == 1:
        # one row fills at most 16 of a block's 256 positions: no mirror
        # is profitable, the API-level test asserts the other route
        assert fill < dc.BSR_MIN_FILL
    else:
        assert fill >= dc.BSR_FILL_ANY_K
    for blk in blocks.values():
        nz = blk[blk != 0]
        assert len(np.unique(nz)) == len(nz)       # all positions distinct
        assert not np.array_equal(blk, blk.T)      # not symmetric
    full = [b for b in blocks.values() if np.count_nonzero(b) == 256]
    assert full or m < 16
    # ragged extents: k tiles and rows
    assert {k % 16 for k in dc.BSR_KS} >= {0, 1, 15}
    assert {mm % 16 for mm in dc.BSR_MS} >= {0, 1, 15}


@pytest.mark.parametrize("dt", _REAL)
def test_ref_bsr_against_scipy(dt):
    M = dc.bsr_case(dt, 33)
    lo16, hi16 = dc.bsr_window(M)
    Bw = dc.rand_dense(2, (hi16 - lo16, 17), dt)
    ref = dc.ref_spmm(M, Bw, lo16)
    _agrees(ref, _scipy(M, lo16, hi16 - lo16) @ Bw.astype(np.float64), dt)


# -- rSpMM / CSC ----------------------------------------------------------------------
@pytest.mark.parametrize("side", dc.SPARSE_SIDES)
def test_hot_cases(side):
    for lo in dc.CSC_RLOS:
        M = dc.csc_case(np.float64, side, lo)
        lens = np.diff(M.indptr)
        assert M.nrows == side and np.sum(lens == 0) >= side // 7
        assert M.indices.min() >= lo and M.ncols == lo + dc.OTHER_SIDE
        assert dc.hot_count(M, lo) == np.sum(lens > 0)
        used = np.bincount(M.indices - lo, minlength=dc.OTHER_SIDE)
        assert np.sum(used == 0) >= 10          # outputs nothing lands on
    assert dc.hot_count(dc.rspmm_case(np.float64, 600)) >= dc.HOT_MIN
    # the lane-stride loops: one trip less, exact, one more, three trips
    assert {e // dc.WAVE for e in dc.EXTENTS} == {0, 1, 2}
    assert {63, 64, 65} <= set(dc.EXTENTS)


@pytest.mark.parametrize("dt", types)
def test_ref_rspmm_and_csc_against_scipy(dt):
    M = dc.rspmm_case(dt, 257)
    A = dc.rand_dense(3, (65, M.nrows), dt)
    ref = dc.ref_rspmm(A, M)
    got = (_scipy(M).T @ A.astype(_down(dt)).T).T
    _agrees(ref, got, dt)
    rlo = 1000
    M = dc.csc_case(dt, 257, rlo)
    csc = _scipy(M, rlo).T                       # (rows, columns)
    x = dc.rand_dense(4, (M.nrows,), dt)
    _agrees(dc.ref_csc(M, x, rlo, rlo + dc.OTHER_SIDE),
            csc @ x.astype(_down(dt)), dt)
    X = dc.rand_dense(5, (M.nrows, 65), dt)
    ref = dc.ref_csc(M, X, rlo, rlo + dc.OTHER_SIDE)
    _agrees(ref, csc @ X.astype(_down(dt)), dt)
    assert np.all(ref.values[ref.n[:, 0] == 0] == 0)


# -- non-canonical constructor input ------------------------------------------------
@pytest.mark.parametrize("kind", dc.NONCANON_KINDS)
def test_noncanonical_input(kind):
    """Duplicates add up (a cancelling pair stays as a stored zero), rows come
    out sorted, every product / conversion matches scipy on the same arrays,
    and the caller's objects are untouched."""
    from sparse import csc_array, csr_array

    dc.check_noncanonical(kind, csr_array, csc_array)


def test_row_order_check_in_slabs():
    """The host pass of canonical_scipy, cut into slabs of every small size,
    against a row-by-row check."""
    from sparse.base import _rows_strictly_increasing

    rng = np.random.default_rng(3)
    seen = set()
    for trial in range(60):
        lens = rng.integers(0, 5, 9)
        ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        ix = np.concatenate([np.sort(rng.choice(12, n, replace=False))
                             for n in lens] + [np.zeros(0, int)]).astype(np.int32)
        if trial % 3 and ix.size > 1:   # break one place: swap or duplicate
            p = int(rng.integers(1, ix.size))
            ix[p] = ix[p - 1] if trial % 2 else max(int(ix[p - 1]) - 1, 0)
        want = all(np.all(np.diff(ix[ip[i]: ip[i + 1]]) > 0)
                   for i in range(len(lens)))
        seen.add(want)
        for slab in (1, 2, 3, 7, 1 << 24):
            assert _rows_strictly_increasing(ix, ip, slab) == want
    assert seen == {True, False}


def test_canonical_input_is_not_copied():
    from sparse.base import canonical_scipy

    s = sps.random(30, 20, 0.3, random_state=1, format="csr")
    s.sort_indices()
    assert canonical_scipy(s) is s
    z = sps.csr_matrix((4, 4))
    assert canonical_scipy(z) is z
    # explicit zeros are part of the pattern
    e = sps.csr_matrix((np.array([0.0, 1.0]), np.array([0, 2]),
                        np.array([0, 2, 2])), shape=(2, 3))
    assert canonical_scipy(e) is e and e.nnz == 2
    d = sps.csr_matrix((np.array([1.0, -1.0, 2.0]), np.array([2, 2, 0]),
                        np.array([0, 3, 3])), shape=(2, 3))
    c = canonical_scipy(d)
    assert c is not d and d.indices.tolist() == [2, 2, 0]
    assert c.indices.tolist() == [0, 2] and c.data.tolist() == [2.0, 0.0]
