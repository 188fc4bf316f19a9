"""Constant-plane DIA mirrors: exact classification at mirror build, and
bit-equality of every DIA op on the compressed mirror (W constants + one
mask word per row) against the forced-plain mirror of the same matrix.
"""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

pytestmark = pytest.mark.gpu

_OMEGA = 0.7
_DIA_OPS = ["dia_spmv", "dia_spmv_dot", "dia_residual", "dia_jacobi",
            "dia_spmv_bpdot"]
_RANGED_OPS = _DIA_OPS[:4]
_MASK_DT = {"u8": torch.uint8, "u16": torch.uint16, "u32": torch.uint32}


@pytest.fixture(autouse=True, scope="module")
def _require_ext():
    if torch.cuda.is_available():
        from sparse.kernels import require

        require()


def _plain_mirror(A):
    from sparse import kernels

    dm = kernels.build_dia(A.local, 0, compress=False)
    assert dm is not None and not dm.compressed and dm.dvals is not None
    return dm


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _classify_np(s):
    """(offs, cbits, mask, compressible) of a scipy matrix, on bit patterns;
    mask has one integer per padded row."""
    coo = s.tocoo()
    m = s.shape[0]
    mp = (m + 1) // 2 * 2
    diag = coo.col.astype(np.int64) - coo.row.astype(np.int64)
    offs = np.unique(diag)
    vb = _bits(coo.data)
    cbits = np.zeros(len(offs), dtype=vb.dtype)
    mask = np.zeros(mp, dtype=np.uint32)
    ok = True
    for k, o in enumerate(offs):
        sel = (diag == o) & (vb != 0)
        pats = np.unique(vb[sel])
        ok = ok and len(pats) <= 1
        if len(pats):
            cbits[k] = pats[0]
        mask[coo.row[sel]] |= np.uint32(1 << k)
    return offs, cbits, mask, ok


def _check_classification(A, s, word):
    dm = A._dia()
    assert dm is not None and dm.compressed and dm.dvals is None
    assert dm.mask.dtype == _MASK_DT[word]
    offs, cbits, mask, ok = _classify_np(s)
    assert ok
    assert np.array_equal(dm.offs.cpu().numpy(), offs)
    assert dm.cvals.dtype == A._values.dtype
    assert np.array_equal(_bits(dm.cvals.cpu().numpy()), cbits)
    assert dm.mask.numel() == len(mask)
    assert np.array_equal(dm.mask.cpu().numpy().astype(np.uint32), mask)


def _const_diags(m, offs, consts, dt=np.float64):
    return sps.diags([np.full(m - abs(o), c) for o, c in zip(offs, consts)],
                     offs, shape=(m, m), format="csr").astype(dt)


# -- classification -----------------------------------------------------------
@pytest.mark.parametrize("make,word", [
    (lambda g: g.poisson2d(16, 32), "u8"),
    (lambda g: g.banded(1025, ndiags=9), "u16"),
    (lambda g: g.banded(1025, ndiags=21), "u32"),
    (lambda g: g.poisson2d(16, 32, dtype=np.float32), "u8"),
], ids=["poisson-u8", "banded9-u16", "banded21-u32", "poisson-fp32"])
def test_constant_diagonals_compress(make, word):
    from sparse import gallery

    A = make(gallery)
    _check_classification(A, A.to_scipy_sparse_csr(), word)


def _poisson_scipy():
    from sparse import gallery

    s = gallery.poisson2d(16, 32).to_scipy_sparse_csr().tocsr()
    s.sort_indices()
    return s


def _random_diagonals():
    rng = np.random.default_rng(11)
    offs = (-16, -1, 0, 1, 16)
    return sps.diags([0.5 + rng.random(512 - abs(o)) for o in offs], offs,
                     shape=(512, 512), format="csr")


def _one_ulp():
    s = _poisson_scipy()
    s.data[777] = np.nextafter(s.data[777], np.inf)
    return s


def _one_negative_zero():
    s = _const_diags(512, (-16, -1, 0, 1, 16), (-1.0, -1.0, 4.0, -1.0, -1.0))
    s.data[np.flatnonzero(s.data == -1.0)[40]] = -0.0
    return s


@pytest.mark.parametrize("make", [
    _random_diagonals, _one_ulp, _one_negative_zero,
    lambda: _poisson_scipy().astype(np.complex128),
], ids=["random", "one-ulp", "negative-zero", "complex128"])
def test_non_constant_stays_plain(make):
    from sparse import csr_array

    s = make()
    A = csr_array(s)
    dm = A._dia()
    assert dm is not None and not dm.compressed
    assert dm.dvals is not None and dm.mask is None and dm.cvals is None
    rng = np.random.default_rng(12)
    x = rng.random(s.shape[1]).astype(s.dtype)
    assert np.allclose(np.asarray(A @ x), s @ x, rtol=1e-12)


def test_stored_positive_zeros_compress():
    """Explicitly stored +0.0 entries are masked-out entries like the
    structural ones."""
    from sparse import csr_array

    s = _const_diags(513, (-19, -1, 0, 1, 19), (-1.0, -1.0, 4.0, -1.0, -1.0))
    z = np.flatnonzero(s.data == -1.0)[::7]
    s.data[z] = 0.0
    assert s.nnz == len(s.data)  # the zeros stay stored
    A = csr_array(s)
    assert A.nnz == s.nnz
    _check_classification(A, s, "u8")
    x = np.random.default_rng(13).random(513)
    assert np.allclose(np.asarray(A @ x), s @ x, rtol=1e-12)


def test_nan_constant_compares_by_bits():
    from sparse import csr_array

    s = _const_diags(512, (-1, 0, 1), (np.nan, 4.0, -1.0))
    A = csr_array(s)
    _check_classification(A, s, "u8")


def test_opt_outs(monkeypatch):
    from sparse import gallery, kernels

    A = gallery.poisson2d(16, 32)
    assert not kernels.build_dia(A.local, 0, compress=False).compressed
    monkeypatch.setenv("SPARSE_DIA_NOCOMPRESS", "1")
    assert not kernels.build_dia(A.local, 0).compressed
    monkeypatch.delenv("SPARSE_DIA_NOCOMPRESS")
    assert kernels.build_dia(A.local, 0).compressed


def test_assigning_data_rebuilds_plain():
    from sparse import gallery

    A = gallery.poisson2d(16, 32)
    assert A._dia().compressed
    s = A.to_scipy_sparse_csr().tocsr()
    d = np.array(A.data)
    d[np.flatnonzero(d == 4.0)[5]] = 4.5
    A.data = d
    s.data[:] = d
    dm = A._dia()
    assert dm is not None and not dm.compressed
    x = np.random.default_rng(14).random(512)
    assert np.allclose(np.asarray(A @ x), s @ x, rtol=1e-12)


# -- bit-equality: compressed vs forced-plain mirror ---------------------------
_CASES = {
    "poisson511": lambda g: g.poisson2d(7, 73),
    "poisson512": lambda g: g.poisson2d(16, 32),
    "poisson513": lambda g: g.poisson2d(19, 27),
    "poisson1025": lambda g: g.poisson2d(25, 41),
    "banded9": lambda g: g.banded(1025, ndiags=9),
    "banded21": lambda g: g.banded(1025, ndiags=21),
    "poisson513-fp32": lambda g: g.poisson2d(19, 27, dtype=np.float32),
}
_CACHE = {}


class _Case:
    """One constant-diagonal matrix, its compressed and forced-plain
    mirrors, seeded vectors and the scipy references of the five ops."""

    def __init__(self, name):
        from sparse import gallery

        self.A = A = _CASES[name](gallery)
        self.m = m = A.shape[0]
        s = A.to_scipy_sparse_csr()
        self.mirrors = {"const": A._dia(), "plain": _plain_mirror(A)}
        assert self.mirrors["const"].compressed
        self.lo, self.hi = A._col_window()
        self.w = self.hi - self.lo
        rng = np.random.default_rng(9000 + m)
        names = ("x", "p", "b", "dinv", "r", "pold")
        self.fp32 = A.dtype == np.float32
        if self.fp32:
            # small integers and beta = 1/2: every product and sum of the
            # SpMVs and dots is exact in fp32, so the fp32 tolerance only
            # has to cover the Jacobi update (omega, no cancellation)
            n = {k: rng.integers(0, 8, m).astype(np.float64) for k in names}
            xmax, bnum = 8.0, 1.0
        else:
            n = {k: rng.random(m) for k in names}
            xmax, bnum = 1.0, 0.7
        self.vrt, self.drt = (1e-4, 1e-4) if self.fp32 else (1e-12, 1e-10)
        # |A x| < 2 * max diagonal * max x: b above it keeps the residual and
        # the Jacobi update free of cancellation (relative tolerances)
        n["b"] = n["b"] + 2 * abs(s.diagonal()).max() * xmax
        tdt = torch.float32 if self.fp32 else torch.float64
        self.tdt = tdt
        self.t = {k: torch.as_tensor(v, device="cuda").to(tdt)
                  for k, v in n.items()}
        self.bn = torch.tensor(bnum, device="cuda", dtype=tdt)
        self.bd = torch.tensor(2.0, device="cuda", dtype=tdt)
        s = s.astype(np.float64)
        Ax = s @ n["x"]
        pn = n["r"] + bnum / 2.0 * n["pold"]
        self.ref = {
            "dia_spmv": ([Ax], None),
            "dia_spmv_dot": ([Ax], n["p"] @ Ax),
            "dia_residual": ([n["b"] - Ax], None),
            "dia_jacobi": ([n["x"] + _OMEGA * n["dinv"] * (n["b"] - Ax)],
                           None),
            "dia_spmv_bpdot": ([pn, s @ pn], pn @ (s @ pn)),
        }

    def pieces(self, name, cut, vecs=None):
        xw = (vecs or self.t)[name][self.lo:self.hi]
        if cut is None:
            return xw[:0], xw, xw[:0]
        c1, c2 = cut
        return xw[:c1].clone(), xw[c1:c2].clone(), xw[c2:].clone()

    def new_out(self, op):
        # NaN-filled: a row no thread wrote fails every comparison
        k = 2 if op == "dia_spmv_bpdot" else 1
        return [torch.full((self.m,), float("nan"), dtype=self.tdt,
                           device="cuda") for _ in range(k)]

    def run(self, which, op, cut=None, rows=(0, -1), out=None, vecs=None):
        """Run one kernel wrapper on mirror `which`; returns (output
        vectors, dot or None)."""
        from sparse import kernels as K

        out = self.new_out(op) if out is None else out
        t, mir, lo, w = vecs or self.t, self.mirrors[which], self.lo, self.w
        px = self.pieces("x", cut, vecs)
        dot = None
        if op == "dia_spmv":
            K.dia_spmv(mir, px, out[0], lo, w, *rows)
        elif op == "dia_spmv_dot":
            dot = K.dia_spmv_dot(mir, px, out[0], t["p"], lo, w, *rows)
        elif op == "dia_residual":
            K.dia_residual(mir, px, t["b"], out[0], lo, w, *rows)
        elif op == "dia_jacobi":
            K.dia_jacobi(mir, px, t["x"], t["b"], t["dinv"], _OMEGA, out[0],
                         lo, w, *rows)
        elif op == "dia_spmv_bpdot":
            assert rows == (0, -1)
            dot = K.dia_spmv_bpdot(mir, self.pieces("r", cut, vecs),
                                   self.pieces("pold", cut, vecs), out[0],
                                   out[1], self.bn, self.bd, lo, w)
        else:
            raise AssertionError(op)
        return out, dot


def _case(name):
    if name not in _CACHE:
        _CACHE[name] = _Case(name)
    return _CACHE[name]


def _pin_cuts(w):
    return [(0, w), (1, 2), (101, w - 137), (w // 2, w // 2)]


def _same_bits(a, b):
    it = torch.int64 if a.element_size() == 8 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def _assert_pair_equal(C, op, ctx, **kw):
    """Compressed and plain runs agree bit for bit; returns the compressed
    result."""
    got, gdot = C.run("const", op, **kw)
    want, wdot = C.run("plain", op, **kw)
    for g, w in zip(got, want):
        assert not torch.isnan(w).any(), ctx
        assert torch.equal(g, w), ctx
    if wdot is not None:
        assert gdot.dim() == 0 and _same_bits(gdot, wdot), ctx
    return got, gdot


@pytest.mark.parametrize("name", list(_CASES))
@pytest.mark.parametrize("op", _DIA_OPS)
def test_compressed_matches_plain_and_scipy(op, name):
    """Single-piece and three-piece windows: the compressed mirror gives
    the plain mirror's bits, the cuts give the single-piece bits, and all
    of it matches scipy."""
    C = _case(name)
    rvecs, rdot = C.ref[op]
    single, sdot = _assert_pair_equal(C, op, (op, name))
    for got, want in zip(single, rvecs):
        assert np.allclose(got.cpu().numpy(), want, rtol=C.vrt), (op, name)
    if rdot is not None:
        assert np.isclose(float(sdot.item()), float(rdot), rtol=C.drt)
    for cut in _pin_cuts(C.w):
        three, tdot = _assert_pair_equal(C, op, (op, name, cut), cut=cut)
        for got, want in zip(three, single):
            assert torch.equal(got, want), (op, name, cut)
        if rdot is not None:
            assert _same_bits(tdot, sdot), (op, name, cut)


@pytest.mark.parametrize("name", list(_CASES))
@pytest.mark.parametrize("op", _RANGED_OPS)
def test_compressed_row_ranges(op, name):
    """[a, b), [0, a), [b, -1) into one output: bit-equal to the plain
    mirror range by range and to the full-range call; split dots match the
    plain mirror's bit for bit."""
    C = _case(name)
    full, fdot = C.run("const", op)
    rvecs, rdot = C.ref[op]
    for a, b in [(2, 258), (0, 512)]:
        outs = {k: C.new_out(op) for k in ("const", "plain")}
        dots = {k: [C.run(k, op, rows=rows, out=outs[k])[1]
                    for rows in [(a, b), (0, a), (b, -1)]]
                for k in ("const", "plain")}
        assert torch.equal(outs["const"][0], outs["plain"][0]), (op, name, a)
        assert torch.equal(outs["const"][0], full[0]), (op, name, a, b)
        assert np.allclose(outs["const"][0].cpu().numpy(), rvecs[0],
                           rtol=C.vrt)
        if fdot is not None:
            for g, w in zip(dots["const"], dots["plain"]):
                assert g.dim() == 0 and _same_bits(g, w), (op, name, a, b)
            assert np.isclose(float(sum(dots["const"]).item()), float(rdot),
                              rtol=C.drt)


# -- non-finite propagation ----------------------------------------------------
@pytest.mark.parametrize("op", _DIA_OPS)
def test_nonfinite_x_through_masked_entries(op):
    """inf / nan in x reach rows through masked-out entries exactly as
    through the stored +0.0 of the plain planes (0 * inf = nan): x loads
    are not skipped.  The inf sits left of a grid row's first point, whose
    row reads it through a masked-out entry only; the nans sit at the two
    clamped window edges."""
    C = _case("poisson512")  # 16 x 32 grid
    first = 5 * 16  # first point of grid row 5
    vecs = {k: v.clone() for k, v in C.t.items()}
    for name in ("x", "r"):
        vecs[name][first - 1] = float("inf")
        vecs[name][0] = float("nan")
        vecs[name][C.m - 1] = float("nan")
    for cut in (None, (1, 2)):
        got, gdot = C.run("const", op, cut=cut, vecs=vecs)
        want, wdot = C.run("plain", op, cut=cut, vecs=vecs)
        for g, w in zip(got, want):
            assert torch.equal(g.view(torch.int64), w.view(torch.int64))
        assert torch.isnan(got[-1][first])
        assert torch.isfinite(got[-1][first + 2])
        if wdot is not None:
            assert _same_bits(gdot, wdot)


# -- end to end ----------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 7, 60])
def test_cg_iterates_bit_equal(iters):
    from sparse import gallery, linalg

    b = np.random.default_rng(16).random(32 * 32)
    A = gallery.poisson2d(32)
    assert A._dia().compressed
    P = gallery.poisson2d(32)
    P._dia_cache = _plain_mirror(P)
    xc, ic = linalg.cg(A, b, tol=1e-10, maxiter=iters, conv_test_iters=5)
    xp, ip = linalg.cg(P, b, tol=1e-10, maxiter=iters, conv_test_iters=5)
    assert not P._dia().compressed
    assert ic == ip
    assert np.array_equal(_bits(np.asarray(xc)), _bits(np.asarray(xp)))
