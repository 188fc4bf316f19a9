"""Constant-plane DIA core: pairs of adjacent diagonals taken from the
neighbour's registers (lane exchange) and the row operand taken from the
offset-0 pair.

The oracle is the streamed-plane mirror of the same matrix, whose kernels
share no code with the interior path under test: every output vector must
have its bits and lie within 1e-12 (fp64) / 1e-4 (fp32) of scipy, every fused
dot within 1e-12 / 1e-5 of the fp64 reference and repeat bit for bit (the
tolerances of test_dia_core_chain.py: every sum here has terms of one sign,
so a summation tree of n terms errs by about log2(n) * eps relative).
Vectors are seeded random, so a value taken from the wrong lane cannot pass;
outputs start as NaN, so a row nobody wrote fails.
"""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

pytestmark = pytest.mark.gpu

# Rows per block: dia_spmv and dia_spmv_dot own 2 * 256 * kDiaPairs = 2048
# with up to 5 diagonals and 1024 with more, dia_residual and dia_jacobi 1024
# (kDiaSmoothPairs), dia_spmv_bpdot 512 (spmv.hip).  S is the largest; the smaller ones divide it, so every row
# named below through S is a block boundary of all five ops.
_R = 4
S = 2 * 256 * _R
M5 = 5 * S + 1  # blocks 1-3 of S rows are interior for short offsets
_OMEGA = 0.7
_OPS = ["dia_spmv", "dia_spmv_dot", "dia_residual", "dia_jacobi",
        "dia_spmv_bpdot"]
_RANGED = _OPS[:4]
_DTYPES = [np.float64, np.float32]
_IDS = ["fp64", "fp32"]
_DOT_RTOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}
_VEC_RTOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-4}

# name -> offsets; all at m = M5
_SETS = {
    "5pt": (-64, -1, 0, 1, 64),            # middle run, even far diagonals
    "5pt-odd": (-63, -1, 0, 1, 63),        # far diagonals odd, no partner
    "m1-0": (-1, 0),
    "0-p1": (0, 1),
    "p1": (1,),
    "m2-m1": (-2, -1),
    "m1-p1": (-1, 1),                      # no centre: nothing adjacent
    "tri": (-1, 0, 1),                     # whole band, W = 3
    "penta": (-2, -1, 0, 1, 2),            # whole band, W = 5
    "7pt": (-(S + 64), -64, -1, 0, 1, 64, S + 64),  # block 2 is interior
    "w8": (-40, -37, -2, -1, 0, 1, 2, 41),  # a run that is no plan
    "w9": (-40, -37, -2, -1, 0, 1, 2, 41, 44),  # run-time W, u16 mask
}
_ADJ = {"5pt": 0b0110, "5pt-odd": 0b0110, "m1-0": 1, "0-p1": 1, "p1": 0,
        "m2-m1": 1, "m1-p1": 0, "tri": 0b11, "penta": 0b1111,
        "7pt": 0b001100, "w8": 0b0111100, "w9": 0b00111100}
_CACHE = {}


@pytest.fixture(autouse=True, scope="module")
def _require_ext():
    if torch.cuda.is_available():
        from sparse.kernels import require

        require()


def _toeplitz(offs, m, dt):
    offs = [o for o in offs if abs(o) < m]
    consts = [0.5 + 0.125 * k for k in range(len(offs))]
    return sps.diags([np.full(m - abs(o), c) for o, c in zip(offs, consts)],
                     offs, shape=(m, m), format="csr").astype(dt)


def _poisson(nx, dt):
    t = sps.diags([-1.0, 4.0, -1.0], [-1, 0, 1], shape=(nx, nx))
    o = sps.diags([-1.0, -1.0], [-1, 1], shape=(nx, nx))
    return (sps.kron(sps.eye(nx), t) + sps.kron(o, sps.eye(nx))).tocsr() \
        .astype(dt)


class _Case:
    """One matrix (scipy CSR `s`), its compressed and streamed mirrors,
    seeded vectors and the fp64 references.  `sign` (+-1 per row) is chosen
    by the caller so that every row sum, update and dot has terms of one
    sign: all ones for positive matrices, a checkerboard for the Laplacian."""

    def __init__(self, s, dt, sign=None, A=None, seed=0):
        from sparse import csr_array, kernels

        m = s.shape[0]
        self.m, self.dt = m, np.dtype(dt)
        self.A = A = csr_array(s) if A is None else A
        self.mirrors = {"const": kernels.build_dia(A.local, 0),
                        "plain": kernels.build_dia(A.local, 0,
                                                   compress=False)}
        assert self.mirrors["const"].compressed
        assert not self.mirrors["plain"].compressed
        self.lo, self.hi = A._col_window()
        self.w = self.hi - self.lo
        sign = np.ones(m) if sign is None else sign
        rng = np.random.default_rng(7000 + m + seed)
        n = {k: (sign * (0.25 + rng.random(m))).astype(dt)
             for k in ("x", "p", "b", "dinv", "r", "pold")}
        # A x carries `sign`; b of the other sign and above |A x| keeps
        # b - A x free of cancellation, and dinv < 0 lets the Jacobi update
        # add to x
        amax = abs(s).sum(axis=1).max() * 1.25
        n["b"] = (-(np.abs(n["b"]) + 2 * amax) * sign).astype(dt)
        n["dinv"] = (-np.abs(n["dinv"])).astype(dt)
        self.t = {k: torch.as_tensor(v, device="cuda") for k, v in n.items()}
        self.tdt = self.t["x"].dtype
        self.bn = torch.tensor(0.7, device="cuda", dtype=self.tdt)
        self.bd = torch.tensor(2.0, device="cuda", dtype=self.tdt)
        beta = (np.asarray(0.7, dtype=dt) / np.asarray(2.0, dtype=dt))
        n = {k: v.astype(np.float64) for k, v in n.items()}
        s64 = s.astype(np.float64).tocsr()
        Ax = s64 @ n["x"]
        pn = n["r"] + float(beta) * n["pold"]
        self.n = n
        self.Ax = Ax
        self.ref = {
            "dia_spmv": ([Ax], None),
            "dia_spmv_dot": ([Ax], n["p"] * Ax),
            "dia_residual": ([n["b"] - Ax], None),
            "dia_jacobi": ([n["x"] + _OMEGA * n["dinv"] * (n["b"] - Ax)],
                           None),
            "dia_spmv_bpdot": ([pn, s64 @ pn], pn * (s64 @ pn)),
        }

    def pieces(self, name, cut, shift=0):
        """Window pieces of a vector: one piece (cut None) or three cloned
        ones; shift > 0 makes the own piece a view that many elements into
        a larger tensor."""
        xw = self.t[name][self.lo:self.hi]
        if cut is None:
            if shift:
                big = torch.empty(xw.numel() + shift, dtype=xw.dtype,
                                  device="cuda")
                big[shift:] = xw
                xw = big[shift:]
            return xw[:0], xw, xw[:0]
        c1, c2 = cut
        return xw[:c1].clone(), xw[c1:c2].clone(), xw[c2:].clone()

    def new_out(self, op):
        k = 2 if op == "dia_spmv_bpdot" else 1
        return [torch.full((self.m,), float("nan"), dtype=self.tdt,
                           device="cuda") for _ in range(k)]

    def run(self, which, op, cut=None, rows=(0, -1), out=None, p=None,
            xloc=None, shift=0, pshift=None):
        from sparse import kernels as K

        out = self.new_out(op) if out is None else out
        t, mir, lo, w = self.t, self.mirrors[which], self.lo, self.w
        px = self.pieces("x", cut, shift)
        dot = None
        if op == "dia_spmv":
            K.dia_spmv(mir, px, out[0], lo, w, *rows)
        elif op == "dia_spmv_dot":
            dot = K.dia_spmv_dot(mir, px, out[0],
                                 t["p"] if p is None else p, lo, w, *rows)
        elif op == "dia_residual":
            K.dia_residual(mir, px, t["b"], out[0], lo, w, *rows)
        elif op == "dia_jacobi":
            K.dia_jacobi(mir, px, t["x"] if xloc is None else xloc, t["b"],
                         t["dinv"], _OMEGA, out[0], lo, w, *rows)
        elif op == "dia_spmv_bpdot":
            assert rows == (0, -1)
            dot = K.dia_spmv_bpdot(mir, self.pieces("r", cut, shift),
                                   self.pieces("pold", cut, shift
                                               if pshift is None else pshift),
                                   out[0],
                                   out[1], self.bn, self.bd, lo, w)
        else:
            raise AssertionError(op)
        return out, dot


def _case(name, dt):
    key = (name, np.dtype(dt))
    if key not in _CACHE:
        if name == "poisson":
            from sparse import gallery

            nx = 128
            ij = np.add.outer(np.arange(nx), np.arange(nx)).ravel()
            _CACHE[key] = _Case(_poisson(nx, dt), dt,
                                sign=np.where(ij % 2 == 0, 1.0, -1.0),
                                A=gallery.poisson2d(nx, dtype=dt))
        else:
            _CACHE[key] = _Case(_toeplitz(_SETS[name], M5, dt), dt,
                                seed=len(_SETS[name]))
    return _CACHE[key]


def _same_bits(a, b):
    it = torch.int64 if a.element_size() == 8 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def _close(got, want, rtol):
    return np.isclose(float(got), float(want), rtol=rtol, atol=0.0)


def _check(C, op, ctx, **kw):
    """const against plain and scipy for one call shape; returns const's
    outputs and dot."""
    rvecs, rterms = C.ref[op]
    got, gdot = C.run("const", op, **kw)
    want, _ = C.run("plain", op, **kw)
    for g, w_, r in zip(got, want, rvecs):
        assert not torch.isnan(w_).any(), ctx
        bad = torch.nonzero(g != w_).flatten()[:8].tolist()
        assert torch.equal(g, w_), (ctx, "first differing rows", bad)
        assert np.allclose(g.cpu().numpy(), r, rtol=_VEC_RTOL[C.dt],
                           atol=0.0), ctx
    if rterms is not None:
        assert gdot.dim() == 0
        print(ctx, float(gdot), float(rterms.sum()))
        assert _close(gdot, rterms.sum(), _DOT_RTOL[C.dt]), ctx
        _, again = C.run("const", op, **kw)
        assert _same_bits(gdot, again), ctx
    return got, gdot


# one piece; three pieces with the own piece starting at an odd and at an
# even index (the parity of every pair flips between the two)
_CUTS = [None, (101, M5 - 137), (102, M5 - 136)]


@pytest.mark.parametrize("dt", _DTYPES, ids=_IDS)
@pytest.mark.parametrize("name", list(_SETS))
def test_adjacency_word(name, dt):
    C = _case(name, dt)
    assert C.mirrors["const"].adj == _ADJ[name]
    assert C.mirrors["plain"].adj == _ADJ[name]


# dia_spmv_bpdot reads its own rows of r and p through the column window, so
# the window has to cover them: it does not where column 0 or m - 1 is empty
_NO_BPDOT = {"p1", "m2-m1"}


@pytest.mark.parametrize("dt", _DTYPES, ids=_IDS)
@pytest.mark.parametrize("op,name", [(op, name) for name in _SETS
                                     for op in _OPS
                                     if not (op == "dia_spmv_bpdot"
                                             and name in _NO_BPDOT)])
def test_offset_sets(op, name, dt):
    C = _case(name, dt)
    assert op != "dia_spmv_bpdot" or (C.lo, C.hi) == (0, C.m)
    for cut in _CUTS:
        _check(C, op, (op, name, cut), cut=cut)


@pytest.mark.parametrize("dt", _DTYPES, ids=_IDS)
@pytest.mark.parametrize("name", ["5pt", "penta", "m1-0"])
@pytest.mark.parametrize("op", _OPS)
def test_shifted_slab(op, name, dt):
    """The own slab is a view one element, and 8 bytes, into its storage:
    the pair parity follows the address, not the index."""
    C = _case(name, dt)
    for shift in sorted({1, 8 // C.dt.itemsize}):
        _check(C, op, (op, name, "shift", shift), shift=shift)
    if op == "dia_spmv_bpdot":  # the two windows differ in parity
        _check(C, op, (op, name, "shift r only"), shift=1, pshift=0)


@pytest.mark.parametrize("dt", _DTYPES, ids=_IDS)
@pytest.mark.parametrize("op", _OPS)
def test_poisson2d(op, dt):
    """gallery.poisson2d(128): 8 S rows, blocks 1 to 6 interior, a mask bit
    missing at both ends of every grid line of 128 rows."""
    C = _case("poisson", dt)
    assert C.m == 8 * S and C.mirrors["const"].adj == 0b0110
    mask = C.mirrors["const"].mask
    assert int((mask[S:3 * S] != 0x1f).sum()) == 2 * (2 * S // 128)
    for cut in [None, (37, C.w - 37), (38, C.w - 38)]:
        _check(C, op, (op, "poisson", cut), cut=cut)


@pytest.mark.parametrize("dt", _DTYPES, ids=_IDS)
@pytest.mark.parametrize("name", ["5pt", "penta"])
@pytest.mark.parametrize("op", _RANGED)
def test_row_ranges(op, name, dt):
    """Row ranges whose first row is and is not a multiple of S, into one
    NaN-filled output: the streamed mirror's bits inside, NaN outside."""
    C = _case(name, dt)
    full, _ = C.run("const", op)
    for a, b in [(2, 2 + S), (S, 2 * S), (S + 2, 3 * S)]:
        for cut in _CUTS[:2]:
            ctx = (op, name, a, b, cut)
            got, gdot = C.run("const", op, cut=cut, rows=(a, b))
            want, _ = C.run("plain", op, cut=cut, rows=(a, b))
            assert not torch.isnan(want[0][a:b]).any(), ctx
            assert torch.equal(got[0][a:b], want[0][a:b]), ctx
            assert torch.equal(got[0][a:b], full[0][a:b]), ctx
            assert torch.isnan(got[0][:a]).all(), ctx
            assert torch.isnan(got[0][b:]).all(), ctx
            if gdot is not None:
                part = C.ref[op][1][a:b].sum()
                print(ctx, float(gdot), float(part))
                assert _close(gdot, part, _DOT_RTOL[C.dt]), ctx


@pytest.mark.parametrize("dt", _DTYPES, ids=_IDS)
@pytest.mark.parametrize("name", ["5pt", "penta", "poisson"])
@pytest.mark.parametrize("op", _OPS)
def test_wave_seams(op, name, dt):
    """The last and first lane of a wave take one element from the
    neighbouring wave's rows: rows 128 k - 1 and 128 k of interior block 2
    (one wave instruction covers 128 consecutive rows), and the block's
    first and last row."""
    C = _case(name, dt)
    seams = sorted({2 * S, 3 * S - 1} |
                   {2 * S + 128 * k + d for k in range(1, S // 128)
                    for d in (-1, 0)})
    idx = torch.as_tensor(seams, device="cuda")
    for cut in _CUTS[:2] if name != "poisson" else [None]:
        got, _ = C.run("const", op, cut=cut)
        want, _ = C.run("plain", op, cut=cut)
        for g, w_, r in zip(got, want, C.ref[op][0]):
            assert torch.equal(g[idx], w_[idx]), (op, name, cut)
            assert np.allclose(g[idx].cpu().numpy(), r[seams],
                               rtol=_VEC_RTOL[C.dt], atol=0.0)


@pytest.mark.parametrize("dt", _DTYPES, ids=_IDS)
@pytest.mark.parametrize("name", ["5pt", "penta", "m1-p1", "poisson"])
def test_operand_aliasing(name, dt):
    """p of dia_spmv_dot being the x slab itself (CG), a clone, and an equal
    view of a larger tensor; xloc of dia_jacobi being the own slab and a
    clone: one set of bits."""
    C = _case(name, dt)
    x = C.t["x"]
    assert C.lo == 0 and C.hi == C.m
    big = torch.cat([x[:3], x])
    plain, _ = C.run("plain", "dia_spmv_dot", p=x)
    dots = []
    for p in (x, x.clone(), big[3:]):
        got, dot = C.run("const", "dia_spmv_dot", p=p)
        assert torch.equal(got[0], plain[0])
        dots.append(dot)
    assert _same_bits(dots[0], dots[1]) and _same_bits(dots[0], dots[2])
    want = (C.n["x"] * C.Ax).sum()
    print(name, float(dots[0]), want)
    assert _close(dots[0], want, _DOT_RTOL[C.dt])
    jplain, _ = C.run("plain", "dia_jacobi", xloc=x)
    for xloc in (x, x.clone(), big[3:]):
        got, _ = C.run("const", "dia_jacobi", xloc=xloc)
        assert torch.equal(got[0], jplain[0])
    assert np.allclose(jplain[0].cpu().numpy(), C.ref["dia_jacobi"][0][0],
                       rtol=_VEC_RTOL[C.dt], atol=0.0)


@pytest.mark.parametrize("dt", _DTYPES, ids=_IDS)
@pytest.mark.parametrize("pos", ["first", "last", "r127", "r128"])
def test_one_cleared_mask_bit(pos, dt):
    """Pentadiagonal Toeplitz, every interior block with full mask words,
    then A[r, r + 1] set to a stored +0.0 at the first / last row of block 2
    and on either side of its first wave seam: the mirror still compresses
    (the entry clears one mask bit) and row r follows the streamed mirror."""
    r = {"first": 2 * S, "last": 3 * S - 1, "r127": 2 * S + 127,
         "r128": 2 * S + 128}[pos]
    key = ("cleared", pos, np.dtype(dt))
    if key not in _CACHE:
        s = _toeplitz(_SETS["penta"], M5, dt)
        nnz = s.nnz
        s[r, r + 1] = 0.0  # an existing entry: stays stored
        assert s.nnz == nnz and s[r, r + 1] == 0.0
        _CACHE[key] = _Case(s, dt, seed=r)
    C = _CACHE[key]
    mask = C.mirrors["const"].mask
    assert int(mask[r]) == 0b10111 and int(mask[r - 1]) == 0b11111
    assert int(mask[r + 1]) == 0b11111
    for op in _OPS:
        got, _ = _check(C, op, (op, pos))
        want, _ = C.run("plain", op)
        assert torch.equal(got[-1][r], want[-1][r])
    for op in _RANGED:  # first row no multiple of S
        a, b = 2 * S - 2, 3 * S + 2
        got, _ = C.run("const", op, rows=(a, b))
        want, _ = C.run("plain", op, rows=(a, b))
        assert torch.equal(got[0][a:b], want[0][a:b]), (op, pos)
