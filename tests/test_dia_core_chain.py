"""Constant-plane DIA core (several row pairs per thread, unclamped interior
blocks, loads issued up front) and the one-barrier block reduction.

Every output vector of the five DIA ops on the compressed mirror must be
bit-equal to the streamed-plane mirror of the same matrix; fused dots may
differ from the fp64 reference by reassociation only.  S is the number of
rows a block of dia_spmv / dia_residual / dia_jacobi owns.
"""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

pytestmark = pytest.mark.gpu

_R = 2  # row pairs per thread (kDiaPairs in spmv.hip)
S = 2 * 256 * _R
_OMEGA = 0.7
_OPS = ["dia_spmv", "dia_spmv_dot", "dia_residual", "dia_jacobi",
        "dia_spmv_bpdot"]
_RANGED = _OPS[:4]
_DTYPES = [np.float64, np.float32]
_PIN_OFFS = (-37, -2, 0, 1, 40)
# rtol of a fused dot against the fp64 reference: positive terms, so any
# summation tree of n terms errs by about log2(n) * eps relative (under
# 3e-15 / 2e-6 at these sizes); these are the pinned tests' tolerances
_DOT_RTOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}
_VEC_RTOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-4}

# name -> (offsets, m)
_MATRICES = {f"pin-{m}": (_PIN_OFFS, m)
             for m in (1, 2, 3, 63, 65, S - 1, S, S + 1, 3 * S + 1)}
# x of a block comes wholly from its neighbours' rows; block 2 is interior
_MATRICES["far"] = ((-(S + 3), 0, S + 3), 5 * S + 1)
# W = 1, 8 (compile-time W, u8 mask), 9 (u16), 32 (u32); both parities
_MATRICES["w1"] = ((0,), 3 * S + 1)
_MATRICES["w8"] = ((-40, -37, -2, -1, 0, 1, 2, 41), 3 * S + 1)
_MATRICES["w9"] = ((-40, -37, -2, -1, 0, 1, 2, 41, 44), 3 * S + 1)
_MATRICES["w32"] = (tuple(range(-17, 15)), 3 * S + 1)
_MASK = {"w1": torch.uint8, "w8": torch.uint8, "w9": torch.uint16,
         "w32": torch.uint32, "far": torch.uint8}
_CACHE = {}


@pytest.fixture(autouse=True, scope="module")
def _require_ext():
    if torch.cuda.is_available():
        from sparse.kernels import require

        require()


class _Case:
    """One constant-diagonal matrix, its compressed and streamed mirrors,
    positive seeded vectors and the fp64 references."""

    def __init__(self, name, dt):
        from sparse import csr_array, kernels

        offs, m = _MATRICES[name]
        offs = [o for o in offs if abs(o) < m]
        consts = [0.5 + 0.125 * k for k in range(len(offs))]
        s = sps.diags([np.full(m - abs(o), c) for o, c in zip(offs, consts)],
                      offs, shape=(m, m), format="csr").astype(dt)
        self.m, self.dt, self.W = m, np.dtype(dt), len(offs)
        self.A = A = csr_array(s)
        self.mirrors = {"const": kernels.build_dia(A.local, 0),
                        "plain": kernels.build_dia(A.local, 0,
                                                   compress=False)}
        assert self.mirrors["const"].compressed
        assert not self.mirrors["plain"].compressed
        if name in _MASK:
            assert self.mirrors["const"].mask.dtype == _MASK[name]
        self.lo, self.hi = A._col_window()
        self.w = self.hi - self.lo
        rng = np.random.default_rng(4000 + m + len(offs))
        n = {k: (0.25 + rng.random(m)).astype(dt)
             for k in ("x", "p", "b", "dinv", "r", "pold")}
        # b above |A x| keeps the residual and the Jacobi update free of
        # cancellation, so relative tolerances hold
        n["b"] = (n["b"] + 2 * sum(consts) * 1.25).astype(dt)
        self.t = {k: torch.as_tensor(v, device="cuda") for k, v in n.items()}
        self.tdt = self.t["x"].dtype
        self.bn = torch.tensor(0.7, device="cuda", dtype=self.tdt)
        self.bd = torch.tensor(2.0, device="cuda", dtype=self.tdt)
        beta = (np.asarray(0.7, dtype=dt) / np.asarray(2.0, dtype=dt))
        n = {k: v.astype(np.float64) for k, v in n.items()}
        self.s64 = s64 = s.astype(np.float64).tocsr()
        Ax = s64 @ n["x"]
        pn = n["r"] + float(beta) * n["pold"]
        self.n = n
        self.ref = {
            "dia_spmv": ([Ax], None),
            "dia_spmv_dot": ([Ax], n["p"] * Ax),
            "dia_residual": ([n["b"] - Ax], None),
            "dia_jacobi": ([n["x"] + _OMEGA * n["dinv"] * (n["b"] - Ax)],
                           None),
            "dia_spmv_bpdot": ([pn, s64 @ pn], pn * (s64 @ pn)),
        }

    def cuts(self):
        w = self.w
        allc = [(0, w), (1, 2), (101, w - 137), (w // 2, w // 2)]
        return [c for c in allc if 0 <= c[0] <= c[1] <= w]

    def pieces(self, name, cut):
        xw = self.t[name][self.lo:self.hi]
        if cut is None:
            return xw[:0], xw, xw[:0]
        c1, c2 = cut
        return xw[:c1].clone(), xw[c1:c2].clone(), xw[c2:].clone()

    def new_out(self, op):
        # NaN-filled: a row no thread wrote fails every comparison
        k = 2 if op == "dia_spmv_bpdot" else 1
        return [torch.full((self.m,), float("nan"), dtype=self.tdt,
                           device="cuda") for _ in range(k)]

    def run(self, which, op, cut=None, rows=(0, -1), out=None, p=None):
        from sparse import kernels as K

        out = self.new_out(op) if out is None else out
        t, mir, lo, w = self.t, self.mirrors[which], self.lo, self.w
        px = self.pieces("x", cut)
        dot = None
        if op == "dia_spmv":
            K.dia_spmv(mir, px, out[0], lo, w, *rows)
        elif op == "dia_spmv_dot":
            dot = K.dia_spmv_dot(mir, px, out[0],
                                 t["p"] if p is None else p, lo, w, *rows)
        elif op == "dia_residual":
            K.dia_residual(mir, px, t["b"], out[0], lo, w, *rows)
        elif op == "dia_jacobi":
            K.dia_jacobi(mir, px, t["x"], t["b"], t["dinv"], _OMEGA, out[0],
                         lo, w, *rows)
        elif op == "dia_spmv_bpdot":
            assert rows == (0, -1)
            dot = K.dia_spmv_bpdot(mir, self.pieces("r", cut),
                                   self.pieces("pold", cut), out[0], out[1],
                                   self.bn, self.bd, lo, w)
        else:
            raise AssertionError(op)
        return out, dot


def _case(name, dt):
    key = (name, np.dtype(dt))
    if key not in _CACHE:
        _CACHE[key] = _Case(name, dt)
    return _CACHE[key]


def _same_bits(a, b):
    it = torch.int64 if a.element_size() == 8 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def _close(got, want, rtol):
    return np.isclose(float(got), float(want), rtol=rtol, atol=0.0)


@pytest.mark.parametrize("dt", _DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", list(_MATRICES))
@pytest.mark.parametrize("op", _OPS)
def test_const_core_matches_streamed(op, name, dt):
    """Single-piece and three-piece windows: every output vector has the
    streamed mirror's bits (and scipy's values); the dot holds against the
    fp64 reference and repeats bit for bit."""
    C = _case(name, dt)
    rvecs, rterms = C.ref[op]
    for cut in [None] + C.cuts():
        ctx = (op, name, cut)
        got, gdot = C.run("const", op, cut=cut)
        want, _ = C.run("plain", op, cut=cut)
        for g, w_, r in zip(got, want, rvecs):
            assert not torch.isnan(w_).any(), ctx
            assert torch.equal(g, w_), ctx
            assert np.allclose(g.cpu().numpy(), r, rtol=_VEC_RTOL[C.dt],
                               atol=0.0), ctx
        if rterms is not None:
            assert gdot.dim() == 0
            print(ctx, float(gdot), float(rterms.sum()))
            assert _close(gdot, rterms.sum(), _DOT_RTOL[C.dt]), ctx
            _, again = C.run("const", op, cut=cut)
            assert _same_bits(gdot, again), ctx


def _ranges(m):
    if m >= 3 * S:
        return [(2, 2 + S), (S, 2 * S)]  # [0, 2) < one block; S and 2 S rows
    if m > 258:
        return [(2, 258)]
    if m > 34:
        return [(2, 34)]
    return []


@pytest.mark.parametrize("dt", _DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["pin-65", f"pin-{S + 1}",
                                  f"pin-{3 * S + 1}", "far", "w9"])
@pytest.mark.parametrize("op", _RANGED)
def test_const_core_row_ranges(op, name, dt):
    """[a, b), [0, a), [b, -1) into one output: the streamed mirror's bits
    and the full-range call's; the split dots sum to the full dot."""
    C = _case(name, dt)
    full, fdot = C.run("const", op)
    rterms = C.ref[op][1]
    cuts = [None] + [c for c in C.cuts() if c == (101, C.w - 137)]
    assert _ranges(C.m)
    for a, b in _ranges(C.m):
        for cut in cuts:
            ctx = (op, name, a, b, cut)
            outs = {k: C.new_out(op) for k in ("const", "plain")}
            dots = {k: [C.run(k, op, cut=cut, rows=rows, out=outs[k])[1]
                        for rows in [(a, b), (0, a), (b, -1)]]
                    for k in ("const", "plain")}
            assert not torch.isnan(outs["plain"][0]).any(), ctx
            assert torch.equal(outs["const"][0], outs["plain"][0]), ctx
            assert torch.equal(outs["const"][0], full[0]), ctx
            if fdot is not None:
                rt = _DOT_RTOL[C.dt]
                split = sum(float(d) for d in dots["const"])
                print(ctx, split, float(fdot), float(rterms.sum()))
                assert _close(split, fdot, rt), ctx
                assert _close(split, rterms.sum(), rt), ctx
                parts = [rterms[a:b].sum(), rterms[:a].sum(),
                         rterms[b:].sum()]
                for g, r in zip(dots["const"], parts):
                    assert g.dim() == 0 and _close(g, r, rt), ctx


@pytest.mark.parametrize("dt", _DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["pin-65", f"pin-{S + 1}",
                                  f"pin-{3 * S + 1}", "far"])
def test_spmv_dot_with_p_being_x(name, dt):
    """CG calls dia_spmv_dot with p the very x slab: same vector bits as
    with a distinct p tensor, and x . A x against the reference."""
    C = _case(name, dt)
    x = C.t["x"]
    assert C.lo == 0 and C.hi == C.m
    alias, adot = C.run("const", "dia_spmv_dot", p=x)
    dist, ddot = C.run("const", "dia_spmv_dot", p=x.clone())
    plain, _ = C.run("plain", "dia_spmv_dot", p=x)
    assert torch.equal(alias[0], plain[0]) and torch.equal(dist[0], plain[0])
    assert _same_bits(adot, ddot)
    want = (C.n["x"] * C.ref["dia_spmv"][0][0]).sum()
    assert _close(adot, want, _DOT_RTOL[C.dt])


# -- reductions of elemwise.hip ------------------------------------------------
_NS = [1, 2, 3, 511, 512, 513, 1025]


def _vecs(n, dt, k):
    rng = np.random.default_rng(5000 + n)
    return [(0.25 + rng.random(n)).astype(dt) for _ in range(k)]


@pytest.mark.parametrize("dt", _DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", _NS)
def test_cg_xr_norm2(n, dt):
    """s = 1/2 makes s * v exact, so a fused multiply-add and numpy's
    multiply-then-add round alike: the vectors are bit-equal."""
    from sparse import kernels as K

    x, p, r, q = _vecs(n, dt, 4)
    r = (r + 1).astype(dt)  # r - q / 2 stays positive
    tx, tp, tr, tq = (torch.as_tensor(v.copy(), device="cuda")
                      for v in (x, p, r, q))
    a = torch.tensor(1.0, device="cuda", dtype=tx.dtype)
    b = torch.tensor(2.0, device="cuda", dtype=tx.dtype)
    rz = K.cg_xr_norm2(tx, tp, tr, tq, a, b)
    s = np.asarray(1.0, dtype=dt) / np.asarray(2.0, dtype=dt)
    xn = x + s * p
    rn = r - s * q
    assert xn.dtype == np.dtype(dt)
    assert np.array_equal(tx.cpu().numpy(), xn)
    assert np.array_equal(tr.cpu().numpy(), rn)
    assert np.array_equal(tp.cpu().numpy(), p)
    assert np.array_equal(tq.cpu().numpy(), q)
    want = (rn.astype(np.float64) ** 2).sum()
    print(n, float(rz), want)
    assert rz.dim() == 0 and _close(rz, want, _DOT_RTOL[np.dtype(dt)])
    tr2 = torch.as_tensor(r.copy(), device="cuda")
    tx2 = torch.as_tensor(x.copy(), device="cuda")
    assert _same_bits(rz, K.cg_xr_norm2(tx2, tp, tr2, tq, a, b))


@pytest.mark.parametrize("dt", _DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("isalpha,negate", [(True, False), (True, True),
                                            (False, False), (False, True)])
@pytest.mark.parametrize("n", _NS)
def test_axpby_norm2(n, isalpha, negate, dt):
    from sparse import kernels as K

    y, x = _vecs(n, dt, 2)
    if negate:
        # the subtracted term is at most 1.25 / 2
        if isalpha:
            y = (y + 1).astype(dt)
        else:
            x = (x + 1).astype(dt)
    ty = torch.as_tensor(y.copy(), device="cuda")
    tx = torch.as_tensor(x, device="cuda")
    a = torch.tensor(1.0, device="cuda", dtype=ty.dtype)
    b = torch.tensor(2.0, device="cuda", dtype=ty.dtype)
    got = K.axpby_norm2(ty, tx, a, b, isalpha, negate)
    s = np.asarray(1.0, dtype=dt) / np.asarray(2.0, dtype=dt)
    if negate:
        s = -s
    yn = (y + s * x) if isalpha else (x + s * y)
    assert np.array_equal(ty.cpu().numpy(), yn)
    assert np.array_equal(tx.cpu().numpy(), x)
    want = (yn.astype(np.float64) ** 2).sum()
    print(n, float(got), want)
    assert got.dim() == 0 and _close(got, want, _DOT_RTOL[np.dtype(dt)])
    ty2 = torch.as_tensor(y.copy(), device="cuda")
    assert _same_bits(got, K.axpby_norm2(ty2, tx, a, b, isalpha, negate))
