"""The streaming CG vector kernels (axpby, cg_xr_norm2) and their memory
modes: nt=0 plain accesses, 1 non-temporal loads of the read-only streams,
2 non-temporal loads and stores, -1 the kernel's own choice by vector length.

A mode changes how the bytes travel, never which bytes: every output vector
and the returned sum must be bit-equal to the nt=0 run, and close to an fp64
evaluation at the tolerance of the older axpby tests.  (Complex axpby keeps
the plain accesses whatever the mode, for that reason: the compiler fuses a
complex multiply-add differently behind a non-temporal load.)  Every vector is a
16-byte-aligned slice of a buffer filled with a sentinel that must survive
on both sides.  Sizes are taken around E = EPT * 256 elements, what one block
covers (EPT = 16 bytes / element size): tail only, one block full and not,
several blocks, and an odd size of about ten blocks.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_MODES = [0, 1, 2, -1]
_PAD = 8  # elements on each side; 8 * itemsize is a multiple of 16 bytes
_SENTINEL = -777.25
_DTYPES = {"fp64": np.float64, "fp32": np.float32,
           "c64": np.complex64, "c128": np.complex128}
_REAL = ["fp64", "fp32"]
# as in the older axpby tests: a few roundings of a positive result
_VEC_RTOL = {"fp64": 1e-12, "fp32": 1e-5, "c64": 1e-5, "c128": 1e-12}
# a sum of n positive terms errs by about log2(n) * eps relative
_DOT_RTOL = {"fp64": 1e-12, "fp32": 1e-5}
_FORMS = [(True, False), (True, True), (False, False), (False, True)]
# the automatic mode turns non-temporal at 256 MiB per vector
_AUTO_MIN_BYTES = 256 << 20


def _ept(name):
    return max(1, 16 // np.dtype(_DTYPES[name]).itemsize)


def _sizes(name):
    ept = _ept(name)
    E = ept * 256
    ns = {1, 2, 3, ept - 1, ept + 1, E - 1, E, E + 1, 2 * E - 1, 2 * E,
          2 * E + 1, 2 * E + E + 1, 3 * E + 7, 10 * E + 3}
    return sorted(n for n in ns if n >= 1)


_CASES = [(name, n) for name in _DTYPES for n in _sizes(name)]
_REAL_CASES = [(name, n) for name in _REAL for n in _sizes(name)]


@pytest.fixture(autouse=True, scope="module")
def _require_ext():
    if torch.cuda.is_available():
        from sparse.kernels import require

        require()


_INPUTS = {}


def _inputs(name, n, k):
    """k seeded host vectors with parts in [0.25, 1.25); made once."""
    key = (name, n, k)
    if key not in _INPUTS:
        dt = _DTYPES[name]
        rng = np.random.default_rng(7000 + n)
        vs = []
        for _ in range(k):
            v = 0.25 + rng.random(n)
            if np.dtype(dt).kind == "c":
                v = v + 1j * (0.25 + rng.random(n))
            v = v.astype(dt)
            v.setflags(write=False)
            vs.append(v)
        _INPUTS[key] = vs
    return _INPUTS[key]


class _Guarded:
    """A device vector inside a sentinel-filled buffer."""

    def __init__(self, host):
        t = torch.as_tensor(np.array(host), device="cuda")
        self.buf = torch.full((t.numel() + 2 * _PAD,), _SENTINEL,
                              dtype=t.dtype, device="cuda")
        self.v = self.buf[_PAD:_PAD + t.numel()]
        self.v.copy_(t)
        assert self.v.data_ptr() % 16 == 0 and self.v.is_contiguous()

    def intact(self):
        n = self.v.numel()
        return bool((self.buf[:_PAD] == _SENTINEL).all()
                    and (self.buf[_PAD + n:] == _SENTINEL).all())


def _bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int64 if t.element_size() == 8
                               else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        _bits(a), _bits(b))


def _scalars(name):
    tdt = torch.as_tensor(np.zeros(1, dtype=_DTYPES[name])).dtype
    if tdt.is_complex:
        a, b = 3.0 + 1.0j, 7.0 - 2.0j
    else:
        a, b = 3.0, 7.0
    return (torch.tensor(a, device="cuda", dtype=tdt),
            torch.tensor(b, device="cuda", dtype=tdt), a / b)


def _wide(v):
    return v.astype(np.complex128 if v.dtype.kind == "c" else np.float64)


@pytest.mark.parametrize("isalpha,negate", _FORMS)
@pytest.mark.parametrize("name,n", _CASES)
def test_axpby_modes(name, n, isalpha, negate):
    from sparse import kernels as K

    y0, x0 = _inputs(name, n, 2)
    if negate:
        # |a/b| < 0.5, the scaled operand's parts are below 1.25: adding 2
        # to the other keeps the result well away from cancellation
        shift = (2 + 2j) if y0.dtype.kind == "c" else 2
        if isalpha:
            y0 = (y0 + shift).astype(y0.dtype)
        else:
            x0 = (x0 + shift).astype(x0.dtype)
    a, b, s = _scalars(name)
    if negate:
        s = -s
    want = (_wide(y0) + s * _wide(x0)) if isalpha else (
        _wide(x0) + s * _wide(y0))
    outs = {}
    for nt in _MODES:
        y, x = _Guarded(y0), _Guarded(x0)
        K.axpby(y.v, x.v, a, b, isalpha, negate, nt=nt)
        torch.cuda.synchronize()
        assert y.intact() and x.intact(), f"sentinel overwritten, nt={nt}"
        assert np.array_equal(x.v.cpu().numpy(), x0), f"x changed, nt={nt}"
        outs[nt] = y.v.clone()
    got = outs[0].cpu().numpy()
    err = np.abs(_wide(got) - want) / np.abs(want)
    print(name, n, isalpha, negate, "max rel err", err.max())
    assert err.max() <= _VEC_RTOL[name]
    for nt in _MODES[1:]:
        assert _same_bits(outs[nt], outs[0]), f"nt={nt} differs from nt=0"


def _slots(name, n):
    return (n // _ept(name) + 255) // 256 + 1


@pytest.mark.parametrize("name,n", _REAL_CASES)
def test_cg_xr_norm2_modes(name, n):
    """Through the wrapper, and through the op with a NaN-filled partial
    buffer: every slot is written, the slots past the data hold exact zeros,
    and slot k is the same in every mode."""
    from sparse import kernels as K

    x0, p0, r0, q0 = _inputs(name, n, 4)
    r0 = (r0 + 1).astype(r0.dtype)  # r - s q stays positive
    a, b, s = _scalars(name)
    want_x = _wide(x0) + s * _wide(p0)
    want_r = _wide(r0) - s * _wide(q0)
    want_rz = (want_r ** 2).sum()
    res = {}
    for nt in _MODES:
        x, p, r, q = (_Guarded(v) for v in (x0, p0, r0, q0))
        rz = K.cg_xr_norm2(x.v, p.v, r.v, q.v, a, b, nt=nt)
        x2, r2 = _Guarded(x0), _Guarded(r0)
        part = torch.full((_slots(name, n) + 3,), float("nan"),
                          dtype=x.v.dtype, device="cuda")
        K.ext().cg_xr_norm2(x2.v, p.v, r2.v, q.v, a, b, part, nt)
        torch.cuda.synchronize()
        for g in (x, p, r, q, x2, r2):
            assert g.intact(), f"sentinel overwritten, nt={nt}"
        assert np.array_equal(p.v.cpu().numpy(), p0)
        assert np.array_equal(q.v.cpu().numpy(), q0)
        assert _same_bits(x2.v, x.v) and _same_bits(r2.v, r.v)
        used = (n // _ept(name) + 255) // 256  # chunks that hold vectors
        ns = _slots(name, n)
        assert not torch.isnan(part[:ns]).any(), "a partial slot not written"
        assert torch.isnan(part[ns:]).all(), "wrote past the partial slots"
        # slot 0 also carries the scalar tail; the rest past the data is zero
        assert (part[max(used, 1):ns] == 0).all()
        assert rz.dim() == 0 and _same_bits(rz, part[:ns].sum())
        res[nt] = (x.v.clone(), r.v.clone(), rz.clone(), part[:ns].clone())
    gx, gr, grz, _ = res[0]
    ex = np.abs(gx.cpu().numpy() - want_x) / np.abs(want_x)
    er = np.abs(gr.cpu().numpy() - want_r) / np.abs(want_r)
    print(name, n, "max rel err x", ex.max(), "r", er.max(), "rz", float(grz),
          want_rz)
    assert ex.max() <= _VEC_RTOL[name] and er.max() <= _VEC_RTOL[name]
    assert np.isclose(float(grz), want_rz, rtol=_DOT_RTOL[name], atol=0.0)
    for nt in _MODES[1:]:
        for got, ref, what in zip(res[nt], res[0], ("x", "r", "rz", "partial")):
            assert _same_bits(got, ref), f"{what}: nt={nt} differs from nt=0"


@pytest.mark.parametrize("nt", _MODES)
def test_empty_vectors(nt):
    from sparse import kernels as K

    for name in _DTYPES:
        a, b, _ = _scalars(name)
        e = torch.empty(0, dtype=a.dtype, device="cuda")
        K.axpby(e, e, a, b, True, False, nt=nt)
        if name in _REAL:
            z = K.cg_xr_norm2(e, e, e, e, a, b, nt=nt)
            assert z.dim() == 0 and float(z) == 0.0 and z.dtype == a.dtype
    torch.cuda.synchronize()


def test_bad_mode_is_an_error():
    from sparse import kernels as K

    a, b, _ = _scalars("fp64")
    v = torch.ones(8, dtype=torch.float64, device="cuda")
    for nt in (-2, 3):
        with pytest.raises(RuntimeError, match="nt must be"):
            K.axpby(v, v.clone(), a, b, True, False, nt=nt)
        with pytest.raises(RuntimeError, match="nt must be"):
            K.cg_xr_norm2(v, v.clone(), v.clone(), v.clone(), a, b, nt=nt)


def test_auto_mode_past_the_threshold():
    """The one size at which nt=-1 leaves the plain path: a vector of just
    over 256 MiB.  Both ops, fp64, bit-equal to nt=0."""
    from sparse import kernels as K

    n = _AUTO_MIN_BYTES // 8 + 3  # odd: vector part and scalar tail
    g = torch.Generator(device="cuda").manual_seed(11)
    x0, p, r0, q = (0.25 + torch.rand(n, dtype=torch.float64, device="cuda",
                                      generator=g) for _ in range(4))
    r0 += 1
    a, b, _ = _scalars("fp64")
    outs = {}
    for nt in (0, -1):
        x, r, y = x0.clone(), r0.clone(), x0.clone()
        rz = K.cg_xr_norm2(x, p, r, q, a, b, nt=nt)
        K.axpby(y, p, a, b, False, False, nt=nt)
        outs[nt] = (x, r, rz, y)
    for got, ref, what in zip(outs[-1], outs[0], ("x", "r", "rz", "y")):
        assert _same_bits(got, ref), f"{what}: nt=-1 differs from nt=0"
    s = 3.0 / 7.0
    assert torch.allclose(outs[0][0], x0 + s * p, rtol=1e-12, atol=0.0)
    assert torch.allclose(outs[0][1], r0 - s * q, rtol=1e-12, atol=0.0)
    assert torch.allclose(outs[0][3], p + s * x0, rtol=1e-12, atol=0.0)


def _cg3(nt):
    """Three CG iterations in the benchmark's call order on a 39 x 39
    Poisson grid (n = 1521: two full blocks, a partial one, a tail)."""
    import sparse
    from sparse import gallery, kernels as K, linalg

    A = gallery.poisson2d(39)
    n = A.shape[0]
    b = sparse.darray.ones((n,), dtype=np.float64)
    xv = sparse.darray.zeros((n,), dtype=np.float64)
    r = b - linalg.aslinearoperator(A).matvec(xv)
    p = r.copy()
    q = sparse.darray.zeros((n,), dtype=np.float64)
    rz_buf = r.dot(r).clone()
    for _ in range(3):
        pq = A.spmv_dot(p, q)
        rz_new = K.cg_xr_norm2(xv.local, p.local, r.local, q.local, rz_buf,
                               pq, nt=nt)
        K.axpby(p.local, r.local, rz_new.to(torch.float64),
                rz_buf.to(torch.float64), False, False, nt=nt)
        rz_buf.copy_(rz_new)
    torch.cuda.synchronize()
    return xv.local, r.local, p.local, q.local, rz_buf


def test_cg_iterations_bitwise():
    ref = _cg3(0)
    assert torch.isfinite(ref[0]).all() and float(ref[4]) > 0
    for nt in _MODES[1:]:
        for got, want, what in zip(_cg3(nt), ref, "x r p q rz".split()):
            assert _same_bits(got, want), f"{what}: nt={nt} differs from nt=0"
