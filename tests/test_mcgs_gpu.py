"""Colouring rounds (color.hip) and multicolour sweeps (relax.hip) vs the
plain-Python / scipy oracles — all @gpu.

Same oracles and inputs as test_mcgs.py (utils/mcgs_cases.py); the tests here
also pin which kernel variant runs (lanes per row, index width, order width).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from utils.common import types
from utils.mcgs_cases import (check_coloring, check_sweeps, dense_block,
                              diagonal_only, lower_bidiagonal, py_greedy,
                              random_sym, raw_csr_array, red_black, rhs,
                              sgs_oracle, shuffled_with_duplicates,
                              sweep_oracle, to_csr_array)
from utils.trisolve_cases import tol

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                  "examples")


@pytest.fixture(autouse=True, scope="module")
def _require_ext():
    if torch.cuda.is_available():
        from sparse.kernels import require

        require()


def _device_csr(A, idx="int32"):
    """csr_array of scipy A on the GPU with int32 or int64 column indices."""
    Ad = to_csr_array(A, idx)
    assert Ad._values.is_cuda
    assert Ad._indices.dtype == (torch.int64 if idx == "int64"
                                 else torch.int32)
    return Ad


@pytest.fixture(scope="module")
def poisson32():
    from sparse import gallery

    A = gallery.poisson2d(32, 32)
    assert A._values.is_cuda
    return A


# -- colouring ------------------------------------------------------------------
@pytest.mark.parametrize("idx", ["int32", "int64"])
@pytest.mark.parametrize("case", [random_sym, dense_block, lower_bidiagonal,
                                  diagonal_only])
def test_greedy_coloring_gpu(case, idx):
    from sparse.gauss_seidel import _greedy_coloring
    from sparse.linalg import greedy_coloring

    A = case()
    Ad = _device_csr(A, idx)
    c = greedy_coloring(Ad)
    assert c.is_cuda and c.dtype == torch.int32
    got = c.cpu().numpy()
    assert np.array_equal(got, py_greedy(A))
    check_coloring(A, got)
    _, rounds = _greedy_coloring(Ad, 0)
    assert 1 <= rounds <= A.shape[0]


def test_coloring_poisson_window_and_seeds_gpu(poisson32):
    from sparse.linalg import greedy_coloring

    S = poisson32.to_scipy_sparse_csr()
    got = greedy_coloring(poisson32).cpu().numpy()
    assert np.array_equal(got, py_greedy(S)) and got.max() + 1 <= 5
    # 70 mutually adjacent rows: the 64-colour window moves
    blk = greedy_coloring(_device_csr(dense_block())).cpu().numpy()
    assert blk.max() + 1 >= 70
    assert sorted(blk[:70].tolist()) == list(range(70))
    # not structurally symmetric: i and i-1 still differ
    bi = greedy_coloring(_device_csr(lower_bidiagonal())).cpu().numpy()
    assert np.all(bi[1:] != bi[:-1])
    A = random_sym()
    Ad = _device_csr(A)
    a = greedy_coloring(Ad, seed=5).cpu().numpy()
    assert np.array_equal(a, greedy_coloring(Ad, seed=5).cpu().numpy())
    assert np.array_equal(a, py_greedy(A, 5))
    other = greedy_coloring(Ad, seed=6).cpu().numpy()
    assert not np.array_equal(a, other)
    assert np.array_equal(other, py_greedy(A, 6))
    check_coloring(A, other)


def test_unsorted_rows_with_duplicates_gpu():
    from sparse.linalg import MulticolorGaussSeidel, greedy_coloring

    A, Ad, summed = shuffled_with_duplicates()
    assert Ad._values.is_cuda
    got = greedy_coloring(Ad).cpu().numpy()
    assert np.array_equal(got, py_greedy(A))
    check_sweeps(MulticolorGaussSeidel(Ad), summed, np.float64)


# -- sweeps ---------------------------------------------------------------------
def _check_gpu(gs, A, dt, **kw):
    assert gs.colors.is_cuda and gs.order.is_cuda and gs.color_ptr.is_cuda
    assert gs.order.dtype == torch.int32
    check_sweeps(gs, A, dt, **kw)


@pytest.mark.parametrize("idx", ["int32", "int64"])
@pytest.mark.parametrize("dt", types)
def test_sweeps_match_scipy_gpu(dt, idx):
    from sparse.linalg import MulticolorGaussSeidel

    A = random_sym(dt)
    gs = MulticolorGaussSeidel(_device_csr(A, idx))
    assert np.array_equal(gs.colors.cpu().numpy(), py_greedy(A))
    # about 7 entries a row: 8 lanes per row in the populous colours
    assert 8 in gs._sched[:, 3].tolist()
    _check_gpu(gs, A, dt)


def test_poisson_greedy_and_red_black_gpu(poisson32):
    from sparse.linalg import MulticolorGaussSeidel

    S = poisson32.to_scipy_sparse_csr()
    gs = MulticolorGaussSeidel(poisson32)
    assert np.array_equal(gs.colors.cpu().numpy(), py_greedy(S))
    _check_gpu(gs, S, np.float64)
    rb = MulticolorGaussSeidel(poisson32, colors=red_black(32, 32))
    assert rb.ncolors == 2 and rb.color_ptr.tolist() == [0, 512, 1024]
    assert rb._sched[:, 3].tolist() == [8, 8]  # 4.9 entries a row
    _check_gpu(rb, S, np.float64)


def test_unused_colour_is_an_empty_segment_gpu():
    """A caller's colouring that leaves colour 1 unused: the schedule has an
    empty segment, skipped (no launch) forwards and in reverse."""
    from sparse import gallery
    from sparse.linalg import MulticolorGaussSeidel

    A = gallery.poisson2d(8, 8)
    assert A._values.is_cuda
    gs = MulticolorGaussSeidel(A, colors=2 * red_black(8, 8))
    assert gs.ncolors == 3
    assert gs.color_ptr.tolist() == [0, 32, 32, 64]
    _check_gpu(gs, A.to_scipy_sparse_csr(), np.float64)


@pytest.mark.parametrize("dt", types)
def test_long_rows_gpu(dt):
    """Rows of 70 entries, one per colour: 64 lanes per row."""
    from sparse.linalg import MulticolorGaussSeidel

    A = dense_block(dt)
    gs = MulticolorGaussSeidel(_device_csr(A))
    assert gs.ncolors >= 70 and 64 in gs._sched[:, 3].tolist()
    _check_gpu(gs, A, dt, shapes=[(200,), (200, 3)])


def test_short_rows_gpu():
    """Two entries a row: one lane per row."""
    from sparse.linalg import MulticolorGaussSeidel

    A = lower_bidiagonal()
    gs = MulticolorGaussSeidel(_device_csr(A))
    assert set(gs._sched[:, 3].tolist()) == {1}
    _check_gpu(gs, A, np.float64)


def test_diagonal_only_and_tiny_gpu():
    from sparse import asdistarray, csr_array
    from sparse.linalg import MulticolorGaussSeidel, greedy_coloring

    A = diagonal_only()
    gs = MulticolorGaussSeidel(_device_csr(A))
    assert gs.ncolors == 1 and gs.color_ptr.tolist() == [0, 100]
    b = rhs((100,), np.float64)
    x = gs.sweep(asdistarray(rhs((100,), np.float64, seed=6)), b)
    assert x.local.is_cuda
    assert np.array_equal(np.asarray(x), b / A.diagonal())
    A0 = csr_array((0, 0))
    assert greedy_coloring(A0).shape == (0,)
    g0 = MulticolorGaussSeidel(A0)
    assert g0.ncolors == 0
    assert np.asarray(g0.sweep(asdistarray(np.zeros(0)), np.zeros(0))).shape \
        == (0,)
    one = csr_array(sps.csr_matrix(np.array([[4.0]])))
    assert greedy_coloring(one).tolist() == [0]
    x = MulticolorGaussSeidel(one).sweep(asdistarray(np.array([9.0])),
                                         np.array([2.0]), "symmetric")
    assert np.allclose(np.asarray(x), [0.5])


def test_errors_gpu(poisson32):
    from sparse import asdistarray, csr_array
    from sparse.linalg import MulticolorGaussSeidel, sgs_preconditioner

    with pytest.raises(ValueError):
        MulticolorGaussSeidel(csr_array(sps.random(
            4, 5, 0.5, random_state=0, format="csr")))
    missing = sps.csr_matrix(np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 1, 3]]))
    with pytest.raises(np.linalg.LinAlgError):
        MulticolorGaussSeidel(csr_array(missing))
    zero = raw_csr_array([1.0, 2.0, 0.0, 3.0], [0, 0, 1, 2], [0, 1, 3, 4], 3)
    with pytest.raises(np.linalg.LinAlgError):
        MulticolorGaussSeidel(zero)
    improper = red_black(32, 32)
    improper[1] = improper[0]
    with pytest.raises(ValueError, match="improper"):
        MulticolorGaussSeidel(poisson32, colors=improper)
    with pytest.raises(ValueError, match="ordering"):
        sgs_preconditioner(poisson32, ordering="colour")
    gs = MulticolorGaussSeidel(poisson32)
    with pytest.raises(ValueError, match="direction"):
        gs.sweep(asdistarray(np.zeros(1024)), np.ones(1024), direction="up")


# -- the preconditioner -----------------------------------------------------------
def test_matvec_is_permuted_sgs_gpu(poisson32):
    from sparse import darray
    from sparse.linalg import MulticolorGaussSeidel, sgs_preconditioner
    from sparse.trisolve import _SGSOperator

    assert type(sgs_preconditioner(poisson32)) is _SGSOperator
    M = sgs_preconditioner(poisson32, ordering="multicolor")
    assert isinstance(M, MulticolorGaussSeidel)
    S = poisson32.to_scipy_sparse_csr()
    order = M.order.cpu().numpy()
    for shape in [(1024,), (1024, 3)]:
        r = rhs(shape, np.float64)
        ref = sgs_oracle(S, order, r)
        z = M.matvec(r)
        assert z.local.is_cuda
        assert np.allclose(np.asarray(z), ref, **tol(np.float64))
        assert np.allclose(np.asarray(M.rmatvec(r)), ref, **tol(np.float64))
        out = darray.ones(shape)
        assert M.matvec(r, out=out) is out
        assert np.allclose(np.asarray(out), ref, **tol(np.float64))
    rd = darray.asdistarray(rhs((1024,), np.float64))  # out may alias r
    assert M.matvec(rd, out=rd) is rd
    assert np.allclose(np.asarray(rd),
                       sgs_oracle(S, order, rhs((1024,), np.float64)),
                       **tol(np.float64))


def test_multicolor_sgs_preconditioned_cg_gpu():
    """Same conditions as the host test: converged to the tolerance in
    strictly fewer iterations than plain CG on poisson2d(64, 64)."""
    from sparse import gallery
    from sparse.linalg import cg, sgs_preconditioner

    A = gallery.poisson2d(64, 64)
    assert A._values.is_cuda
    S = A.to_scipy_sparse_csr()
    b = np.ones(4096)

    def iterations(M):
        count = [0]

        def cb(_x):
            count[0] += 1

        x, info = cg(A, b, tol=1e-6, conv_test_iters=1, M=M, callback=cb)
        assert info == 0
        r = b - S @ np.asarray(x)
        assert np.linalg.norm(r) <= 1.001e-6 * np.linalg.norm(b)
        return count[0]

    plain = iterations(None)
    mc = iterations(sgs_preconditioner(A, ordering="multicolor"))
    print(f"CG iterations on the GPU: plain {plain}, multicolour SGS {mc}")
    assert mc < plain


# -- streams and graphs -----------------------------------------------------------
def test_sweep_captured_in_a_graph_gpu():
    """One symmetric sweep captured after two warm-up sweeps on a side stream
    and replayed on two right-hand sides equals the eager sweep bit for bit:
    the same kernels in the same order."""
    from sparse import asdistarray, darray
    from sparse.linalg import MulticolorGaussSeidel

    A = random_sym()
    n = A.shape[0]
    gs = MulticolorGaussSeidel(_device_csr(A))
    bbuf = asdistarray(rhs((n,), np.float64))
    x = darray.zeros((n,))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            x.local.zero_()
            gs.sweep(x, bbuf, "symmetric")
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x.local.zero_()
        gs.sweep(x, bbuf, "symmetric")
    for seed in (7, 8):
        b = rhs((n,), np.float64, seed=seed)
        bbuf.local.copy_(torch.as_tensor(b))
        g.replay()
        torch.cuda.synchronize()
        replayed = x.local.clone()
        eager = gs.sweep(darray.zeros((n,)), b, "symmetric")
        assert torch.equal(replayed, eager.local)
        assert np.allclose(replayed.cpu().numpy(),
                           sweep_oracle(A, gs.order.cpu().numpy(),
                                        np.zeros(n), b, "symmetric"),
                           **tol(np.float64))


# -- the AMG example --------------------------------------------------------------
def _amg(*a):
    r = subprocess.run([sys.executable, os.path.join(EX, "amg.py"), *a],
                       capture_output=True, timeout=300)
    assert r.returncode == 0, \
        r.stdout.decode()[-1200:] + r.stderr.decode()[-1200:]
    out = r.stdout.decode()
    assert "info=0" in out, out
    return out, int(out.split("iters=")[1].split()[0])


def test_amg_gauss_seidel_smoother_gpu():
    out, gs = _amg("-n", "65536", "-maxiter", "100", "-smoother", "gs")
    assert "hipGraph capture unavailable" not in out, out  # stays captured
    _, jacobi = _amg("-n", "65536", "-maxiter", "100", "-smoother", "jacobi")
    print(f"AMG-CG iterations on the GPU: jacobi {jacobi}, gs {gs}")
    assert gs <= jacobi
