"""bench.py command-line contract: plain vs --full result line and
--dump-outputs (CPU, one rank, tiny grid)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX = 24


def _bench(*extra, nx=NX, gpu=False):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    if not gpu:
        env["CUDA_VISIBLE_DEVICES"] = env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", "--nx", str(nx), *extra],
        env=env, capture_output=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout.decode()[-800:]
    return json.loads(line[0])


def _cg_reference(nx, iters):
    """Plain numpy CG on the 5-pt Poisson system with b = 1, x0 = 0."""
    import scipy.sparse as sps

    T = sps.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx))
    A = (sps.kron(sps.identity(nx), T) + sps.kron(T, sps.identity(nx))).tocsr()
    b = np.ones(nx * nx)
    x = np.zeros_like(b)
    r = b.copy()
    p = r.copy()
    rz = r @ r
    for _ in range(iters):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        rz_new = r @ r
        p = r + (rz_new / rz) * p
        rz = rz_new
    return x, r, p, rz


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d1 = tmp_path_factory.mktemp("dump_plain")
    d2 = tmp_path_factory.mktemp("dump_full")
    plain = _bench("--dump-outputs", str(d1))
    full = _bench("--full", "--dump-outputs", str(d2))
    return plain, full, d1, d2


def test_result_line_plain_and_full(runs):
    plain, full, _, _ = runs
    for rec in (plain, full):
        assert rec["metric"] == "cg_iters_per_sec" and rec["unit"] == "iters/s"
        assert rec["higher_is_better"] is True and rec["dtype"] == "fp64"
        assert rec["steps"] == 3 and rec["warmup"] == 1
        assert rec["ms_per_step"] > 0
        assert np.isclose(rec["value"], 1000.0 / rec["ms_per_step"])
    assert "spmv_gflops" not in plain["config"]
    assert full["config"]["spmv_gflops"] > 0
    assert full["config"]["spmv_effective_gbps"] > 0


def test_dump_outputs_reproducible_and_correct(runs):
    """The dump is the CG state after warmup + steps iterations: identical
    across runs, float64, and equal to a plain numpy CG on the same system."""
    _, _, d1, d2 = runs
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2))
    assert {"x.npy", "r.npy", "p.npy", "q.npy", "rz.npy"} <= set(names)
    got = {}
    for nm in names:
        a, b = np.load(d1 / nm), np.load(d2 / nm)
        assert a.dtype == np.float64
        assert np.array_equal(a, b), nm
        got[nm[:-4]] = a
    x, r, p, rz = _cg_reference(NX, 4)  # warmup 1 + steps 3
    assert got["x"].shape == (NX * NX,)
    assert np.allclose(got["x"], x, rtol=1e-10, atol=1e-12)
    assert np.allclose(got["r"], r, rtol=1e-10, atol=1e-12)
    assert np.allclose(got["p"], p, rtol=1e-10, atol=1e-12)
    assert np.allclose(got["rz"], rz, rtol=1e-10)


@pytest.mark.gpu
def test_dump_outputs_gpu_sampled(tmp_path):
    """GPU path at a size above the whole-vector limit: the dump is a fixed
    sample (positions in sample_index.npy) of the state after the 4
    pre-capture iterations + warmup 1 + steps 3.  Tolerance: 8 iterations
    of fp64 reductions over 1.2M terms in a different order than numpy's,
    well below 1e-10 relative."""
    nx = 1100
    rec = _bench("--dump-outputs", str(tmp_path), nx=nx, gpu=True)
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    idx = got["sample_index"].astype(np.int64)
    assert idx.shape == (1 << 20,) and len(np.unique(idx)) == idx.size
    assert idx.min() >= 0 and idx.max() < nx * nx
    x, r, p, rz = _cg_reference(nx, 8)
    for name, ref in (("x", x), ("r", r), ("p", p)):
        assert got[name].dtype == np.float64
        assert np.allclose(got[name], ref[idx], rtol=1e-10, atol=1e-12), name
    assert np.allclose(got["rz"], rz, rtol=1e-10)
