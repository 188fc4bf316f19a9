"""Triangular-solve benchmark for one MI355X: python tools/trsv_bench.py

Three structures, fp64, single right-hand side:
  poisson   lower triangle of poisson2d(nx, nx): 2*nx-1 levels of <= nx rows
  random    n rows with 4 random dependencies each: few, wide levels
  bidiag    bidiagonal, n levels of one row: the sequential worst case

For each it reports the analysis time (TriangularSolver construction, host
wall clock ending in a device synchronise), the solve time (HIP events,
warmed up, median and min over repetitions) and two yardsticks measured in
the same run:
  spmv      the project's CSR SpMV kernel on the same strict triangle — a
            lower bound: the same bytes with no dependencies
  host      the route without this solver: b device->host, scipy
            spsolve_triangular, x host->device (host wall clock; the matrix
            is already on the host as scipy CSR, which favours this route)
and the largest relative difference between the two solutions.

It needs a GPU and fails without one; --dry-run only builds the cases and
checks the solver against scipy on whatever device the runtime has (for
rehearsing sizes and paths, prints no timings).
"""
import argparse
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import scipy.sparse as sps  # noqa: E402
import torch  # noqa: E402
from scipy.sparse.linalg import spsolve_triangular as sp_solve  # noqa: E402


def poisson_case(nx):
    from sparse import gallery

    return gallery.poisson2d(nx, nx)


def random_case(n, deps=4, seed=7):
    """Row i > 0: `deps` uniformly random columns below i (duplicates add
    up), magnitudes <= 0.2 under a diagonal of 2."""
    from sparse import csr_array
    from sparse.parallel.partition import RowPartition
    from sparse.runtime import runtime

    dev = runtime().device
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    rows = torch.arange(1, n, dtype=torch.int64).repeat_interleave(deps)
    cols = (torch.rand(rows.numel(), generator=g, dtype=torch.float64)
            * rows).long()
    cols = torch.minimum(cols, rows - 1)
    vals = torch.rand(rows.numel(), generator=g, dtype=torch.float64) * 0.4 - 0.2
    ar = torch.arange(n, dtype=torch.int64)
    key = torch.cat([rows * n + cols, ar * n + ar])
    v = torch.cat([vals, torch.full((n,), 2.0, dtype=torch.float64)])
    key, perm = torch.sort(key)
    r = torch.div(key, n, rounding_mode="floor")
    indptr = torch.zeros(n + 1, dtype=torch.int64)
    torch.cumsum(torch.bincount(r, minlength=n), 0, out=indptr[1:])
    return csr_array.from_local(
        indptr.to(dev), (key - r * n).to(torch.int32).to(dev),
        v[perm].to(dev), RowPartition.equal(n, 1), (n, n))


def bidiag_case(n):
    from sparse import csr_array

    d = np.full(n, 2.0)
    e = np.where(np.arange(n - 1) % 2 == 0, -0.9, 0.7)
    return csr_array(sps.diags([e, d], [-1, 0], format="csr"))


def device_ms(fn, warmup, reps):
    """Per-call device time by HIP events around each call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return out


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def fmt(ts):
    return f"median {statistics.median(ts):10.3f} ms   min {min(ts):10.3f} ms"


def run_case(name, A, reps, emit, dry):
    from sparse import darray, kernels
    from sparse.linalg import TriangularSolver
    from sparse.ops.local import LocalCSR

    n = A.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the sequential-structure warning
        solver = TriangularSolver(A, lower=True)
    kinds = [k for k, _, _ in solver.schedule]
    emit(f"== {name}: n = {n}, strict nnz = {solver._values.numel()}, "
         f"levels = {solver.nlevels}, launches = {len(kinds)} "
         f"({kinds.count('wide')} wide, {kinds.count('chain')} chain)")
    b = darray.ones((n,), dtype=np.float64)
    x = darray.zeros((n,), dtype=np.float64)
    S = sps.tril(A.to_scipy_sparse_csr()).tocsr()
    solver.solve(b, out=x)
    ref = sp_solve(S, np.ones(n), lower=True)
    err = float(np.max(np.abs(np.asarray(x) - ref) / np.maximum(np.abs(ref),
                                                                1e-300)))
    emit(f"   max relative difference to scipy: {err:.2e}")
    if dry:
        return

    def analyse():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            TriangularSolver(A, lower=True)

    emit(f"   analysis  {fmt(wall_ms(analyse, 3))}   (host wall clock)")
    emit(f"   solve     {fmt(device_ms(lambda: solver.solve(b, out=x), 3, reps))}"
         "   (HIP events)")
    strict = LocalCSR(solver._indptr, solver._indices, solver._values, n, n)
    y = torch.empty(n, dtype=torch.float64, device=x.local.device)
    emit(f"   spmv      {fmt(device_ms(lambda: kernels.spmv(strict, b.local, y, 0, 0.0), 3, reps))}"
         "   (HIP events; lower bound)")

    def host_route():
        xh = sp_solve(S, b.local.cpu().numpy(), lower=True)
        return torch.as_tensor(xh).to(b.local.device)

    host_route()
    emit(f"   host      {fmt(wall_ms(host_route, 3))}   (host wall clock)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--poisson-nx", type=int, default=2048)
    ap.add_argument("--random-n", type=int, default=4_000_000)
    ap.add_argument("--bidiag-n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles",
                                                  "trsv_bench.txt"))
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit("trsv_bench: no GPU — timings are only taken on one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if not args.dry_run:
        from sparse.kernels import require

        require()
        emit(f"device: {torch.cuda.get_device_name(0)}; fp64, one right-hand "
             f"side; {args.reps} timed solves per case after 3 warm-ups")
    run_case(f"poisson2d({args.poisson_nx}, {args.poisson_nx}) lower",
             poisson_case(args.poisson_nx), args.reps, emit, args.dry_run)
    run_case("random, 4 dependencies per row", random_case(args.random_n),
             args.reps, emit, args.dry_run)
    run_case("bidiagonal", bidiag_case(args.bidiag_n),
             max(3, args.reps // 4), emit, args.dry_run)
    if not args.dry_run:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
