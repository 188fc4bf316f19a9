"""ILU(0) benchmark for one MI355X: python tools/ilu0_bench.py

Two structures, fp64:
  poisson   poisson2d(nx, nx): 2*nx-1 levels of <= nx rows, 5 entries a row
  random    n rows with about 4 random entries below the diagonal, mirrored
            (a symmetric pattern), under a dominant diagonal: few, wide levels

For each it reports
  ilu0()    analysis plus the first factorisation (host wall clock ending in
            a device synchronise)
  factor    the numeric phase alone: the factorisation kernels over a fresh
            copy of A's values (HIP events, warmed up, median and min)
  refactor  ILU0.refactor: copy, kernels, new solver values and the one host
            read of the pivot word (host wall clock)
  solve     one U^-1 L^-1 r (HIP events), and the L solve alone: the
            factorisation runs the same schedule
and two yardsticks measured in the same run:
  spmv      the project's CSR SpMV kernel on the same matrix — a lower
            bound: the same bytes with no dependencies
  host      the route without this kernel: values device->host, the
            extension's sequential CPU op, factor host->device (host wall
            clock; the structure is already on the host, which favours it)
and, on the Poisson case (step "cg"), the time CG takes to reach the
tolerance with no preconditioner, SGS and ILU(0) (host wall clock, after a
short warm-up run), with the iteration counts.

It needs a GPU and fails without one; --dry-run only builds the cases and
checks the factor against the host op on whatever device the runtime has
(for rehearsing sizes and paths, prints no timings).  --steps runs a subset
(poisson, random, cg) so that each can be given a time limit of its own;
--append adds to the output file instead of replacing it.
"""
import argparse
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def poisson_case(nx):
    from sparse import gallery

    return gallery.poisson2d(nx, nx)


def random_case(n, deps=4, seed=7):
    """Row i > 0: `deps` uniformly random columns below i, duplicates
    dropped, mirrored through the diagonal; magnitudes <= 0.2 and
    |a_ii| = 1 + sum_j |a_ij|."""
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
    ar = torch.arange(n, dtype=torch.int64)
    key = torch.unique(torch.cat([rows * n + cols, cols * n + rows,
                                  ar * n + ar]))  # sorted, duplicate-free
    r = torch.div(key, n, rounding_mode="floor")
    c = key - r * n
    v = torch.rand(key.numel(), generator=g, dtype=torch.float64) * 0.4 - 0.2
    off = r != c
    rowsum = torch.zeros(n, dtype=torch.float64)
    rowsum.index_add_(0, r[off], v[off].abs())
    v[~off] = 1.0 + rowsum
    indptr = torch.zeros(n + 1, dtype=torch.int64)
    torch.cumsum(torch.bincount(r, minlength=n), 0, out=indptr[1:])
    return csr_array.from_local(
        indptr.to(dev), c.to(torch.int32).to(dev), v.to(dev),
        RowPartition.equal(n, 1), (n, n))


def device_ms(fn, warmup, reps, before=None):
    """Per-call device time by HIP events around each call; `before` runs
    ahead of each call, outside the timed window."""
    out = []
    for it in range(warmup + reps):
        if before is not None:
            before()
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if it >= warmup:
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


def _quiet(fn):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the sequential-structure warning
        return fn()


def host_factor(host, values):
    """The extension's CPU op (numpy without it) on host copies; returns the
    factor's values on the host."""
    from sparse import kernels
    from sparse.ilu import _ilu0_numpy

    v = values.cpu().clone()
    ip, ix, dp = host
    if kernels.ext() is not None:
        flag = torch.full((1,), torch.iinfo(torch.int64).max)
        empty = torch.zeros(0, dtype=torch.int64)
        kernels.ext().ilu0_factor(ip, ix, v, dp, empty, empty,
                                  torch.zeros((0, 4), dtype=torch.int64),
                                  flag)
    else:
        _ilu0_numpy(ip.numpy(), ix.numpy(), v.numpy(), dp.numpy())
    return v


def run_case(name, A, reps, emit, dry):
    from sparse import darray, kernels
    from sparse.linalg import ilu0

    n = A.shape[0]
    fac = _quiet(lambda: ilu0(A))
    host = (fac._indptr.cpu(), fac._indices.cpu(), fac._diag_ptr.cpu())
    kinds = [k for k, _, _ in fac.schedule]
    emit(f"== {name}: n = {n}, nnz = {fac.nnz}, levels = {fac.nlevels}, "
         f"launches = {len(kinds)} ({kinds.count('wide')} wide, "
         f"{kinds.count('chain')} chain), lanes per row "
         f"{sorted(set(fac._sched[:, 3].tolist()))}")
    vals = A.local.values
    ref = host_factor(host, vals)
    err = float(((fac._fvals.cpu() - ref).abs()
                 / ref.abs().clamp_min(1e-300)).max()) if n else 0.0
    emit(f"   max relative difference to the host op: {err:.2e}")
    if dry:
        return
    dev = vals.device
    emit(f"   ilu0()    {fmt(wall_ms(lambda: _quiet(lambda: ilu0(A)), 3))}"
         "   (host wall clock; analysis + first factorisation)")
    fv = torch.empty_like(vals)
    flag = torch.full((1,), torch.iinfo(torch.int64).max, dtype=torch.int64,
                      device=dev)
    emit(f"   factor    {fmt(device_ms(lambda: kernels.ilu0_factor(fac, fv, flag), 3, reps, before=lambda: fv.copy_(vals)))}"
         "   (HIP events; kernels only)")
    assert int(flag.item()) >= n
    emit(f"   refactor  {fmt(wall_ms(lambda: fac.refactor(A), max(3, reps // 4)))}"
         "   (host wall clock)")
    b = darray.ones((n,), dtype=np.float64)
    x = darray.zeros((n,), dtype=np.float64)
    emit(f"   solve     {fmt(device_ms(lambda: fac.solve(b, out=x), 3, reps))}"
         "   (HIP events; L then U)")
    emit(f"   L solve   {fmt(device_ms(lambda: fac._Ls.solve(b, out=x), 3, reps))}"
         "   (HIP events; same schedule as the factorisation)")
    y = torch.empty(n, dtype=torch.float64, device=dev)
    emit(f"   spmv      {fmt(device_ms(lambda: kernels.spmv(A.local, b.local, y, 0, 0.0), 3, reps))}"
         "   (HIP events; lower bound)")
    host_factor(host, vals)
    emit(f"   host      {fmt(wall_ms(lambda: host_factor(host, vals).to(dev), 3))}"
         "   (host wall clock)")


def run_cg(nx, tol, maxiter, emit, dry):
    from sparse import darray
    from sparse.linalg import cg, ilu0, sgs_preconditioner

    A = poisson_case(nx)
    n = A.shape[0]
    b = darray.ones((n,), dtype=np.float64)
    emit(f"== CG on poisson2d({nx}, {nx}), b = 1, tol {tol:g}, residual "
         "tested every 25 iterations")
    makers = [("none", lambda: None),
              ("SGS", lambda: sgs_preconditioner(A)),
              ("ILU(0)", lambda: ilu0(A))]
    for name, make in makers:
        t = time.perf_counter()
        M = _quiet(make)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        setup = (time.perf_counter() - t) * 1e3
        count = [0]

        def cb(_x):
            count[0] += 1

        if dry:
            x, info = cg(A, b, tol=tol, maxiter=50, M=M, callback=cb)
            emit(f"   {name:7s} dry run: {count[0]} iterations ran")
            continue
        cg(A, b, tol=tol, maxiter=5, M=M)  # warm-up
        torch.cuda.synchronize()
        count[0] = 0
        t = time.perf_counter()
        x, info = cg(A, b, tol=tol, maxiter=maxiter, M=M, callback=cb)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3
        res = float((b - A.dot(x)).norm().item()) / float(b.norm().item())
        emit(f"   {name:7s} setup {setup:10.1f} ms   solve {ms:10.1f} ms   "
             f"{count[0]:6d} iterations   info {info}   |r|/|b| {res:.2e}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--poisson-nx", type=int, default=2048)
    ap.add_argument("--random-n", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cg-tol", type=float, default=1e-6)
    ap.add_argument("--cg-maxiter", type=int, default=20000)
    ap.add_argument("--steps", default="poisson,random,cg")
    ap.add_argument("--out", default=os.path.join("profiles",
                                                  "ilu0_bench.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit("ilu0_bench: no GPU — timings are only taken on one")
    steps = args.steps.split(",")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if not args.dry_run:
        from sparse.kernels import require

        require()
        if not args.append:
            emit(f"device: {torch.cuda.get_device_name(0)}; fp64; "
                 f"{args.reps} timed repetitions per figure after 3 warm-ups "
                 "unless stated")
    if "poisson" in steps:
        run_case(f"poisson2d({args.poisson_nx}, {args.poisson_nx})",
                 poisson_case(args.poisson_nx), args.reps, emit, args.dry_run)
    if "random" in steps:
        run_case("random symmetric pattern, ~4 entries below the diagonal "
                 "per row", random_case(args.random_n), args.reps, emit,
                 args.dry_run)
    if "cg" in steps:
        run_cg(args.poisson_nx, args.cg_tol, args.cg_maxiter, emit,
               args.dry_run)
    if not args.dry_run:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
