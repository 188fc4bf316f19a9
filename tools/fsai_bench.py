"""FSAI benchmark for one MI355X: python tools/fsai_bench.py

The two structures of tools/ilu0_bench.py, fp64:
  poisson   poisson2d(nx, nx), pattern tril(A^power) for power 1, 2, 3
  random    n rows with about 4 random entries below the diagonal, mirrored,
            under a dominant positive diagonal; fsai reads its lower triangle
            only, which makes it the symmetric positive definite matrix with
            that triangle; power 1

For each it reports
  fsai()    analysis plus the first numeric phase (host wall clock ending in a
            device synchronise), and the analysis alone as the difference to
  numeric   the numeric phase alone: the per-row kernels into G's values (HIP
            events, warmed up, median and min)
  refactor  FSAI.refactor: kernels, the values of G^H, the one host read of the
            breakdown word (host wall clock)
  apply     one z = G^H (G r) (HIP events) and which SpMV mirror G and G^H got
and two yardsticks measured in the same run:
  spmv      the project's CSR SpMV kernel on A, and A.dot through A's own
            mirror
  2 spmv    two of the CSR kernel back to back: what the apply would cost if
            G had A's entries
and, on the Poisson case (step "cg"), the time CG takes to reach the
tolerance with no preconditioner and with FSAI of each power (host wall
clock, after a short warm-up run), with the iteration counts.

It needs a GPU and fails without one; --dry-run only builds the cases and
checks G against the host path on whatever device the runtime has (prints no
timings).  --steps runs a subset (poisson, random, cg) so that each can be
given a time limit of its own; --append adds to the output file instead of
replacing it.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ilu0_bench import (device_ms, fmt, poisson_case, random_case,  # noqa: E402
                        wall_ms)


def mirror(M):
    """Which SpMV path csr_array.dot takes for M."""
    dm = M._dia()
    if dm is not None:
        return (f"DIA, {dm.W} diagonals"
                + (", constant planes" if dm.compressed else ""))
    ell = M._ell()
    if ell is not None:
        return f"ELL, width {ell.W}"
    return "CSR (nnz-split)"


def host_check(fac, A):
    """Largest relative difference of G to the numpy host path on a sample of
    rows (the first 2000: the host loop is slow)."""
    from sparse.fsai import _fsai_numpy

    k = min(2000, A.shape[0])
    pip = fac._indptr[: k + 1].cpu().numpy()
    pix = fac._indices[: int(pip[-1])].cpu().numpy()
    lc = A.local
    gv = np.zeros(int(pip[-1]), dtype=np.float64)
    # rows < k of a lower pattern only reference rows < k of A
    aip = lc.indptr[: k + 1].cpu().numpy()
    bad = _fsai_numpy(aip, lc.indices[: int(aip[-1])].cpu().numpy(),
                      lc.values[: int(aip[-1])].cpu().numpy(), pip, pix, gv)
    assert bad == k
    got = fac.G._values[: int(pip[-1])].cpu().numpy()
    return float(np.abs(got - gv).max() / np.abs(gv).max())


def run_case(name, A, power, reps, emit, dry):
    from sparse import darray, kernels
    from sparse.linalg import fsai

    n = A.shape[0]
    fac = fsai(A, power=power)
    emit(f"== {name}, power {power}: n = {n}, nnz(A) = {A.nnz}, nnz(G) = "
         f"{fac.nnz}, longest row {fac.max_row}, launches (lanes per row, "
         f"rows) {fac.row_classes}")
    emit(f"   max difference to the host path, first rows: "
         f"{host_check(fac, A):.2e}")
    if dry:
        return
    vals = A.local.values
    dev = vals.device
    total = wall_ms(lambda: fsai(A, power=power), 3)
    gv = torch.zeros_like(fac.G._values)
    flag = torch.full((1,), torch.iinfo(torch.int64).max, dtype=torch.int64,
                      device=dev)
    numeric = device_ms(lambda: kernels.fsai_factor(fac, vals, gv, flag), 3,
                        reps)
    assert int(flag.item()) >= n and torch.equal(gv, fac.G._values)
    emit(f"   fsai()    {fmt(total)}   (host wall clock; analysis + first "
         "numeric phase)")
    emit(f"   numeric   {fmt(numeric)}   (HIP events; kernels only)")
    emit(f"   analysis  about {statistics.median(total) - statistics.median(numeric):10.3f} ms"
         "   (fsai() minus numeric, medians)")
    emit(f"   refactor  {fmt(wall_ms(lambda: fac.refactor(A), max(3, reps // 4)))}"
         "   (host wall clock)")
    b = darray.ones((n,), dtype=np.float64)
    x = darray.zeros((n,), dtype=np.float64)
    fac.solve(b, out=x)
    emit(f"   apply     {fmt(device_ms(lambda: fac.solve(b, out=x), 3, reps))}"
         f"   (HIP events; G: {mirror(fac.G)}; GH: {mirror(fac.GH)})")
    y = torch.empty(n, dtype=torch.float64, device=dev)
    spmv = lambda: kernels.spmv(A.local, b.local, y, 0, 0.0)  # noqa: E731
    emit(f"   spmv      {fmt(device_ms(spmv, 3, reps))}"
         "   (HIP events; CSR kernel on A)")
    emit(f"   2 spmv    {fmt(device_ms(lambda: (spmv(), spmv()), 3, reps))}"
         "   (HIP events; CSR kernel on A, twice)")
    A.dot(b, out=x)
    emit(f"   A.dot     {fmt(device_ms(lambda: A.dot(b, out=x), 3, reps))}"
         f"   (HIP events; A: {mirror(A)})")


def run_cg(nx, tol, maxiter, emit, dry):
    from sparse import darray
    from sparse.linalg import cg, fsai

    A = poisson_case(nx)
    n = A.shape[0]
    b = darray.ones((n,), dtype=np.float64)
    emit(f"== CG on poisson2d({nx}, {nx}), b = 1, tol {tol:g}, residual "
         "tested every 25 iterations")
    makers = [("none", lambda: None)] + [
        (f"FSAI p={p}", (lambda p=p: fsai(A, power=p))) for p in (1, 2, 3)]
    for name, make in makers:
        t = time.perf_counter()
        M = make()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        setup = (time.perf_counter() - t) * 1e3
        count = [0]

        def cb(_x):
            count[0] += 1

        if dry:
            x, info = cg(A, b, tol=tol, maxiter=50, M=M, callback=cb)
            emit(f"   {name:8s} dry run: {count[0]} iterations ran")
            continue
        cg(A, b, tol=tol, maxiter=5, M=M)  # warm-up
        torch.cuda.synchronize()
        count[0] = 0
        t = time.perf_counter()
        x, info = cg(A, b, tol=tol, maxiter=maxiter, M=M, callback=cb)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3
        res = float((b - A.dot(x)).norm().item()) / float(b.norm().item())
        emit(f"   {name:8s} setup {setup:10.1f} ms   solve {ms:10.1f} ms   "
             f"{count[0]:6d} iterations   {ms / max(count[0], 1):7.3f} ms "
             f"each   info {info}   |r|/|b| {res:.2e}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--poisson-nx", type=int, default=2048)
    ap.add_argument("--random-n", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cg-tol", type=float, default=1e-6)
    ap.add_argument("--cg-maxiter", type=int, default=20000)
    ap.add_argument("--steps", default="poisson,random,cg")
    ap.add_argument("--out", default=os.path.join("profiles",
                                                  "fsai_bench.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit("fsai_bench: no GPU — timings are only taken on one")
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
        A = poisson_case(args.poisson_nx)
        for power in (1, 2, 3):
            run_case(f"poisson2d({args.poisson_nx}, {args.poisson_nx})", A,
                     power, args.reps, emit, args.dry_run)
    if "random" in steps:
        run_case("random symmetric pattern, ~4 entries below the diagonal "
                 "per row", random_case(args.random_n), 1, args.reps, emit,
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
