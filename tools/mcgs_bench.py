"""Multicolour Gauss-Seidel benchmark for one MI355X: python tools/mcgs_bench.py

Two structures, fp64 (the cases of tools/ilu0_bench.py):
  poisson   poisson2d(nx, nx): 5 entries a row, 2*nx-1 levels in natural order
  random    n rows with about 4 random entries below the diagonal, mirrored
            (a symmetric pattern), under a dominant diagonal

For each it reports
  colours   the number of colours, the class sizes and the Jones-Plassmann
            rounds; the colours are compared with the sequential host op
  coloring  greedy_coloring(A) (host wall clock ending in a device
            synchronise: symmetry check, rounds, one host read per round)
  analysis  MulticolorGaussSeidel(A, colors=...) with the colours passed in:
            diagonal, validation, order, schedule (host wall clock)
  sweep     one symmetric sweep from zero, matvec (HIP events, warmed up,
            median and min)
and two yardsticks measured in the same run:
  natural   one application of the natural-order sgs_preconditioner: two
            level-scheduled triangular solves and a scale (HIP events)
  2 spmv    two CSR SpMVs on A — a lower bound: the same bytes with no
            ordering (HIP events)
and, on the Poisson case (step "cg"), CG to the tolerance with no
preconditioner and with the multicolour one (host wall clock, after a short
warm-up run), with the iteration counts; and (step "amg") examples/amg.py
with both smoothers: iterations, setup and solve time as it prints them.

It needs a GPU and fails without one; --dry-run runs every step at a small
size on whatever device the runtime has and prints no timings (for rehearsing
sizes and paths).  --steps runs a subset (poisson, random, cg, amg) so that
each can be given a time limit of its own; --append adds to the output file
instead of replacing it.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ilu0_bench import (_quiet, device_ms, fmt, poisson_case,  # noqa: E402
                        random_case, wall_ms)


def host_colors(A, seed=0):
    """The sequential host colouring of the same graph (the extension's CPU
    op, numpy without it)."""
    from sparse import kernels
    from sparse.gauss_seidel import _graph, _greedy_numpy

    indptr, indices = _graph(A)
    ip, ix = indptr.cpu(), indices.cpu()
    if kernels.ext() is not None:
        return kernels.color_greedy(ip, ix, seed)
    return torch.from_numpy(_greedy_numpy(ip.numpy(), ix.numpy(), seed))


def run_case(name, A, reps, emit, dry):
    from sparse import darray, kernels
    from sparse.gauss_seidel import _greedy_coloring
    from sparse.linalg import MulticolorGaussSeidel, sgs_preconditioner

    n = A.shape[0]
    colors, rounds = _greedy_coloring(A, 0)
    gs = MulticolorGaussSeidel(A, colors=colors)
    sizes = np.diff(gs.color_ptr.cpu().numpy())
    emit(f"== {name}: n = {n}, nnz = {A.nnz}, colours = {gs.ncolors}, "
         f"rounds = {rounds}, class sizes "
         f"{' / '.join(f'{100.0 * s / max(n, 1):.1f}' for s in sizes)} %, "
         f"lanes per row {sorted(set(gs._sched[:, 3].tolist()))}")
    same = bool(torch.equal(colors.cpu(), host_colors(A)))
    emit(f"   colours equal to the sequential host op: {same}")
    assert same
    b = darray.ones((n,), dtype=np.float64)
    x = darray.zeros((n,), dtype=np.float64)
    if dry:
        gs.matvec(b, out=x)
        emit(f"   dry run: |M^-1 1| = {float(x.norm().item()):.6e}")
        return
    emit(f"   coloring  {fmt(wall_ms(lambda: _greedy_coloring(A, 0), 3))}"
         "   (host wall clock)")
    emit(f"   analysis  {fmt(wall_ms(lambda: MulticolorGaussSeidel(A, colors=colors), 3))}"
         "   (host wall clock; colours passed in)")
    emit(f"   sweep     {fmt(device_ms(lambda: gs.matvec(b, out=x), 3, reps))}"
         f"   (HIP events; symmetric, {2 * gs.ncolors} launches)")
    nat = _quiet(lambda: sgs_preconditioner(A))
    launches = len(nat._L.schedule) + len(nat._U.schedule)
    emit(f"   natural   {fmt(device_ms(lambda: nat.matvec(b, out=x), 3, reps))}"
         f"   (HIP events; natural-order SGS, {launches} launches)")
    y = torch.empty(n, dtype=torch.float64, device=b.local.device)

    def two_spmv():
        kernels.spmv(A.local, b.local, y, 0, 0.0)
        kernels.spmv(A.local, b.local, y, 0, 0.0)

    emit(f"   2 spmv    {fmt(device_ms(two_spmv, 3, reps))}"
         "   (HIP events; lower bound)")


def run_cg(nx, tol, maxiter, emit, dry):
    from sparse import darray
    from sparse.linalg import cg, sgs_preconditioner

    A = poisson_case(nx)
    n = A.shape[0]
    b = darray.ones((n,), dtype=np.float64)
    emit(f"== CG on poisson2d({nx}, {nx}), b = 1, tol {tol:g}, residual "
         "tested every 25 iterations")
    makers = [("none", lambda: None),
              ("multicolour SGS",
               lambda: sgs_preconditioner(A, ordering="multicolor"))]
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
            emit(f"   {name:15s} dry run: {count[0]} iterations ran")
            continue
        cg(A, b, tol=tol, maxiter=5, M=M)  # warm-up
        torch.cuda.synchronize()
        count[0] = 0
        t = time.perf_counter()
        x, info = cg(A, b, tol=tol, maxiter=maxiter, M=M, callback=cb)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) * 1e3
        res = float((b - A.dot(x)).norm().item()) / float(b.norm().item())
        emit(f"   {name:15s} setup {setup:10.1f} ms   solve {ms:10.1f} ms   "
             f"{count[0]:6d} iterations   info {info}   |r|/|b| {res:.2e}")


def run_amg(n, emit):
    emit(f"== examples/amg.py -n {n} -maxiter 200 (its own output line)")
    for smoother in ("jacobi", "gs"):
        r = subprocess.run(
            [sys.executable, os.path.join(ROOT, "examples", "amg.py"), "-n",
             str(n), "-maxiter", "200", "-smoother", smoother],
            capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"mcgs_bench: amg.py -smoother {smoother} failed:\n"
                     + r.stdout[-1500:] + r.stderr[-1500:])
        line = [l for l in r.stdout.splitlines() if "iters=" in l][-1]
        emit(f"   {smoother:7s} {line}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--poisson-nx", type=int, default=2048)
    ap.add_argument("--random-n", type=int, default=4_000_000)
    ap.add_argument("--amg-n", type=int, default=1_048_576)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cg-tol", type=float, default=1e-6)
    ap.add_argument("--cg-maxiter", type=int, default=20000)
    ap.add_argument("--steps", default="poisson,random,cg,amg")
    ap.add_argument("--out", default=os.path.join("profiles",
                                                  "mcgs_bench.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args()
    if not args.dry_run and not torch.cuda.is_available():
        sys.exit("mcgs_bench: no GPU — timings are only taken on one")
    if args.dry_run:
        args.poisson_nx = min(args.poisson_nx, 64)
        args.random_n = min(args.random_n, 20_000)
        args.amg_n = min(args.amg_n, 4096)
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
    if "amg" in steps:
        run_amg(args.amg_n, emit)
    if not args.dry_run:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
