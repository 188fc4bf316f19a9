"""Smoothed-aggregation AMG preconditioned CG.

Capability parity with reference examples/amg.py: strength-of-connection
filtering (amg.py:134-146), MIS-based aggregation (amg.py:199-283),
tentative prolongator from the candidate vector (fit_candidates,
amg.py:148-158), Jacobi-smoothed prolongator with a spectral-radius
estimate (amg.py:160-197), Galerkin coarse operators R@A@P (the distributed
SpGEMM benchmark path, amg.py:390), V-cycle + CG (amg.py:354-474).

Setup-graph aggregation runs on the gathered structure host-side (the
hierarchy is built once); all operator algebra (A@P, R@(AP), smoothing,
V-cycles, CG) runs distributed on the GPUs.

python examples/amg.py -n 262144 -maxiter 200
python examples/amg.py -n 262144 -smoother gs   (multicolour Gauss-Seidel
                                                 smoothing, one GPU)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import scipy.sparse as sps

from benchmark import parse_common_args

parser = argparse.ArgumentParser()
parser.add_argument("-n", type=int, default=16384, help="problem size (grid^2)")
parser.add_argument("-theta", type=float, default=0.0)
parser.add_argument("-maxiter", type=int, default=400)
parser.add_argument("-tol", type=float, default=1e-8)
parser.add_argument("-max_coarse", type=int, default=512)
parser.add_argument("-smoother", choices=["jacobi", "gs"], default="jacobi",
                    help="weighted Jacobi, or multicolour Gauss-Seidel "
                         "(one GPU only)")
# parse argv only when run as a script: importing this module (e.g. the
# pyamg bridge reusing vcycle) must not react to the host program's argv
args, _ = parser.parse_known_args(None if __name__ == "__main__" else [])
_, timer, npx, sparse, linalg, use_sparse = parse_common_args(
    None if __name__ == "__main__" else [])

from sparse import csr_array, darray, gallery
from sparse.parallel import comm


def strength_mask_host(S: sps.csr_matrix, theta: float) -> sps.csr_matrix:
    """Symmetric strength of connection: keep |a_ij| >= theta*sqrt(a_ii a_jj)
    (reference amg.py:134-146)."""
    if theta <= 0:
        return S
    d = np.sqrt(np.abs(S.diagonal()))
    C = S.tocoo()
    keep = np.abs(C.data) >= theta * d[C.row] * d[C.col]
    keep |= C.row == C.col
    return sps.csr_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=S.shape)


def aggregate_host(C: sps.csr_matrix) -> np.ndarray:
    """Greedy MIS(2)-style aggregation (role of reference amg.py:199-283).
    Returns agg id per node (-1 only transiently)."""
    n = C.shape[0]
    agg = -np.ones(n, dtype=np.int64)
    indptr, indices = C.indptr, C.indices
    next_agg = 0
    # pass 1: seed aggregates from nodes with no aggregated neighbors
    for i in range(n):
        if agg[i] != -1:
            continue
        neigh = indices[indptr[i]: indptr[i + 1]]
        if np.all(agg[neigh] == -1):
            agg[i] = next_agg
            agg[neigh] = next_agg
            next_agg += 1
    # pass 2: attach leftovers to any aggregated neighbor
    for i in range(n):
        if agg[i] != -1:
            continue
        neigh = indices[indptr[i]: indptr[i + 1]]
        cand = agg[neigh]
        cand = cand[cand != -1]
        if len(cand):
            agg[i] = cand[0]
        else:
            agg[i] = next_agg
            next_agg += 1
    return agg


def aggregate_device(C: csr_array, seed: int = 17) -> np.ndarray:
    """Luby-style MIS aggregation on the DEVICE using the tropical
    (max, lexicographic) semiring SpMV — the distributed counterpart of the
    reference's maximal_independent_set + mis_aggregate (amg.py:199-283).

    Round structure: unaggregated local priority maxima become aggregate
    roots; their unaggregated neighbors join them; repeat.  Returns the
    aggregate id per node (gathered numpy)."""
    import torch

    n = C.shape[0]
    rng = np.random.default_rng(seed)
    prio_g = rng.permutation(n).astype(np.int64) + 1  # distinct, >= 1
    prio = darray.asdistarray(prio_g)
    ids = darray.arange(n)
    agg = darray.asdistarray(np.full(n, -1, dtype=np.int64))
    root_of = darray.asdistarray(np.full(n, -1, dtype=np.int64))
    def trop(fields):
        return C.tropical_spmv(darray.DistArray.from_local(
            fields, agg.partition, (n, 2))).local

    # Saturated distance-2 root selection, then attachment — measured A/B
    # at 128^2/256^2 against alternatives (iters, opcx with the same
    # smoothed-P build; host greedy = the reference's quality):
    #   one-shot mis2 + joins:    15 it, 1.26   (65 it at 1M)
    #   mis1 + join:               7 it, 2.08 at 128^2 BUT 25 it, 2.43 at 256^2
    #   saturated mis2 (this):    12 it, 1.30
    #   host greedy:               7 it, 1.30
    # Saturating roots first (candidates = nodes at distance >= 3 from all
    # existing roots) packs roots at host-like spacing before any
    # attachment, fixing the sparse-root/large-fringe quality loss of the
    # one-shot variant.
    root = torch.zeros_like(agg.local, dtype=torch.bool)
    cand = torch.ones_like(root)
    for _round in range(64):
        if not bool(comm_any(cand)):
            break
        f0 = torch.where(cand, prio.local, torch.zeros_like(prio.local))
        nb2 = trop(trop(torch.stack([f0, ids.local], dim=1)))
        newroots = cand & (f0 == nb2[:, 0]) & (f0 > 0)
        if not bool(comm_any(newroots)):
            break
        root |= newroots
        rf = torch.where(root, prio.local, torch.zeros_like(prio.local))
        ball2 = trop(trop(torch.stack([rf, ids.local], dim=1)))[:, 0] > 0
        cand = cand & ~ball2 & ~root
    agg.local[root] = ids.local[root]
    # attach: distance-1 to a root, then distance-2 via an aggregated
    # neighbor
    rf = torch.where(root, prio.local, torch.zeros_like(prio.local))
    j1 = trop(torch.stack([rf, ids.local], dim=1))
    live = agg.local < 0
    join = live & (j1[:, 0] > 0)
    agg.local[join] = j1[join, 1]
    for _ in range(2):
        af = torch.where(agg.local >= 0, prio.local,
                         torch.zeros_like(prio.local))
        j2 = trop(torch.stack([af, agg.local], dim=1))
        live = agg.local < 0
        if not bool(comm_any(live)):
            break
        join2 = live & (j2[:, 0] > 0)
        agg.local[join2] = j2[join2, 1]
    # leftovers (isolated): own aggregate
    left = agg.local < 0
    agg.local[left] = ids.local[left]
    # compact ids
    g = agg.gather().cpu().numpy()
    _, compact = np.unique(g, return_inverse=True)
    return compact


def comm_any(mask) -> bool:
    import torch

    t = mask.any().to(torch.int32)
    from sparse.parallel import comm as _c

    _c.all_reduce_(t, op="max")
    return bool(t.item())


def build_hierarchy(A: csr_array, theta: float, max_coarse: int,
                    smoother: str = "jacobi"):
    """Returns list of levels: dicts with A, P, R, dinv, omega and, with
    smoother="gs", gs: the level's MulticolorGaussSeidel (colouring and
    analysis are part of the setup)."""
    levels = []
    cur = A
    while cur.shape[0] > max_coarse and len(levels) < 20:
        # ---- setup graph on gathered structure (host) ----------------------
        if os.environ.get("SPARSE_AMG_HOST_AGG"):
            S = cur.to_scipy_sparse_csr()
            agg = aggregate_host(strength_mask_host(S, theta))
        else:
            Cs = cur  # theta=0: full connectivity strength graph
            if theta > 0:
                S = cur.to_scipy_sparse_csr()
                Cs = csr_array(strength_mask_host(S, theta))
            agg = aggregate_device(Cs)
        nc = int(agg.max()) + 1
        if nc >= 0.9 * cur.shape[0]:  # aggregation stalled
            break
        if nc >= cur.shape[0]:
            break
        # tentative prolongator: T[i, agg[i]] = 1, column-normalized —
        # exactly one nnz per row, built directly as device slabs (no
        # scipy round-trip)
        import torch as _t

        dev = cur._values.device
        agg_t = _t.as_tensor(agg, device=dev)
        counts_t = _t.bincount(agg_t, minlength=nc).to(_t.float64)
        vals_all = 1.0 / _t.sqrt(counts_t[agg_t])
        me_r = comm.rank()
        s0, s1 = cur.partition.start(me_r), cur.partition.stop(me_r)
        idt = _t.int32 if nc < 2**31 - 1 else _t.int64
        Td = csr_array.from_local(
            _t.arange(s1 - s0 + 1, dtype=_t.int64, device=dev),
            agg_t[s0:s1].to(idt), vals_all[s0:s1].to(cur._values.dtype),
            cur.partition, (cur.shape[0], nc))
        # ---- smoothed prolongator: P = (I - omega D^-1 A) T (distributed) --
        dinv_vec = 1.0 / cur.diagonal().gather()
        # rho(D^-1 A) power iteration
        x = darray.random((cur.shape[0],), seed=3)
        dv = darray.asdistarray(dinv_vec)
        rho = 1.0
        for _ in range(10):
            y = cur.dot(x) * dv
            rho = float(y.norm().item())
            x = y * (1.0 / max(rho, 1e-30))
        omega = (4.0 / 3.0) / max(rho, 1e-30)
        # scale rows of A by -omega*dinv (structure preserving)
        import torch

        lc = cur.local
        rows_local = torch.repeat_interleave(
            torch.arange(lc.nrows, device=lc.device),
            (lc.indptr[1:] - lc.indptr[:-1]))
        dloc = torch.as_tensor(
            dinv_vec[cur.partition.start(comm.rank()): cur.partition.stop(comm.rank())],
            device=lc.device)
        scaled_vals = -omega * lc.values * dloc[rows_local]
        DinvA = csr_array.from_local(lc.indptr, lc.indices, scaled_vals,
                                     cur.partition, cur.shape)
        P = (DinvA @ Td) + Td  # (I - omega D^-1 A) T
        R = P.T.tocsr()  # materialized row-partitioned (ELL restriction)
        AP = cur @ P
        Ac = R @ AP  # Galerkin product (distributed SpGEMM chain)
        d = cur.diagonal()
        levels.append({
            "A": cur, "P": P, "R": R,
            "dinv": darray.DistArray.from_local(1.0 / d.local, d.partition, d.shape),
            "omega": omega,
        })
        if smoother == "gs":
            # the Galerkin operators are unstructured: coloured, not
            # red-black by grid parity
            levels[-1]["gs"] = linalg.MulticolorGaussSeidel(cur)
        cur = Ac
    import torch

    coarse = cur.to_scipy_sparse_csr().toarray()
    levels.append({"A": cur, "coarse_inv": torch.as_tensor(
        np.linalg.pinv(coarse), device=cur._values.device,
        dtype=cur._values.dtype)})
    return levels


class _Shim:
    pass


def build_repl_tail(levels, repl_threshold=1 << 16, smooth_iters=2):
    """Replicated coarse tail at ws>1 (sparse.multigrid; same latency plan
    as gmg.py): returns (ReplicatedCoarseCycle | None, cut index)."""
    from sparse.multigrid import ReplicatedCoarseCycle, find_replication_cut

    ri = find_replication_cut(levels, repl_threshold)
    if comm.world_size() == 1 or ri >= len(levels):
        return None, len(levels)
    shims = []
    for l in levels[ri:]:
        sh = _Shim()
        sh.A = l["A"]
        if "dinv" in l:
            sh.dinv = l["dinv"]
            sh.omega = l["omega"]
        if "R" in l:
            sh.Rdown = l["R"]
            sh.Pdown = l["P"]
        shims.append(sh)
    return ReplicatedCoarseCycle(shims, levels[-1]["coarse_inv"],
                                 smooth_iters), ri


def vcycle(levels, li, b, repl=None, ri=None):
    from sparse.parallel import comm as _comm

    lvl = levels[li]
    if repl is not None and li == ri:
        bf = b.gather() if _comm.world_size() > 1 else b.local
        xf = repl.apply(bf)
        me = _comm.rank()
        return darray.DistArray.from_local(
            xf[b.partition.start(me): b.partition.stop(me)].clone(),
            b.partition, b.gshape)
    if "coarse_inv" in lvl:
        bg = b.gather() if _comm.world_size() > 1 else b.local
        return darray.asdistarray(lvl["coarse_inv"] @ bg)
    if "gs" in lvl:
        # two forward sweeps from x = 0 before, two backward sweeps after the
        # coarse correction: the post-smoother is the adjoint of the
        # pre-smoother, so the cycle stays symmetric for CG
        import torch

        A, gs = lvl["A"], lvl["gs"]
        x = darray.DistArray.from_local(torch.zeros_like(b.local),
                                        b.partition, b.gshape)
        gs.sweep(x, b, "forward", 2)
        r = A.residual(x, b)
        rc = lvl["R"].dot(r)
        xc = vcycle(levels, li + 1, rc, repl, ri)
        x += lvl["P"].dot(xc)
        return gs.sweep(x, b, "backward", 2)
    A, dinv, omega = lvl["A"], lvl["dinv"], lvl["omega"]
    x = b * dinv
    x.local.mul_(omega)
    x = A.jacobi_smooth(x, b, dinv, omega)
    r = A.residual(x, b)
    rc = lvl["R"].dot(r)
    xc = vcycle(levels, li + 1, rc, repl, ri)
    x += lvl["P"].dot(xc)
    for _ in range(2):
        x = A.jacobi_smooth(x, b, dinv, omega)
    return x


class _GraphedVcycle:
    """hipGraph-captured V-cycle (same recipe as gmg.py)."""

    def __init__(self, levels):
        self.levels = levels
        self.repl, self.ri = build_repl_tail(levels)
        self.graph = None
        self.tried = False

    def __call__(self, r, out=None):
        import torch

        r = darray.asdistarray(r)
        from sparse.parallel import comm as _comm

        if not self.tried:
            self.tried = True
            if r.local.is_cuda and _comm.world_size() == 1 and not os.environ.get(
                    "SPARSE_NO_HIPGRAPH"):
                try:
                    self.gin = r.local.clone()
                    rin = darray.DistArray.from_local(self.gin, r.partition, r.gshape)
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        for _ in range(2):
                            vcycle(self.levels, 0, rin, self.repl, self.ri)
                    torch.cuda.current_stream().wait_stream(side)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        z = vcycle(self.levels, 0, rin, self.repl, self.ri)
                    self.graph = g
                    self.gout = z.local
                except Exception as e:
                    print(f"[amg] hipGraph capture unavailable ({e})")
                    self.graph = None
        if self.graph is not None:
            self.gin.copy_(r.local)
            self.graph.replay()
            if out is not None:
                out.local.copy_(self.gout)
                return out
            return darray.DistArray.from_local(self.gout.clone(), r.partition, r.gshape)
        z = vcycle(self.levels, 0, r, self.repl, self.ri)
        if out is not None:
            out.local.copy_(z.local.to(out.local.dtype))
            return out
        return z


def main():
    import math

    if args.smoother == "gs" and comm.world_size() > 1:
        sys.exit("amg: -smoother gs is not implemented at world size > 1 "
                 "(multicolour Gauss-Seidel runs on one GPU); use "
                 "-smoother jacobi")
    nx = int(round(args.n ** 0.5))
    A = gallery.poisson2d(nx)
    n = A.shape[0]
    b = darray.random((n,), seed=42)
    timer.start()
    levels = build_hierarchy(A, args.theta, args.max_coarse, args.smoother)
    setup_ms = timer.stop()
    op_complexity = sum(l["A"].nnz for l in levels) / levels[0]["A"].nnz

    gv = _GraphedVcycle(levels)
    M = linalg.LinearOperator((n, n), matvec=gv)
    gv(b)  # warm + capture outside the timer

    it_count = [0]
    timer.start()
    x, info = linalg.cg(A, b, M=M, tol=args.tol, maxiter=args.maxiter,
                        conv_test_iters=5,
                        callback=lambda _x: it_count.__setitem__(0, it_count[0] + 1))
    solve_ms = timer.stop()
    r = b - A.dot(x)  # collective: all ranks participate
    rn = float(r.norm().item())  # all-reduce: all ranks
    if comm.rank() == 0:
        print(f"levels={len(levels)} opcx={op_complexity:.2f} "
              f"setup={setup_ms:.1f}ms solve={solve_ms:.1f}ms iters={it_count[0]} "
              f"({it_count[0] / max(solve_ms, 1e-9) * 1000.0:.2f} iters/s) "
              f"residual={rn:.3e} info={info}")


if __name__ == "__main__":
    main()
