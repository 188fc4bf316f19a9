"""Sparse triangular solves by level scheduling.

scipy.sparse.linalg.spsolve_triangular surface plus a reusable analysis
object (TriangularSolver) and the symmetric Gauss-Seidel preconditioner built
from two of them — an API superset of the reference, which has no triangular
solve.

Analysis (once per matrix and triangle): the selected triangle of A is split
into a strict-triangle CSR and a diagonal vector; one sequential O(nnz) host
pass gives every row its dependency level (0 without strict entries, else
1 + the maximum over its strict columns); rows sorted by (level, row) form
`order`, cut at `level_ptr`.  The host-side schedule groups the levels: a
maximal run of consecutive levels of at most TRSV_CHAIN_WIDTH rows each is one
"chain" segment (one launch of a single workgroup that steps through the
levels with a barrier), every other level is its own "wide" segment (one
launch).  Solving enqueues the schedule on the current stream and never
synchronises with the host (kernels/src/relax.hip).  The steps shared with
ILU(0) and the multicolour sweeps are in sparse/rowsched.py.

Semantics: only the selected triangle is read (so SGS can use A itself);
duplicate stored entries add up, on the diagonal too; unit_diagonal ignores
stored diagonal entries; otherwise a missing or zero diagonal raises
numpy.linalg.LinAlgError at analysis.  Without a GPU the same API is backed by
scipy's spsolve_triangular on the explicitly extracted triangle.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import rowsched
from .darray import DistArray
from .linalg import LinearOperator
from .rowsched import as_csr, single_rank
from .types import common_value_dtype, to_numpy_dtype
from .utils import perf_warning

__all__ = ["TRSV_CHAIN_WIDTH", "TriangularSolver", "spsolve_triangular",
           "sgs_preconditioner"]

# levels of at most this many rows are stepped through inside one workgroup;
# wider ones get a launch of their own
TRSV_CHAIN_WIDTH = 1024


def _levels_numpy(indptr: np.ndarray, indices: np.ndarray,
                  lower: bool) -> np.ndarray:
    """The level pass without the extension (same walk as trsv_levels)."""
    n = len(indptr) - 1
    lv = np.zeros(n, dtype=np.int64)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        s, e = indptr[i], indptr[i + 1]
        if e > s:
            lv[i] = lv[indices[s:e]].max() + 1
    return lv


def _row_group(mean_len: float) -> int:
    """Lanes per row of a wide level, from its mean strict row length."""
    return 1 if mean_len <= 4 else 8 if mean_len <= 32 else 64


class TriangularSolver(LinearOperator):
    """Analysis of one triangle of A, reusable over right-hand sides.

    A LinearOperator: matvec(b, out=None) == solve(b, out=None) == T⁻¹ b
    for the lower (or upper) triangle T of A."""

    def __init__(self, A, lower: bool = True, unit_diagonal: bool = False):
        A = rowsched.square_csr(A, "TriangularSolver")
        n = A.shape[0]
        super().__init__(A.shape, dtype=A.dtype)
        self.lower = bool(lower)
        self.unit_diagonal = bool(unit_diagonal)
        lc = A.local
        dev = lc.device
        from . import kernels

        self._gpu = lc.values.is_cuda
        if self._gpu:
            kernels.require()

        # 1. split the triangle: strict CSR (original row order) + diagonal
        _, rows = rowsched.row_index(lc.indptr)
        cols = lc.indices.long()
        if unit_diagonal:
            diag = torch.ones(n, dtype=lc.values.dtype, device=dev)
        else:  # one device reduction, one host read
            diag = rowsched.summed_diagonal(cols == rows, rows, lc.values, n)
        strict = cols < rows if lower else cols > rows
        self._indices = lc.indices[strict].contiguous()
        self._values = lc.values[strict].contiguous()
        self._diag = diag
        self._indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n:
            torch.cumsum(torch.bincount(rows[strict], minlength=n), 0,
                         out=self._indptr[1:])
        self._cast = {}  # value dtype -> (values, diag) for a wider b

        # 2. levels: one sequential pass over a host copy of the structure
        ip_h = self._indptr.cpu()
        ix_h = self._indices.cpu()
        if kernels.ext() is not None:
            levels = kernels.trsv_levels(ip_h, ix_h, self.lower)
        else:
            levels = torch.from_numpy(
                _levels_numpy(ip_h.numpy(), ix_h.numpy(), self.lower))
        self._levels = levels

        # 3. row order by (level, row), level boundaries, schedule
        cl = self._classes = rowsched.RowClasses(levels, dev)
        self._nlevels = cl.nclasses
        self._order = cl.order
        self._level_ptr = cl.ptr
        self._seg = rowsched.chain_segments(np.diff(cl.ptr_host),
                                            TRSV_CHAIN_WIDTH)
        level_nnz = cl.sums(self._indptr[1:] - self._indptr[:-1])
        self._sched = rowsched.schedule_rows(cl.ptr_host, level_nnz,
                                             self._seg, _row_group)

        # 4. inherently sequential structure
        if self._nlevels > n / 32:
            perf_warning(
                f"triangular solve: {self._nlevels} dependency levels for "
                f"{n} rows — this structure is inherently sequential")

    # -- read-only analysis results -------------------------------------------
    @property
    def levels(self) -> torch.Tensor:
        """Per-row dependency level (int64, on the host)."""
        return self._levels

    @property
    def nlevels(self) -> int:
        return self._nlevels

    @property
    def schedule(self) -> List[Tuple[str, int, int]]:
        """(kind, level_lo, level_hi) per launch, kind "wide" or "chain"."""
        chain, starts, ends = self._seg
        return [("chain" if c else "wide", int(lo), int(hi))
                for c, lo, hi in zip(chain, starts, ends)]

    def _set_values(self, values: torch.Tensor,
                    diag: Optional[torch.Tensor] = None) -> None:
        """New strict-triangle values (and diagonal) on the unchanged
        structure, copied into the solver's own arrays; the analysis stays
        (ILU0.refactor in sparse/ilu.py)."""
        self._values.copy_(values)
        if diag is not None:
            self._diag.copy_(diag)
        self._cast.clear()

    # -- solve ----------------------------------------------------------------
    def solve(self, b, out: Optional[DistArray] = None) -> DistArray:
        """x = T⁻¹ b for b of shape (n,) or (n, k).  out may alias b."""
        b = rowsched.as_rhs(b, self.shape[0], "b")
        tdt = common_value_dtype(self._values.dtype, b.local.dtype)
        x, direct = rowsched.result_buffer(b, out, tdt)
        if self._gpu:
            from . import kernels

            vals, diag = rowsched.cast_operands(self._cast, self._values,
                                                self._diag, tdt)
            kernels.trsv_solve(self, vals, diag,
                               b.local.to(tdt).contiguous(), x)
        else:
            x.copy_(self._solve_host(b.local, tdt))
        return rowsched.finish_result(x, direct, b, out)

    def matvec(self, b, out=None):
        return self.solve(b, out=out)

    def _solve_host(self, b: torch.Tensor, tdt) -> torch.Tensor:
        import scipy.sparse as sps
        from scipy.sparse.linalg import spsolve_triangular as sp_solve

        n = self.shape[0]
        if n == 0 or b.numel() == 0:
            return torch.empty(b.shape, dtype=tdt)
        ndt = to_numpy_dtype(tdt)
        ip = self._indptr.numpy()
        rows = np.repeat(np.arange(n), np.diff(ip))
        ar = np.arange(n)
        # the explicitly extracted triangle; coo -> csr sums duplicates
        T = sps.csr_matrix(
            (np.concatenate([self._values.numpy().astype(ndt),
                             self._diag.numpy().astype(ndt)]),
             (np.concatenate([rows, ar]),
              np.concatenate([self._indices.numpy().astype(np.int64), ar]))),
            shape=(n, n))
        x = sp_solve(T, b.numpy().astype(ndt), lower=self.lower,
                     unit_diagonal=self.unit_diagonal)
        return torch.from_numpy(np.ascontiguousarray(x)).to(tdt)


def spsolve_triangular(A, b, lower=True, overwrite_A=False, overwrite_b=False,
                       unit_diagonal=False) -> DistArray:
    """Solve A x = b for a triangular A (scipy.sparse.linalg signature).

    Only the selected triangle of A is read.  The analysis is cached on the
    matrix and dropped when its values change.  overwrite_b solves in place
    when b is a DistArray of the result dtype; overwrite_A is accepted for
    scipy compatibility (A is never modified)."""
    single_rank("spsolve_triangular")
    A = as_csr(A)
    key = ("trsv", bool(lower), bool(unit_diagonal))
    solver = A._plan_cache.get(key)
    if solver is None:
        solver = TriangularSolver(A, lower=lower, unit_diagonal=unit_diagonal)
        A._plan_cache[key] = solver
    out = None
    if overwrite_b and isinstance(b, DistArray) and b.tdtype == \
            common_value_dtype(solver._values.dtype, b.tdtype):
        out = b  # solve() writes straight into it
    return solver.solve(b, out=out)


class _SGSOperator(LinearOperator):
    """z = (D+U)⁻¹ D (D+L)⁻¹ r, the inverse of M = (D+L) D⁻¹ (D+U)."""

    def __init__(self, A):
        A = as_csr(A)
        self._L = TriangularSolver(A, lower=True)
        self._U = TriangularSolver(A, lower=False)
        super().__init__(A.shape, dtype=A.dtype)

    def matvec(self, r, out=None):
        z = self._L.solve(r, out=out)
        d = self._L._diag
        z.local.mul_(d if z.ndim == 1 else d.unsqueeze(1))
        return self._U.solve(z, out=z)

    rmatvec = matvec


def sgs_preconditioner(A, ordering: str = "natural",
                       seed: int = 0) -> LinearOperator:
    """Symmetric Gauss-Seidel preconditioner of A as a LinearOperator.

    ordering="natural": two triangular solves over A itself and one diagonal
    scale, in the row order of A.  ordering="multicolor": the same
    preconditioner in the order of a greedy colouring of A (seed as in
    greedy_coloring), one launch per colour and direction — a
    gauss_seidel.MulticolorGaussSeidel."""
    single_rank("sgs_preconditioner")
    if ordering == "natural":
        return _SGSOperator(A)
    if ordering == "multicolor":
        from .gauss_seidel import MulticolorGaussSeidel

        return MulticolorGaussSeidel(A, seed=seed)
    raise ValueError(
        f"ordering must be 'natural' or 'multicolor', got {ordering!r}")
