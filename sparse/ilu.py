"""ILU(0): incomplete LU factorisation without fill, as a preconditioner.

ilu0(A) returns an ILU0 object — an API superset of the reference, which has
no factorisation — whose solve applies U⁻¹ L⁻¹ through two level-scheduled
TriangularSolvers (sparse/trisolve.py).  L (unit lower) and U (upper) live on
the pattern of A and (L @ U)[i, j] == A[i, j] on every stored position of A;
no pivoting, no conjugation, stored zeros are part of the pattern.

Analysis (once per structure): one device reduction checks that the rows are
column-sorted, duplicate-free and carry a stored diagonal (its positions are
diag_ptr); the dependency levels of a row-wise ILU(0) are exactly those of
the strict lower triangle of the pattern, so the factorisation runs over the
level analysis of the L solver (its order / level_ptr and the same chain cut;
only the lanes per row are chosen from the full row length).

Numeric phase (ilu0() and refactor()): the factor is computed in place in a
copy of A's values by kernels/src/ilu0.hip, one launch per schedule segment
on the current stream; a pivot that becomes exactly zero is recorded on the
device and read once afterwards — the only host synchronisation of the
phase.  The two solvers then get the new values; nothing is re-analysed.
Without a GPU the same API is backed by the extension's sequential CPU op, or
by numpy when the extension is not built.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import rowsched
from .darray import DistArray
from .linalg import LinearOperator
from .trisolve import TriangularSolver

__all__ = ["ILU0", "ilu0"]

_NO_PIVOT_ROW = torch.iinfo(torch.int64).max


def _ilu0_group(mean_len: float) -> int:
    """Lanes per row, from the mean FULL row length of a segment: a lane
    owns every G-th entry of the row, so rows of a handful of entries (a
    stencil) stay with one lane."""
    return 1 if mean_len <= 8 else 8 if mean_len <= 64 else 64


def _ilu0_numpy(ip: np.ndarray, ix: np.ndarray, v: np.ndarray,
                dp: np.ndarray) -> int:
    """Sequential IKJ ILU(0) in place in v without the extension (same walk
    as the ilu0_factor CPU op).  Returns the first row with a zero pivot, or
    n."""
    n = len(ip) - 1
    bad = n
    with np.errstate(all="ignore"):
        for i in range(n):
            pe = ip[i + 1]
            for q in range(ip[i], dp[i]):
                k = ix[q]
                m = v[q] / v[dp[k]]
                v[q] = m
                kcols = ix[dp[k] + 1: ip[k + 1]]
                icols = ix[q + 1: pe]
                if len(kcols) and len(icols):
                    pos = np.searchsorted(icols, kcols)
                    hit = pos < len(icols)
                    hit[hit] = icols[pos[hit]] == kcols[hit]
                    v[q + 1 + pos[hit]] -= m * v[dp[k] + 1: ip[k + 1]][hit]
            if bad == n and v[dp[i]] == 0:
                bad = i
    return bad


class ILU0(LinearOperator):
    """ILU(0) factors of A.  A LinearOperator: matvec(r, out=None) ==
    solve(r, out=None) == U⁻¹ L⁻¹ r.  Not cached on the matrix."""

    def __init__(self, A):
        A = rowsched.square_csr(A, "ilu0")
        super().__init__(A.shape, dtype=A.dtype)
        n = A.shape[0]
        lc = A.local
        from . import kernels

        self._gpu = lc.values.is_cuda
        if self._gpu:
            kernels.require()
        self._partition = A.partition
        self._indptr = lc.indptr.to(torch.int64).contiguous()
        self._indices = lc.indices.contiguous()

        # 1. structure: sorted duplicate-free rows with a stored diagonal
        counts, rows = rowsched.row_index(self._indptr)
        cols = self._indices.long()
        unsorted = ((cols < 0) | (cols >= n)).any()
        if cols.numel() > 1:
            unsorted = unsorted | ((rows[1:] == rows[:-1])
                                   & (cols[1:] <= cols[:-1])).any()
        on = cols == rows
        missing = (torch.bincount(rows[on], minlength=n) != 1).any()
        # one device reduction, one host read
        unsorted, missing = torch.stack([unsorted, missing]).tolist()
        if unsorted:
            raise ValueError(
                "ilu0 needs column-sorted, duplicate-free rows with columns "
                "inside the matrix")
        if missing:
            raise np.linalg.LinAlgError(
                "ILU(0) does not exist: a row has no stored diagonal entry")
        self._diag_ptr = on.nonzero(as_tuple=False).flatten()
        self._lpos = (cols < rows).nonzero(as_tuple=False).flatten()
        self._upos = (cols > rows).nonzero(as_tuple=False).flatten()

        # 2. levels: the L solver's analysis (the only lower level pass);
        # its values are replaced by the factor's below
        self._Ls = TriangularSolver(A, lower=True, unit_diagonal=True)
        self._Us: Optional[TriangularSolver] = None
        ls = self._Ls

        # 3. the same segments with lanes per row from the full row length
        cl = ls._classes
        self._sched = rowsched.schedule_rows(
            cl.ptr_host, cl.sums(counts), ls._seg, _ilu0_group,
            chain_group=_ilu0_group)

        # 4. numeric phase
        self._fvals = torch.empty_like(lc.values)
        self._L = self._U = None
        self._factor(lc.values)

    # -- numeric phase --------------------------------------------------------
    def _factor(self, values: torch.Tensor) -> None:
        from . import kernels

        n = self.shape[0]
        fv = self._fvals
        fv.copy_(values)
        flag = torch.full((1,), _NO_PIVOT_ROW, dtype=torch.int64,
                          device=fv.device)
        if kernels.ext() is not None:
            kernels.ilu0_factor(self, fv, flag)
        else:
            flag[0] = _ilu0_numpy(self._indptr.numpy(), self._indices.numpy(),
                                  fv.numpy(), self._diag_ptr.numpy())
        self._L = self._U = None
        self._Ls._set_values(fv[self._lpos])
        if self._Us is not None:
            self._Us._set_values(fv[self._upos], fv[self._diag_ptr])
        bad = int(flag.item())  # the one host read of the phase
        if bad < n:
            raise np.linalg.LinAlgError(
                f"ILU(0) breakdown: zero pivot in row {bad}")
        if self._Us is None:  # first factorisation: analyse U's triangle
            from .csr import csr_array

            self._Us = TriangularSolver(
                csr_array.from_local(self._indptr, self._indices, fv,
                                     self._partition, self.shape),
                lower=False)

    def refactor(self, A) -> "ILU0":
        """New values on the SAME structure: numeric phase only.  After a
        LinAlgError (zero pivot) the factors are unusable until the next
        successful refactor."""
        A = rowsched.as_csr(A)
        if tuple(A.shape) != self.shape:
            raise ValueError(
                f"refactor: shape {A.shape} differs from {self.shape}")
        lc = A.local
        if lc.values.dtype != self._fvals.dtype:
            raise ValueError(
                f"refactor: dtype {A.dtype} differs from {self.dtype}")
        if not (rowsched.same_structure(lc.indptr, self._indptr)
                and rowsched.same_structure(lc.indices, self._indices)):
            raise ValueError(
                "refactor: the matrix does not have the factorised "
                "structure (indptr / indices differ)")
        self._factor(lc.values)
        return self

    # -- read-only results ----------------------------------------------------
    @property
    def nnz(self) -> int:
        """Stored entries of the factor (those of A's pattern)."""
        return int(self._fvals.numel())

    @property
    def nlevels(self) -> int:
        return self._Ls.nlevels

    @property
    def schedule(self) -> List[Tuple[str, int, int]]:
        """(kind, level_lo, level_hi) per launch of the factorisation, kind
        "wide" or "chain" — the L solver's segments."""
        return self._Ls.schedule

    def _triangle(self, lower: bool):
        from .csr import csr_array

        n = self.shape[0]
        strict = self._lpos if lower else self._upos
        pos = torch.sort(torch.cat([strict, self._diag_ptr])).values
        vals = self._fvals
        if lower:
            vals = vals.clone()
            vals[self._diag_ptr] = 1
        indptr = torch.zeros(n + 1, dtype=torch.int64,
                             device=self._indptr.device)
        counts = (self._diag_ptr - self._indptr[:-1] + 1 if lower
                  else self._indptr[1:] - self._diag_ptr)
        torch.cumsum(counts, 0, out=indptr[1:])
        return csr_array.from_local(indptr, self._indices[pos].contiguous(),
                                    vals[pos].contiguous(), self._partition,
                                    self.shape)

    @property
    def L(self):
        """Unit lower factor as a csr_array (diagonal stored as 1)."""
        if self._L is None:
            self._L = self._triangle(True)
        return self._L

    @property
    def U(self):
        """Upper factor as a csr_array, diagonal included."""
        if self._U is None:
            self._U = self._triangle(False)
        return self._U

    # -- apply ----------------------------------------------------------------
    def solve(self, r, out: Optional[DistArray] = None) -> DistArray:
        """z = U⁻¹ L⁻¹ r for r of shape (n,) or (n, k).  out may alias r."""
        z = self._Ls.solve(r, out=out)
        return self._Us.solve(z, out=z)

    def matvec(self, r, out=None):
        return self.solve(r, out=out)

    def rmatvec(self, r, out=None):
        raise NotImplementedError(
            "ILU0 has no rmatvec: transposed triangular solves are not "
            "implemented")


def ilu0(A) -> ILU0:
    """ILU(0) factorisation of the square sparse matrix A (no pivoting, no
    fill) as a LinearOperator for use as M in the Krylov solvers."""
    return ILU0(A)
