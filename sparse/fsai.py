"""FSAI: the factorised sparse approximate inverse (Kolotilina-Yeremin) as a
preconditioner that is applied by two SpMVs.

fsai(A) returns an FSAI object — an API superset of the reference, which has
no preconditioner — holding a sparse lower-triangular G with G A Gᴴ ≈ I;
solve applies z = Gᴴ (G r) through csr_array.dot, so both products get the
DIA / ELL / CSR mirror selection of every other SpMV and there are no levels,
no colours and no dependency between rows.

Definition.  A is square and treated as Hermitian positive definite: ONLY
entries of A on and below the diagonal are read, the upper triangle is
implied by conjugate symmetry (as in a Cholesky routine).  P is a
lower-triangular pattern containing the whole diagonal.  For row i with the
sorted columns J of P's row (the last one is i, m = |J|), S = A[J, J] (an
absent position counts as 0) and S y = e_m,

    G[i, J] = conj(y) / sqrt(y_m)

so G has a real positive diagonal, (G A)[i, j] = 0 for every j in J, j != i,
and (G A Gᴴ)[i, i] = 1.  Computed in the Cholesky form: S = C Cᴴ and
Cᴴ g = e_m give G[i, J] = conj(g).  A pivot that is not finite and > 0 is a
breakdown (a row of A without a stored diagonal breaks down by itself).

Analysis (once per structure): the pattern — tril(A^power) formed
structurally, on a copy of A whose values are all ones, through SpGEMM, or
the lower triangle of `pattern`; missing diagonal positions are added — the
rows bucketed by length into the classes of FSAI_CUTS, and the permutation
that turns G's values into those of Gᴴ stored as CSR.

Numeric phase (fsai() and refactor()): kernels/src/fsai.hip, one launch per
non-empty length class on the current stream; rows are independent.  A
breakdown is recorded on the device and read once afterwards — the only host
synchronisation of the phase.  Without a GPU the same API is backed by a
numpy loop over the rows.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import rowsched
from .darray import DistArray
from .linalg import LinearOperator

__all__ = ["FSAI", "fsai", "FSAI_MAX_ROW", "FSAI_CUTS", "FSAI_LDS_ROW"]

# Longest pattern row accepted.  The dense solve of a row costs m^3 / 6.
FSAI_MAX_ROW = 1024
# Bucket cuts: a row of m pattern entries goes to the first cut >= m and is
# solved by that many lanes with S in LDS (several rows share a wave below
# 64; at 64 a wave has one row).
FSAI_CUTS = (4, 8, 16, 64)
# Longest row solved in LDS, the same for every dtype: 64 (64 + 1) / 2 + 64
# complex128 values are 34304 B, so no workgroup goes past 64 KiB.  Rows of
# FSAI_LDS_ROW < m <= FSAI_MAX_ROW take the same algorithm on a global-memory
# workspace, one workgroup per row.
FSAI_LDS_ROW = FSAI_CUTS[-1]
# values of global workspace handed to one launch of the long-row kernel
_WORK_VALUES = 1 << 24

_NO_ROW = torch.iinfo(torch.int64).max


def _fsai_numpy(aip, aix, av, pip, pix, gv) -> int:
    """The numeric phase on the host, row by row, in the dtype of av.
    Returns the first row that breaks down, or n; that row and later broken
    ones are left unwritten."""
    n = len(pip) - 1
    bad = n
    for i in range(n):
        J = pix[pip[i]: pip[i + 1]]
        m = len(J)
        S = np.zeros((m, m), dtype=av.dtype)
        for a in range(m):
            r = J[a]
            cols = aix[aip[r]: aip[r + 1]]
            want = J[: a + 1]
            pos = np.searchsorted(cols, want)
            hit = pos < len(cols)
            hit[hit] = cols[pos[hit]] == want[hit]
            S[a, : a + 1][hit] = av[aip[r]: aip[r + 1]][pos[hit]]
        d = S.diagonal().real
        try:
            if not (np.isfinite(S).all() and (d > 0).all()):
                raise np.linalg.LinAlgError
            C = np.linalg.cholesky(S)  # reads the lower triangle only
            if not np.isfinite(C).all():
                raise np.linalg.LinAlgError
        except np.linalg.LinAlgError:
            bad = min(bad, i)
            continue
        e = np.zeros(m, dtype=av.dtype)
        e[-1] = 1
        gv[pip[i]: pip[i + 1]] = np.linalg.solve(C.conj().T, e).conj()
    return bad


def _values_rewritten(M) -> None:
    """M's value tensor was rewritten in place: drop what was built from the
    old values (the SpMV mirrors); the structure-only plans stay."""
    M._ell_cache = M._dia_cache = M._bsr_cache = M._csc_cache = None
    M._plan_cache = {k: p for k, p in M._plan_cache.items() if k[0] != "trsv"}


class FSAI(LinearOperator):
    """G with G A Gᴴ ≈ I on a lower-triangular pattern.  A LinearOperator:
    matvec(r, out=None) == solve(r, out=None) == Gᴴ (G r); Hermitian positive
    definite, so rmatvec is the same.  Not cached on the matrix."""

    def __init__(self, A, power: int = 1, pattern=None):
        A = rowsched.square_csr(A, "fsai")
        if not isinstance(power, (int, np.integer)) or power < 1:
            raise ValueError(f"power must be an int >= 1, got {power!r}")
        if pattern is not None and power != 1:
            raise ValueError("give either pattern or power, not both")
        super().__init__(A.shape, dtype=A.dtype)
        from . import kernels
        from .csr import csr_array

        n = A.shape[0]
        lc = A.local
        dev = lc.values.device
        self._gpu = lc.values.is_cuda
        if self._gpu:
            kernels.require()
        self._a_indptr = lc.indptr.to(torch.int64).contiguous()
        self._a_indices = lc.indices.contiguous()

        # 1. the pattern P: lower triangle of the source structure + diagonal
        if pattern is not None:
            src = rowsched.as_csr(pattern)
            if tuple(src.shape) != tuple(A.shape):
                raise ValueError(
                    f"pattern has shape {src.shape}, A has {A.shape}")
        else:
            src = A
            if power > 1:
                ones = csr_array.from_local(
                    lc.indptr, lc.indices,
                    torch.ones(lc.values.numel(), dtype=torch.float64,
                               device=dev), A.partition, A.shape)
                src = ones
                for _ in range(power - 1):
                    src = src.dot(ones)
        idt = self._a_indices.dtype
        sip = src._indptr.to(torch.int64).to(dev)
        cols = src._indices.to(dev).long()
        _, rows = rowsched.row_index(sip)
        keep = cols <= rows
        rows, cols = rows[keep], cols[keep]
        if n and int((cols == rows).sum().item()) != n:  # add the diagonal
            ar = torch.arange(n, dtype=torch.int64, device=dev)
            key = torch.unique(torch.cat([rows * n + cols, ar * n + ar]))
            rows = torch.div(key, n, rounding_mode="floor")
            cols = key - rows * n
        m = torch.bincount(rows, minlength=n)
        self._indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(m, 0, out=self._indptr[1:])
        self._indices = cols.to(idt).contiguous()

        # 2. rows by length class (one host read for the longest row, one per
        # class for its size)
        self.max_row = 0
        self._classes: List[Tuple[int, torch.Tensor, int]] = []
        if n:
            longest, where = (int(v) for v in
                              torch.stack(m.max(0)).tolist())
            if longest > FSAI_MAX_ROW:
                raise ValueError(
                    f"fsai: row {where} of the pattern has {longest} "
                    f"entries, more than FSAI_MAX_ROW = {FSAI_MAX_ROW}; use "
                    "a thinner pattern (a lower power, or pattern=)")
            self.max_row = longest
            lo = 0
            for cut in FSAI_CUTS + (FSAI_MAX_ROW,):
                if lo >= longest:
                    break
                rl = ((m > lo) & (m <= cut)).nonzero(as_tuple=False).flatten()
                if rl.numel():
                    lanes = cut if cut <= FSAI_LDS_ROW else 0
                    self._classes.append((lanes, rl.contiguous(),
                                          min(cut, longest)))
                lo = cut

        # 3. Gᴴ as CSR: values of G permuted, conjugated
        self._perm = torch.sort(cols * n + rows).indices
        hip = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(cols, minlength=n), 0, out=hip[1:])
        self._gvals = torch.zeros(cols.numel(), dtype=lc.values.dtype,
                                  device=dev)
        self._ghvals = torch.zeros_like(self._gvals)
        self.G = csr_array.from_local(self._indptr, self._indices,
                                      self._gvals, A.partition, A.shape)
        self.GH = csr_array.from_local(
            hip, rows[self._perm].to(idt).contiguous(), self._ghvals,
            A.partition, A.shape)
        self._tmp: Dict[tuple, DistArray] = {}

        # 4. numeric phase
        self._factor(lc.values)

    # -- numeric phase --------------------------------------------------------
    def _factor(self, values: torch.Tensor) -> None:
        from . import kernels

        n = self.shape[0]
        gv = self._gvals
        flag = torch.full((1,), _NO_ROW, dtype=torch.int64, device=gv.device)
        if self._gpu:
            kernels.fsai_factor(self, values.contiguous(), gv, flag)
        else:
            flag[0] = _fsai_numpy(
                self._a_indptr.numpy(), self._a_indices.numpy(),
                values.numpy(), self._indptr.numpy(), self._indices.numpy(),
                gv.numpy())
        torch.index_select(gv, 0, self._perm, out=self._ghvals)
        if self._ghvals.is_complex():
            self._ghvals.conj_physical_()
        _values_rewritten(self.G)
        _values_rewritten(self.GH)
        bad = int(flag.item())  # the one host read of the phase
        if bad < n:
            raise np.linalg.LinAlgError(
                f"FSAI breakdown: the pattern block of row {bad} is not "
                "positive definite (pivot not finite and > 0)")

    def refactor(self, A) -> "FSAI":
        """New values on the SAME structure of A: numeric phase only; G and GH
        keep their index arrays.  After a LinAlgError the operator is
        unusable until the next successful refactor."""
        A = rowsched.as_csr(A)
        if tuple(A.shape) != self.shape:
            raise ValueError(
                f"refactor: shape {A.shape} differs from {self.shape}")
        lc = A.local
        if lc.values.dtype != self._gvals.dtype:
            raise ValueError(
                f"refactor: dtype {A.dtype} differs from {self.dtype}")
        if not (rowsched.same_structure(lc.indptr, self._a_indptr)
                and rowsched.same_structure(lc.indices, self._a_indices)):
            raise ValueError(
                "refactor: the matrix does not have the factorised "
                "structure (indptr / indices differ)")
        self._factor(lc.values)
        return self

    # -- read-only results ----------------------------------------------------
    @property
    def nnz(self) -> int:
        """Stored entries of G (those of the pattern)."""
        return int(self._gvals.numel())

    @property
    def row_classes(self) -> List[Tuple[int, int]]:
        """(lanes per row, rows) per launch of the numeric phase; lanes 0 is
        the global-workspace route for rows longer than FSAI_LDS_ROW."""
        return [(lanes, int(rl.numel())) for lanes, rl, _ in self._classes]

    # -- apply ----------------------------------------------------------------
    def solve(self, r, out: Optional[DistArray] = None) -> DistArray:
        """z = Gᴴ (G r) for r of shape (n,) or (n, k).  out may alias r."""
        b = rowsched.as_rhs(r, self.shape[0], "r")
        tdt = self.G._out_dtype(b.local.dtype)
        key = (tuple(b.local.shape), tdt, b.local.device)
        t = self._tmp.get(key)
        if t is None:
            t = self._tmp[key] = DistArray.from_local(
                torch.empty(b.local.shape, dtype=tdt, device=b.local.device),
                b.partition, b.shape)
        self.G.dot(b, out=t)
        return self.GH.dot(t, out=out)

    def matvec(self, r, out=None):
        return self.solve(r, out=out)

    def rmatvec(self, r, out=None):
        return self.solve(r, out=out)


def fsai(A, power: int = 1, pattern=None) -> FSAI:
    """Factorised sparse approximate inverse of the Hermitian positive
    definite sparse matrix A (its lower triangle is read) as a LinearOperator
    for use as M in the Krylov solvers.  The pattern of G is that of
    tril(A^power), or the lower triangle of `pattern` (values ignored); the
    diagonal is always part of it."""
    return FSAI(A, power=power, pattern=pattern)
