"""Multicolour Gauss-Seidel: graph colouring and colour-ordered sweeps.

greedy_coloring(A) colours the rows of a square matrix so that no stored
off-diagonal entry of A or Aᵀ joins two rows of one colour, and
MulticolorGaussSeidel(A) sweeps colour by colour: rows of one colour do not
depend on each other, so a Gauss-Seidel sweep is one launch per colour
instead of one per dependency level of the natural row order
(sparse/trisolve.py).  An API superset of the reference, which has neither.

Colouring.  The graph has one vertex per row and an edge {i, j}, i != j,
where A[i, j] or A[j, i] is stored (stored zeros count).  Vertex i has the
priority (h(i), i) with the 32-bit hash h of _hash32, and the result is
defined as what sequential greedy gives when it visits the vertices by
decreasing priority, each taking the smallest colour none of its coloured
neighbours has.  On the GPU this runs as Jones-Plassmann rounds
(kernels/src/color.hip), one launch and one host read of the remaining count
per round over a compacted list of uncoloured rows; without one, as the
extension's sequential CPU op, or in numpy when the extension is not built.
All three give the same colours.  A pattern that is not structurally
symmetric is symmetrised on the device first; a column-sorted duplicate-free
symmetric pattern is detected with one reduction and used as it is.

Sweeps.  The analysis extracts the diagonal (the sum of the stored diagonal
entries of a row; a missing or zero one raises numpy.linalg.LinAlgError),
sorts the rows by (colour, row) into `order`, cut at `color_ptr`, and picks
the lanes per row of each colour from its mean row length.  A caller's
colouring (colors=) is validated on the device: this is what makes the
in-place sweeps race-free.  The matrix arrays are referenced, not copied; the
diagonal is extracted once, so a matrix whose values change needs a new
object (the colouring can be passed back in).  sweep() enqueues one launch
per colour on the current stream (kernels/src/relax.hip) and never
synchronises with the host.  The steps shared with the triangular solve and
ILU(0) are in sparse/rowsched.py.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import rowsched
from .darray import DistArray, asdistarray
from .linalg import LinearOperator
from .trisolve import _row_group
from .types import common_value_dtype, to_numpy_dtype

__all__ = ["MulticolorGaussSeidel", "greedy_coloring"]

_DIRECTIONS = ("forward", "backward", "symmetric")


def _hash32(i: np.ndarray, seed: int) -> np.ndarray:
    """h(i) in 32-bit unsigned arithmetic (the same steps as color.hip)."""
    x = np.asarray(i).astype(np.uint32) ^ np.uint32(seed & 0xFFFFFFFF)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def _greedy_numpy(indptr: np.ndarray, indices: np.ndarray,
                  seed: int) -> np.ndarray:
    """Sequential greedy in priority order without the extension (same walk
    as the color_greedy CPU op) on a structurally symmetric pattern."""
    n = len(indptr) - 1
    ar = np.arange(n, dtype=np.int64)
    visit = np.lexsort((ar, _hash32(ar, seed)))[::-1]
    colors = np.full(n, -1, dtype=np.int32)
    for i in visit:
        nb = indices[indptr[i]: indptr[i + 1]]
        c = colors[nb]
        c = c[(nb != i) & (c >= 0)]
        taken = np.zeros(len(c) + 1, dtype=bool)  # a free one among 0..len(c)
        taken[c[c <= len(c)]] = True
        colors[i] = int(np.argmin(taken))
    return colors


def _graph(A) -> Tuple[torch.Tensor, torch.Tensor]:
    """(indptr, indices) of a structurally symmetric pattern holding the
    graph of A: A's own arrays when its pattern is column-sorted,
    duplicate-free and symmetric (one device reduction, one host read), else
    the pattern of A ∪ Aᵀ without the diagonal, built on the device."""
    lc = A.local
    n = A.shape[0]
    dev = lc.values.device
    indptr = lc.indptr.to(torch.int64).contiguous()
    indices = lc.indices.contiguous()
    _, rows = rowsched.row_index(indptr)
    cols = indices.long()
    outside = ((cols < 0) | (cols >= n)).any()
    off = rows != cols
    key = rows[off] * n + cols[off]
    key_t = cols[off] * n + rows[off]
    if key.numel():
        canonical = (key[1:] > key[:-1]).all()
        # the transposed entries looked up in the (then sorted) entries
        pos = torch.searchsorted(key, key_t).clamp_(max=key.numel() - 1)
        symmetric = (key[pos] == key_t).all()
    else:
        canonical = symmetric = torch.ones((), dtype=torch.bool, device=dev)
    outside, canonical, symmetric = torch.stack(
        [outside, canonical, symmetric]).tolist()
    if outside:
        raise ValueError("A has column indices outside the matrix")
    if canonical and symmetric:
        return indptr, indices
    both = torch.unique(torch.cat([key, key_t]))  # sorted, duplicate-free
    r = torch.div(both, n, rounding_mode="floor")
    sym_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(r, minlength=n), 0, out=sym_ptr[1:])
    return sym_ptr, (both - r * n).to(indices.dtype)


def _greedy_coloring(A, seed: int) -> Tuple[torch.Tensor, Optional[int]]:
    """(colours, Jones-Plassmann rounds or None on the host path)."""
    n = A.shape[0]
    dev = A.local.values.device
    from . import kernels

    if n == 0:
        return torch.zeros(0, dtype=torch.int32, device=dev), 0
    indptr, indices = _graph(A)
    if not A.local.values.is_cuda:
        ip_h, ix_h = indptr.cpu(), indices.cpu()
        if kernels.ext() is not None:
            return kernels.color_greedy(ip_h, ix_h, seed).to(dev), None
        return torch.from_numpy(
            _greedy_numpy(ip_h.numpy(), ix_h.numpy(), seed)).to(dev), None
    kernels.require()
    colors = torch.full((n,), -1, dtype=torch.int32, device=dev)
    work = torch.arange(n, dtype=torch.int64, device=dev)
    rest = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    nwork, rounds = n, 0
    while nwork:
        # every round colours at least the highest-priority uncoloured row
        if rounds >= n:
            raise RuntimeError(
                f"greedy_coloring: {nwork} rows still uncoloured after {n} "
                "rounds")
        count.zero_()
        kernels.color_round(indptr, indices, work, nwork, seed, colors, rest,
                            count)
        left = int(count.item())  # the one host read of the round
        if left >= nwork:
            raise RuntimeError("greedy_coloring: a round coloured no row")
        nwork, rounds = left, rounds + 1
        work, rest = rest, work
    return colors, rounds


def greedy_coloring(A, seed: int = 0) -> torch.Tensor:
    """Colours 0..C-1 of the rows of the square matrix A as an int32 tensor
    on A's device: the greedy colouring in decreasing (h(i), i) priority of
    the graph of A ∪ Aᵀ (module docstring)."""
    A = rowsched.square_csr(A, "greedy_coloring")
    return _greedy_coloring(A, int(seed))[0]


class MulticolorGaussSeidel(LinearOperator):
    """Colour-ordered Gauss-Seidel sweeps over A, reusable over right-hand
    sides.

    A LinearOperator: matvec(r, out=None) is one symmetric sweep from zero,
    (D+U)⁻¹ D (D+L)⁻¹ r with the triangles taken in the colour ordering —
    the multicolour symmetric Gauss-Seidel preconditioner."""

    def __init__(self, A, colors=None, seed: int = 0):
        A = rowsched.square_csr(A, "MulticolorGaussSeidel")
        n = A.shape[0]
        super().__init__(A.shape, dtype=A.dtype)
        lc = A.local
        dev = lc.values.device
        from . import kernels

        self._gpu = lc.values.is_cuda
        if self._gpu:
            kernels.require()
        self._partition = A.partition
        # the matrix arrays are referenced, not copied
        self._indptr = lc.indptr.to(torch.int64).contiguous()
        self._indices = lc.indices.contiguous()
        self._values = lc.values.contiguous()

        # 1. diagonal: the sum of the stored diagonal entries of each row
        counts, rows = rowsched.row_index(self._indptr)
        cols = self._indices.long()
        on = cols == rows
        # one device reduction, one host read: the columns ride with the
        # diagonal's check (the sweeps index x with the columns unchecked)
        outside = ((cols < 0) | (cols >= n)).any()
        self._diag = rowsched.summed_diagonal(
            on, rows, self._values, n, first=[(outside, ValueError(
                "A has column indices outside the matrix"))])
        self._cast = {}  # value dtype -> (values, diag) for a wider x
        self._host = {}  # numpy dtype -> per-colour scipy operands

        # 2. colours: greedy, or the caller's after validation
        self._rounds: Optional[int] = None
        if colors is None:
            col, self._rounds = _greedy_coloring(A, int(seed))
        else:
            if isinstance(colors, DistArray):
                colors = colors.local
            if not isinstance(colors, torch.Tensor):
                colors = torch.as_tensor(np.asarray(colors))
            if colors.shape != (n,) or colors.is_floating_point() \
                    or colors.is_complex():
                raise ValueError(
                    f"colors must be {n} integers, one per row of A")
            wide = colors.to(dev).long()
            bad = (wide < 0).any() | (wide >= 2**31 - 1).any()
            off = ~on
            clash = (wide[rows[off]] == wide[cols[off]]).any() \
                if n else bad
            bad, clash = torch.stack([bad, clash]).tolist()
            if bad:
                raise ValueError("colors must be non-negative int32 values")
            if clash:
                raise ValueError(
                    "improper colouring: a stored off-diagonal entry joins "
                    "two rows of one colour")
            col = wide.to(torch.int32)
        self._colors = col.contiguous()

        # 3. rows by (colour, row), class boundaries, lanes per row
        cl = self._classes = rowsched.RowClasses(self._colors, dev)
        self._order = cl.order
        self._ncolors = cl.nclasses
        self._color_ptr = cl.ptr
        self._sched = rowsched.schedule_rows(
            cl.ptr_host, cl.sums(counts),
            rowsched.plain_segments(cl.nclasses), _row_group)

    # -- read-only analysis results -------------------------------------------
    @property
    def colors(self) -> torch.Tensor:
        """Colour of every row (int32, on A's device)."""
        return self._colors

    @property
    def ncolors(self) -> int:
        return self._ncolors

    @property
    def order(self) -> torch.Tensor:
        """Rows sorted by (colour, row); int32 when n fits."""
        return self._order

    @property
    def color_ptr(self) -> torch.Tensor:
        """Class boundaries in `order` (int64, ncolors + 1)."""
        return self._color_ptr

    # -- sweeps ---------------------------------------------------------------
    def sweep(self, x, b, direction: str = "forward",
              iterations: int = 1) -> DistArray:
        """Gauss-Seidel sweeps in place in x, which is returned: for every
        colour, ascending ("forward") or descending ("backward"), each row i
        of the colour gets x[i] = (b[i] - sum_{j != i} a_ij x[j]) / a_ii;
        "symmetric" is a forward sweep followed by a backward one.  x and b
        have shape (n,) or (n, k); x is a DistArray of the result dtype."""
        if direction not in _DIRECTIONS:
            raise ValueError(
                f"direction must be one of {_DIRECTIONS}, got {direction!r}")
        if not isinstance(x, DistArray):
            raise TypeError("x must be a DistArray: the sweep works in place")
        b = asdistarray(b)
        n = self.shape[0]
        if x.ndim not in (1, 2) or x.shape[0] != n or b.shape != x.shape:
            raise ValueError(
                f"x has shape {x.shape} and b {b.shape}, expected both "
                f"({n},) or ({n}, k)")
        tdt = x.local.dtype
        if common_value_dtype(self._values.dtype, b.local.dtype, tdt) != tdt:
            raise ValueError(
                f"x of dtype {x.dtype} cannot hold the result of a sweep "
                f"with A of dtype {self.dtype} and b of dtype {b.dtype}")
        if not x.local.is_contiguous():
            raise ValueError("x must be contiguous: the sweep works in place")
        self._sweep_local(x.local, b.local.to(tdt).contiguous(), direction,
                          int(iterations))
        return x

    def _sweep_local(self, x: torch.Tensor, b: torch.Tensor, direction: str,
                     iterations: int) -> None:
        passes = {"forward": (False,), "backward": (True,),
                  "symmetric": (False, True)}[direction]
        if self._gpu:
            from . import kernels

            vals, diag = rowsched.cast_operands(self._cast, self._values,
                                                self._diag, x.dtype)
            for _ in range(iterations):
                for backward in passes:
                    kernels.mcgs_sweep(self, vals, diag, b, x, backward)
            return
        if x.numel() == 0:
            return
        per_color, d = self._host_operands(to_numpy_dtype(x.dtype))
        xh, bh = x.numpy(), b.numpy()  # views: x is updated in place
        for _ in range(iterations):
            for backward in passes:
                for rows, off in (reversed(per_color) if backward
                                  else per_color):
                    dr = d[rows] if xh.ndim == 1 else d[rows, None]
                    xh[rows] = (bh[rows] - off @ xh) / dr
        return

    def _host_operands(self, ndt):
        """Per colour (rows, off-diagonal part of those rows of A) as scipy
        CSR in dtype ndt, and the diagonal; built once per dtype."""
        if ndt not in self._host:
            import scipy.sparse as sps

            n = self.shape[0]
            ip = self._indptr.numpy()
            r = np.repeat(np.arange(n), np.diff(ip))
            c = self._indices.numpy().astype(np.int64)
            v = self._values.numpy().astype(ndt)
            off = r != c
            # coo -> csr sums duplicates
            S = sps.csr_matrix((v[off], (r[off], c[off])), shape=(n, n))
            order = self._order.numpy().astype(np.int64)
            cp = self._classes.ptr_host
            per_color = []
            for k in range(self._ncolors):
                rows = order[cp[k]: cp[k + 1]]
                if len(rows):
                    per_color.append((rows, S[rows]))
            self._host[ndt] = (per_color, self._diag.numpy().astype(ndt))
        return self._host[ndt]

    # -- LinearOperator ---------------------------------------------------------
    def matvec(self, r, out: Optional[DistArray] = None) -> DistArray:
        """One symmetric sweep from x = 0: the multicolour SGS preconditioner
        applied to r of shape (n,) or (n, k)."""
        r = rowsched.as_rhs(r, self.shape[0], "r")
        tdt = common_value_dtype(self._values.dtype, r.local.dtype)
        x, direct = rowsched.result_buffer(r, out, tdt)
        b = r.local.to(tdt).contiguous()
        if b.data_ptr() == x.data_ptr():  # out aliases r
            b = b.clone()
        x.zero_()
        self._sweep_local(x, b, "symmetric", 1)
        return rowsched.finish_result(x, direct, r, out)

    rmatvec = matvec
