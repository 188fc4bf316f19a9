"""Row schedules: what the level- and colour-scheduled operators share.

The triangular solve (sparse/trisolve.py), ILU(0) (sparse/ilu.py) and the
multicolour Gauss-Seidel sweeps (sparse/gauss_seidel.py) all sort the rows by
an integer class, a dependency level or a colour, into `order`, cut it at the
class boundaries, pick the lanes per row of each segment from its mean row
length and hand the kernels a host-side schedule with one row
(kind, lo, hi, G) per launch (kernels/src/rowsched.h).  This module holds
the steps of that analysis, and of applying the result to a right-hand side,
that do not depend on which of the three is asking.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from .darray import DistArray, asdistarray
from .parallel import comm

Segments = Tuple[np.ndarray, np.ndarray, np.ndarray]  # chain?, lo, hi (classes)


# -- preamble -------------------------------------------------------------------
def single_rank(what: str) -> None:
    if comm.world_size() > 1:
        raise NotImplementedError(
            f"{what} is not implemented at world size > 1: rows depend on "
            "rows of other ranks' slabs (a per-slab block-Jacobi variant is "
            "out of scope)")


def as_csr(A):
    from .csr import csr_array
    from .module import is_sparse_matrix

    if isinstance(A, csr_array):
        return A
    return A.tocsr() if is_sparse_matrix(A) else csr_array(A)


def square_csr(A, what: str):
    """A as a csr_array, for an operator `what` that needs a square matrix
    on a single rank."""
    single_rank(what)
    A = as_csr(A)
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"A must be square, got shape {A.shape}")
    return A


# -- structure ------------------------------------------------------------------
def row_index(indptr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(stored entries per row, row of every stored entry) of a CSR
    structure, both int64 on indptr's device."""
    counts = indptr[1:] - indptr[:-1]
    rows = torch.repeat_interleave(
        torch.arange(counts.numel(), dtype=torch.int64, device=indptr.device),
        counts)
    return counts, rows


def same_structure(new: torch.Tensor, old: torch.Tensor) -> bool:
    """Whether the index array `new` of a matrix handed to a refactor holds
    what the analysed `old` one does: the same memory, or equal contents."""
    if (new.data_ptr() == old.data_ptr() and new.dtype == old.dtype
            and new.numel() == old.numel()):
        return True
    return (new.numel() == old.numel() and new.device == old.device
            and torch.equal(new.to(old.dtype), old))


def summed_diagonal(on: torch.Tensor, rows: torch.Tensor,
                    values: torch.Tensor, n: int,
                    first: Sequence[Tuple[torch.Tensor, Exception]] = ()
                    ) -> torch.Tensor:
    """The sum of the stored diagonal entries of each row (`on` marks them
    among the stored entries, `rows` holds every entry's row); a missing or
    zero one raises numpy.linalg.LinAlgError.  `first` holds (flag,
    exception) pairs, flag a 0-d bool tensor on the device: they ride in the
    same host read and are raised, in order, before the diagonal's."""
    diag = torch.zeros(n, dtype=values.dtype, device=values.device)
    diag.index_add_(0, rows[on], values[on])
    # one device reduction, one host read
    *flags, singular = torch.stack(
        [f for f, _ in first] + [(diag == 0).any()]).tolist()
    for hit, (_, exc) in zip(flags, first):
        if hit:
            raise exc
    if singular:
        raise np.linalg.LinAlgError(
            "A is singular: zero or missing entry on the diagonal")
    return diag


class RowClasses:
    """The rows sorted by (class, row) for a per-row integer class `key` >= 0
    (a dependency level, a colour), given on the host or on the device `dev`.

    order     rows by (class, row) on dev; int32 when n < 2**31
    ptr       class boundaries in `order` (int64, nclasses + 1) on dev
    ptr_host  the same as a numpy array
    A key on the host costs no host read; one on the device costs two (the
    number of classes, then the boundaries)."""

    def __init__(self, key: torch.Tensor, dev):
        if key.is_cuda:
            widths = torch.bincount(key.long())  # host read of C
        else:  # numpy: torch.bincount on the host is ten times slower
            widths = torch.from_numpy(np.bincount(key.numpy()))
        self.nclasses = int(widths.numel())
        ptr = torch.zeros(self.nclasses + 1, dtype=torch.int64,
                          device=key.device)
        torch.cumsum(widths, 0, out=ptr[1:])
        self.ptr = ptr.to(dev)
        self.ptr_host = ptr.cpu().numpy()
        order = torch.sort(key.to(dev), stable=True).indices
        if key.numel() < 2**31:
            order = order.to(torch.int32)
        self.order = order.contiguous()

    def sums(self, counts: torch.Tensor) -> np.ndarray:
        """Per class, the sum of the per-row vector `counts` (stored entries
        of a row, on the device) — one host read."""
        cs = torch.zeros(counts.numel() + 1, dtype=torch.int64,
                         device=counts.device)
        torch.cumsum(counts[self.order.long()], 0, out=cs[1:])
        return np.diff(cs[self.ptr].cpu().numpy())


# -- schedule -------------------------------------------------------------------
def plain_segments(nclasses: int) -> Segments:
    """Every class a wide segment of its own."""
    lo = np.arange(nclasses, dtype=np.int64)
    return np.zeros(nclasses, dtype=bool), lo, lo + 1


def chain_segments(widths: np.ndarray, chain_width: int) -> Segments:
    """A maximal run of consecutive classes of at most chain_width rows each
    is one chain segment, every other class a wide segment of its own."""
    nclasses = len(widths)
    if not nclasses:
        return plain_segments(0)
    small = widths <= chain_width
    # a class opens a segment unless it and its predecessor are both small
    starts = np.flatnonzero(np.r_[True, ~(small[1:] & small[:-1])])
    ends = np.r_[starts[1:], nclasses].astype(np.int64)
    return small[starts], starts, ends


def schedule_rows(ptr: np.ndarray, nnz: np.ndarray, seg: Segments,
                  group: Callable[[float], int],
                  chain_group: Optional[Callable[[float], int]] = None
                  ) -> torch.Tensor:
    """The host-side schedule, int64 (nseg, 4): per segment
    (0, row_lo, row_hi, G) for a wide one and (1, class_lo, class_hi, G) for
    a chain.  G = group(mean row length of the segment) from the per-class
    entry counts `nnz`; a chain gets chain_group(...) or, without one, 0."""
    chain, starts, ends = seg
    sched = np.zeros((len(starts), 4), dtype=np.int64)
    for s, (c, lo, hi) in enumerate(zip(chain, starts, ends)):
        mean = nnz[lo:hi].sum() / max(ptr[hi] - ptr[lo], 1)
        if c:
            sched[s] = (1, lo, hi, chain_group(mean) if chain_group else 0)
        else:
            sched[s] = (0, ptr[lo], ptr[hi], group(mean))
    return torch.from_numpy(sched)


# -- applying an operator to a right-hand side ------------------------------------
def cast_operands(cache: dict, values: torch.Tensor, diag: torch.Tensor, tdt
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(values, diag) in the value dtype tdt of a wider right-hand side, cast
    once per dtype into `cache`."""
    if tdt == values.dtype:
        return values, diag
    if tdt not in cache:
        cache[tdt] = (values.to(tdt), diag.to(tdt))
    return cache[tdt]


def as_rhs(b, n: int, name: str) -> DistArray:
    b = asdistarray(b)
    if b.ndim not in (1, 2) or b.shape[0] != n:
        raise ValueError(
            f"{name} has shape {b.shape}, expected ({n},) or ({n}, k)")
    return b


def result_buffer(b: DistArray, out: Optional[DistArray], tdt
                  ) -> Tuple[torch.Tensor, bool]:
    """(x, direct): the uninitialised local buffer a kernel writes the result
    for b into — out's own when it has the result's dtype and shape and is
    contiguous (direct), else a new one."""
    direct = (out is not None and out.local.dtype == tdt
              and out.shape == b.shape and out.local.is_contiguous())
    x = out.local if direct else torch.empty(
        b.local.shape, dtype=tdt, device=b.local.device)
    return x, direct


def finish_result(x: torch.Tensor, direct: bool, b: DistArray,
                  out: Optional[DistArray]) -> DistArray:
    """What the operator returns for result_buffer's x: out itself, written
    directly or by a converting copy, else x wrapped like b."""
    if direct:
        return out
    res = DistArray.from_local(x, b.partition, b.shape)
    if out is not None:
        out.local.copy_(res.local.to(out.local.dtype))
        return out
    return res
