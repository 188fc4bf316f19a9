// The relaxation step over a row list, shared by the sparse triangular solve
// (sparse/trisolve.py) and the multicolour Gauss-Seidel sweeps
// (sparse/gauss_seidel.py):
//
//   x[i] = (b[i] - sum_j a_ij x[j]) / a_ii        (a true division)
//
// for the rows order[row_lo : row_lo + nrows] of a CSR matrix, a_ii taken from
// the vector `diag`.  The rows of one launch never read each other's x, by
// construction of the row schedule (rowsched.h):
//  - triangular solve, SkipDiag = false.  The matrix is the STRICT triangle,
//    the rows are sorted by (dependency level, row), and every row of a level
//    depends only on rows of earlier levels.  A wide level is one launch; a
//    run of narrow levels is one launch of relax_chain_kernel.
//  - Gauss-Seidel sweep, SkipDiag = true.  The matrix is the full A, the rows
//    are sorted by (colour, row), and no stored off-diagonal entry joins two
//    rows of one colour (checked at analysis), so a row reads only x of other
//    colours and a colour is one launch.  Stored diagonal entries are skipped
//    in the sum (their sum is `diag`); duplicate off-diagonal entries simply
//    add up.  A sweep takes the colours ascending, or (backward) descending.
// SkipDiag is the only difference and a template parameter: the triangular
// solve has no compare in its loop.
//  - relax_rows_kernel        one right-hand side: G lanes per row reduce over
//                             the row's entries (G = 1 / 8 / 64 from the mean
//                             row length of the segment).
//  - relax_rows_multi_kernel  k > 1 right-hand sides (row-major (n, k)): one
//                             lane per (row, column), column fastest.
//  - relax_chain_kernel       one launch, ONE 1024-thread workgroup, for a run
//                             of narrow levels with a workgroup barrier
//                             between levels (a bidiagonal matrix is one
//                             launch, not n).
//
// There is no waiting between workgroups anywhere: ordering comes from kernel
// boundaries and, inside the chain kernel's single workgroup, from
// __syncthreads().  x values are written to global memory and, in the chain
// kernel, re-read after the barrier by waves of the same workgroup (same CU,
// same L1), so plain loads see them.  x is read and written in place by
// different lanes of one launch and out may alias b (b[i] is read only by
// the lanes that write x[i]), so x and b are deliberately NOT __restrict__.
#include "rowsched.h"

namespace {

// One segment, single right-hand side: G lanes per row reduce over the row's
// entries.  Rows are order[row_lo + ri], ri < nrows.
template <typename T, typename I, int G, bool SkipDiag>
__global__ __launch_bounds__(ROWSCHED_BLOCK) void relax_rows_kernel(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ values, const T* __restrict__ diag,
    const void* __restrict__ order, bool o64, int64_t row_lo, int64_t nrows,
    const T* b, T* x) {
  const int64_t tid = (int64_t)blockIdx.x * ROWSCHED_BLOCK + threadIdx.x;
  const int64_t ri = tid / G;
  const int g = (int)(tid % G);
  if (ri >= nrows) return;  // the G lanes of a group leave together
  const int64_t row = order_at(order, o64, row_lo + ri);
  const int64_t pe = indptr[row + 1];
  T acc = ZeroOf<T>::value();
  for (int64_t p = indptr[row] + g; p < pe; p += G) {
    // constant false for the triangular solve: no column load, no compare
    const bool skip = SkipDiag && (int64_t)indices[p] == row;
    const T a = nt_load(values + p);
    if (!skip) acc += a * x[(int64_t)indices[p]];
  }
  if constexpr (G > 1) acc = group_reduce_sum<G>(acc);
  if (g == 0) x[row] = (b[row] - acc) / diag[row];
}

// One segment, k > 1 right-hand sides (X, B row-major (n, k)): one lane per
// (row, column), column fastest, so the X reads and writes of a row coalesce.
template <typename T, typename I, bool SkipDiag>
__global__ __launch_bounds__(ROWSCHED_BLOCK) void relax_rows_multi_kernel(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ values, const T* __restrict__ diag,
    const void* __restrict__ order, bool o64, int64_t row_lo, int64_t nrows,
    int64_t k, const T* b, T* x) {
  const int64_t tid = (int64_t)blockIdx.x * ROWSCHED_BLOCK + threadIdx.x;
  const int64_t ri = tid / k;
  const int64_t c = tid % k;
  if (ri >= nrows) return;
  const int64_t row = order_at(order, o64, row_lo + ri);
  const int64_t pe = indptr[row + 1];
  T acc = ZeroOf<T>::value();
  for (int64_t p = indptr[row]; p < pe; ++p) {
    const bool skip = SkipDiag && (int64_t)indices[p] == row;
    if (!skip) acc += values[p] * x[(int64_t)indices[p] * k + c];
  }
  x[row * k + c] = (b[row * k + c] - acc) / diag[row];
}

// Levels [level_lo, level_hi), each at most ROWSCHED_CHAIN_THREADS rows, in
// ONE workgroup: thread t takes item t of the level's width*k (row, column)
// items and strides by the block size; a workgroup barrier separates levels.
// Launched with a grid of exactly one block.  Strict-triangle rows only: the
// colour schedule has no chain segments.
template <typename T, typename I>
__global__ __launch_bounds__(ROWSCHED_CHAIN_THREADS) void relax_chain_kernel(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ values, const T* __restrict__ diag,
    const void* __restrict__ order, bool o64,
    const int64_t* __restrict__ level_ptr, int64_t level_lo, int64_t level_hi,
    int64_t k, const T* b, T* x) {
  for (int64_t l = level_lo; l < level_hi; ++l) {
    const int64_t base = level_ptr[l];
    const int64_t items = (level_ptr[l + 1] - base) * k;
    for (int64_t it = threadIdx.x; it < items; it += ROWSCHED_CHAIN_THREADS) {
      const int64_t ri = k == 1 ? it : it / k;
      const int64_t c = k == 1 ? 0 : it % k;
      const int64_t row = order_at(order, o64, base + ri);
      const int64_t pe = indptr[row + 1];
      T acc = ZeroOf<T>::value();
      for (int64_t p = indptr[row]; p < pe; ++p)
        acc += values[p] * x[(int64_t)indices[p] * k + c];
      x[row * k + c] = (b[row * k + c] - acc) / diag[row];
    }
    // all threads of the block reach this barrier every level (the loop
    // bounds are uniform); it orders this level's x stores before the next
    // level's x loads within the workgroup
    __syncthreads();
  }
}

// One pass over the schedule (rowsched.h), forwards or in reverse, one launch
// per non-empty segment on the current stream.  level_ptr is undefined for
// the sweep, whose schedule has wide segments only.
template <bool SkipDiag>
void relax_hip(const at::Tensor& indptr, const at::Tensor& indices,
               const at::Tensor& values, const at::Tensor& diag,
               const at::Tensor& order, const at::Tensor& level_ptr,
               const at::Tensor& sched, const at::Tensor& b,
               const at::Tensor& x, bool reverse) {
  constexpr const char* OP = SkipDiag ? "mcgs_sweep" : "trsv_solve";
  const int64_t n = indptr.numel() - 1;
  const bool o64 = rowsched_check_operands(
      OP, x, {indptr, indices, values, diag, order, b}, indptr, indices,
      values, order, level_ptr);
  TORCH_CHECK(x.dim() >= 1 && x.size(0) == n && b.sizes() == x.sizes(), OP,
              ": b/x shape mismatch");
  TORCH_CHECK(values.scalar_type() == x.scalar_type() &&
                  diag.scalar_type() == x.scalar_type() &&
                  b.scalar_type() == x.scalar_type(),
              OP, ": value dtype mismatch");
  TORCH_CHECK(diag.numel() == n, OP, ": bad analysis tensors");
  rowsched_check_schedule(OP, sched, n, level_ptr, false);
  if (n == 0 || sched.size(0) == 0) return;
  const int64_t k = x.numel() / n;
  if (k == 0) return;
  hipStream_t stream = cur_stream();
  DISPATCH_VALUES(values.scalar_type(), OP, [&] {
    using T = scalar_t;
    DISPATCH_INDEX(indices.scalar_type(), OP, [&] {
      const int64_t* ip = indptr.data_ptr<int64_t>();
      const index_t* ix = indices.data_ptr<index_t>();
      const T* av = values.data_ptr<T>();
      const T* dg = diag.data_ptr<T>();
      const void* ord = order.data_ptr();
      const T* bp = b.data_ptr<T>();
      T* xp = x.data_ptr<T>();
      rowsched_for_each(sched, reverse, [&](int64_t kind, int64_t lo,
                                            int64_t hi, int64_t G) {
        if (kind == 1) {
          if constexpr (!SkipDiag)
            hipLaunchKernelGGL((relax_chain_kernel<T, index_t>), dim3(1),
                               dim3(ROWSCHED_CHAIN_THREADS), 0, stream, ip, ix,
                               av, dg, ord, o64, level_ptr.data_ptr<int64_t>(),
                               lo, hi, k, bp, xp);
          return;
        }
        const int64_t nrows = hi - lo;
        if (k > 1) {
          const int64_t blocks =
              (nrows * k + ROWSCHED_BLOCK - 1) / ROWSCHED_BLOCK;
          hipLaunchKernelGGL((relax_rows_multi_kernel<T, index_t, SkipDiag>),
                             dim3(blocks), dim3(ROWSCHED_BLOCK), 0, stream, ip,
                             ix, av, dg, ord, o64, lo, nrows, k, bp, xp);
          return;
        }
        const int64_t blocks =
            (nrows * G + ROWSCHED_BLOCK - 1) / ROWSCHED_BLOCK;
        rowsched_with_group(G, [&](auto gg) {
          hipLaunchKernelGGL(
              (relax_rows_kernel<T, index_t, decltype(gg)::value, SkipDiag>),
              dim3(blocks), dim3(ROWSCHED_BLOCK), 0, stream, ip, ix, av, dg,
              ord, o64, lo, nrows, bp, xp);
        });
      });
    });
  });
  SPARSE_CHECK_HIP(hipGetLastError());
}

}  // namespace

void trsv_solve_hip(at::Tensor indptr, at::Tensor indices, at::Tensor values,
                    at::Tensor diag, at::Tensor order, at::Tensor level_ptr,
                    at::Tensor sched, at::Tensor b, at::Tensor x) {
  relax_hip<false>(indptr, indices, values, diag, order, level_ptr, sched, b,
                   x, false);
}

void mcgs_sweep_hip(at::Tensor indptr, at::Tensor indices, at::Tensor values,
                    at::Tensor diag, at::Tensor order, at::Tensor sched,
                    at::Tensor b, at::Tensor x, bool backward) {
  relax_hip<true>(indptr, indices, values, diag, order, at::Tensor(), sched, b,
                  x, backward);
}
