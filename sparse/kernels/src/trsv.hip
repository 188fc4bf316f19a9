// Sparse triangular solve by level scheduling (sparse/trisolve.py).
//
// The analysis splits the selected triangle into a strict-triangle CSR plus
// a diagonal vector and sorts the rows by dependency level: `order` lists the
// rows by (level, row), `level_ptr` the level boundaries in `order`.  Every
// row of a level depends only on rows of earlier levels, so
//
//   x[i] = (b[i] - sum_j a_ij x[j]) / a_ii        (a true division)
//
// runs level by level:
//  - trsv_level_kernel      one launch per WIDE level; the rows it depends on
//                           were written by earlier launches on the stream.
//  - trsv_chain_kernel      one launch, ONE 1024-thread workgroup, for a run
//                           of narrow levels with a workgroup barrier between
//                           levels (a bidiagonal matrix is one launch, not n).
//
// There is no waiting between workgroups anywhere: ordering comes from kernel
// boundaries and, inside the chain kernel's single workgroup, from
// __syncthreads().  x values are written to global memory and, in the chain
// kernel, re-read after the barrier by waves of the same workgroup (same CU,
// same L1), so plain loads see them; x and b are deliberately NOT __restrict__
// (out may alias b: b[i] is read only by the lanes that write x[i]).
#include "common.h"

namespace {

constexpr int TRSV_BLOCK = 256;
constexpr int TRSV_CHAIN_THREADS = 1024;

// `order` is int32 when n fits, int64 otherwise (wave-uniform branch)
__device__ __forceinline__ int64_t order_at(const void* order, bool o64,
                                            int64_t i) {
  return o64 ? static_cast<const int64_t*>(order)[i]
             : static_cast<int64_t>(static_cast<const int32_t*>(order)[i]);
}

// sum over the G consecutive lanes of a row group; the group's lane 0 holds it
template <int G, typename T>
__device__ __forceinline__ T group_reduce_sum(T v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_down(v, off, G);
  return v;
}
template <int G, typename T>
__device__ __forceinline__ c10::complex<T> group_reduce_sum(c10::complex<T> v) {
  return {group_reduce_sum<G>(v.real()), group_reduce_sum<G>(v.imag())};
}

// One wide level, single right-hand side: G lanes per row reduce over the
// row's strict entries.  Rows are order[row_lo + ri], ri < nrows.
template <typename T, typename I, int G>
__global__ __launch_bounds__(TRSV_BLOCK) void trsv_level_kernel(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ values, const T* __restrict__ diag,
    const void* __restrict__ order, bool o64, int64_t row_lo, int64_t nrows,
    const T* b, T* x) {
  const int64_t tid = (int64_t)blockIdx.x * TRSV_BLOCK + threadIdx.x;
  const int64_t ri = tid / G;
  const int g = (int)(tid % G);
  if (ri >= nrows) return;  // the G lanes of a group leave together
  const int64_t row = order_at(order, o64, row_lo + ri);
  const int64_t pe = indptr[row + 1];
  T acc = ZeroOf<T>::value();
  for (int64_t p = indptr[row] + g; p < pe; p += G)
    acc += nt_load(values + p) * x[(int64_t)indices[p]];
  if constexpr (G > 1) acc = group_reduce_sum<G>(acc);
  if (g == 0) x[row] = (b[row] - acc) / diag[row];
}

// One wide level, k > 1 right-hand sides (X, B row-major (n, k)): one lane
// per (row, column), column fastest, so the X reads and writes of a row
// coalesce.
template <typename T, typename I>
__global__ __launch_bounds__(TRSV_BLOCK) void trsv_level_multi_kernel(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ values, const T* __restrict__ diag,
    const void* __restrict__ order, bool o64, int64_t row_lo, int64_t nrows,
    int64_t k, const T* b, T* x) {
  const int64_t tid = (int64_t)blockIdx.x * TRSV_BLOCK + threadIdx.x;
  const int64_t ri = tid / k;
  const int64_t c = tid % k;
  if (ri >= nrows) return;
  const int64_t row = order_at(order, o64, row_lo + ri);
  const int64_t pe = indptr[row + 1];
  T acc = ZeroOf<T>::value();
  for (int64_t p = indptr[row]; p < pe; ++p)
    acc += values[p] * x[(int64_t)indices[p] * k + c];
  x[row * k + c] = (b[row * k + c] - acc) / diag[row];
}

// Levels [level_lo, level_hi), each at most TRSV_CHAIN_THREADS rows, in ONE
// workgroup: thread t takes item t of the level's width*k (row, column)
// items and strides by the block size; a workgroup barrier separates levels.
// Launched with a grid of exactly one block.
template <typename T, typename I>
__global__ __launch_bounds__(TRSV_CHAIN_THREADS) void trsv_chain_kernel(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ values, const T* __restrict__ diag,
    const void* __restrict__ order, bool o64,
    const int64_t* __restrict__ level_ptr, int64_t level_lo, int64_t level_hi,
    int64_t k, const T* b, T* x) {
  for (int64_t l = level_lo; l < level_hi; ++l) {
    const int64_t base = level_ptr[l];
    const int64_t items = (level_ptr[l + 1] - base) * k;
    for (int64_t it = threadIdx.x; it < items; it += TRSV_CHAIN_THREADS) {
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

}  // namespace

// sched: host (CPU) int64 tensor (nseg, 4), one row per segment:
//   wide  {0, row_lo, row_hi, G}      rows order[row_lo:row_hi], one level
//   chain {1, level_lo, level_hi, 0}  levels [level_lo, level_hi)
// All launches go to the current stream in schedule order; nothing here
// synchronises with the host.
void trsv_solve_hip(at::Tensor indptr, at::Tensor indices, at::Tensor values,
                    at::Tensor diag, at::Tensor order, at::Tensor level_ptr,
                    at::Tensor sched, at::Tensor b, at::Tensor x) {
  const int64_t n = indptr.numel() - 1;
  TORCH_CHECK(!sched.is_cuda() && sched.scalar_type() == at::kLong &&
                  sched.dim() == 2 && sched.size(1) == 4 &&
                  sched.is_contiguous(),
              "trsv_solve: sched must be a contiguous CPU int64 (nseg, 4)");
  for (const at::Tensor& t :
       {indptr, indices, values, diag, order, level_ptr, b})
    TORCH_CHECK(t.is_cuda() && t.device() == x.device() && t.is_contiguous(),
                "trsv_solve: operands must be contiguous and on x's device");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(),
              "trsv_solve: x must be a contiguous device tensor");
  TORCH_CHECK(x.dim() >= 1 && x.size(0) == n && b.sizes() == x.sizes(),
              "trsv_solve: b/x shape mismatch");
  TORCH_CHECK(values.scalar_type() == x.scalar_type() &&
                  diag.scalar_type() == x.scalar_type() &&
                  b.scalar_type() == x.scalar_type(),
              "trsv_solve: value dtype mismatch");
  TORCH_CHECK(diag.numel() == n && order.numel() == n &&
                  indices.numel() == values.numel() &&
                  indptr.scalar_type() == at::kLong &&
                  level_ptr.scalar_type() == at::kLong,
              "trsv_solve: bad analysis tensors");
  if (n == 0 || sched.size(0) == 0) return;
  const int64_t k = x.numel() / n;
  if (k == 0) return;
  const int64_t nlevels = level_ptr.numel() - 1;
  const bool o64 = order.scalar_type() == at::kLong;
  TORCH_CHECK(o64 || order.scalar_type() == at::kInt,
              "trsv_solve: order must be int32 or int64");
  const int64_t* sc = sched.data_ptr<int64_t>();
  const int64_t nseg = sched.size(0);
  // validate the whole schedule against the analysis sizes before the first
  // launch: the kernels index order/level_ptr with these bounds unchecked
  for (int64_t s = 0; s < nseg; ++s) {
    const int64_t kind = sc[4 * s], lo = sc[4 * s + 1], hi = sc[4 * s + 2],
                  G = sc[4 * s + 3];
    if (kind == 0) {
      TORCH_CHECK(0 <= lo && lo <= hi && hi <= n &&
                      (G == 1 || G == 8 || G == 64),
                  "trsv_solve: bad wide segment");
    } else {
      TORCH_CHECK(kind == 1 && 0 <= lo && lo <= hi && hi <= nlevels,
                  "trsv_solve: bad chain segment");
    }
  }
  hipStream_t stream = cur_stream();
  DISPATCH_VALUES(values.scalar_type(), "trsv_solve", [&] {
    using T = scalar_t;
    DISPATCH_INDEX(indices.scalar_type(), "trsv_solve", [&] {
      const int64_t* ip = indptr.data_ptr<int64_t>();
      const index_t* ix = indices.data_ptr<index_t>();
      const T* av = values.data_ptr<T>();
      const T* dg = diag.data_ptr<T>();
      const void* ord = order.data_ptr();
      const int64_t* lp = level_ptr.data_ptr<int64_t>();
      const T* bp = b.data_ptr<T>();
      T* xp = x.data_ptr<T>();
      for (int64_t s = 0; s < nseg; ++s) {
        const int64_t kind = sc[4 * s], lo = sc[4 * s + 1], hi = sc[4 * s + 2],
                      G = sc[4 * s + 3];
        if (hi <= lo) continue;  // empty segment: no launch
        if (kind == 1) {
          hipLaunchKernelGGL((trsv_chain_kernel<T, index_t>), dim3(1),
                             dim3(TRSV_CHAIN_THREADS), 0, stream, ip, ix, av,
                             dg, ord, o64, lp, lo, hi, k, bp, xp);
          continue;
        }
        const int64_t nrows = hi - lo;
        if (k > 1) {
          const int64_t blocks = (nrows * k + TRSV_BLOCK - 1) / TRSV_BLOCK;
          hipLaunchKernelGGL((trsv_level_multi_kernel<T, index_t>),
                             dim3(blocks), dim3(TRSV_BLOCK), 0, stream, ip, ix,
                             av, dg, ord, o64, lo, nrows, k, bp, xp);
          continue;
        }
        const int64_t blocks = (nrows * G + TRSV_BLOCK - 1) / TRSV_BLOCK;
        auto level = [&](auto gg) {
          constexpr int GG = decltype(gg)::value;
          hipLaunchKernelGGL((trsv_level_kernel<T, index_t, GG>), dim3(blocks),
                             dim3(TRSV_BLOCK), 0, stream, ip, ix, av, dg, ord,
                             o64, lo, nrows, bp, xp);
        };
        if (G == 1) level(std::integral_constant<int, 1>{});
        else if (G == 8) level(std::integral_constant<int, 8>{});
        else level(std::integral_constant<int, 64>{});
      }
    });
  });
  SPARSE_CHECK_HIP(hipGetLastError());
}
