// Multicolour Gauss-Seidel sweeps (sparse/gauss_seidel.py).
//
// The rows are sorted by (colour, row) into `order`; no stored off-diagonal
// entry joins two rows of one colour (checked at analysis), so within a
// colour every row
//
//   x[i] = (b[i] - sum_{j != i} a_ij x[j]) / a_ii     (a true division)
//
// reads only x of other colours and the colour is ONE launch over the row
// list order[row_lo : row_lo + nrows] of the full CSR matrix.  Stored
// diagonal entries are skipped in the sum (their sum is `diag`), duplicate
// off-diagonal entries simply add up.
//  - mcgs_rows_kernel        one right-hand side: G lanes per row reduce over
//                            the row's entries (G = 1 / 8 / 64 from the mean
//                            row length of the colour, as in trsv.hip).
//  - mcgs_rows_multi_kernel  k > 1 right-hand sides (row-major (n, k)): one
//                            lane per (row, column), column fastest.
// A sweep is a purely sequential chain of launches on the current stream,
// ascending colours forward and descending backward; ordering comes from the
// kernel boundaries alone and nothing synchronises with the host.  x is read
// and written in place by different lanes of one launch, so x and b are
// deliberately NOT __restrict__.
#include "common.h"

namespace {

constexpr int MCGS_BLOCK = 256;

// `order` is int32 when n fits, int64 otherwise (wave-uniform branch)
__device__ __forceinline__ int64_t mcgs_order_at(const void* order, bool o64,
                                                 int64_t i) {
  return o64 ? static_cast<const int64_t*>(order)[i]
             : static_cast<int64_t>(static_cast<const int32_t*>(order)[i]);
}

// sum over the G consecutive lanes of a row group; the group's lane 0 holds it
template <int G, typename T>
__device__ __forceinline__ T mcgs_group_sum(T v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_down(v, off, G);
  return v;
}
template <int G, typename T>
__device__ __forceinline__ c10::complex<T> mcgs_group_sum(c10::complex<T> v) {
  return {mcgs_group_sum<G>(v.real()), mcgs_group_sum<G>(v.imag())};
}

template <typename T, typename I, int G>
__global__ __launch_bounds__(MCGS_BLOCK) void mcgs_rows_kernel(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ values, const T* __restrict__ diag,
    const void* __restrict__ order, bool o64, int64_t row_lo, int64_t nrows,
    const T* b, T* x) {
  const int64_t tid = (int64_t)blockIdx.x * MCGS_BLOCK + threadIdx.x;
  const int64_t ri = tid / G;
  const int g = (int)(tid % G);
  if (ri >= nrows) return;  // the G lanes of a group leave together
  const int64_t row = mcgs_order_at(order, o64, row_lo + ri);
  const int64_t pe = indptr[row + 1];
  T acc = ZeroOf<T>::value();
  for (int64_t p = indptr[row] + g; p < pe; p += G) {
    const int64_t j = (int64_t)indices[p];
    const T a = nt_load(values + p);
    if (j != row) acc += a * x[j];
  }
  if constexpr (G > 1) acc = mcgs_group_sum<G>(acc);
  if (g == 0) x[row] = (b[row] - acc) / diag[row];
}

template <typename T, typename I>
__global__ __launch_bounds__(MCGS_BLOCK) void mcgs_rows_multi_kernel(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    const T* __restrict__ values, const T* __restrict__ diag,
    const void* __restrict__ order, bool o64, int64_t row_lo, int64_t nrows,
    int64_t k, const T* b, T* x) {
  const int64_t tid = (int64_t)blockIdx.x * MCGS_BLOCK + threadIdx.x;
  const int64_t ri = tid / k;
  const int64_t c = tid % k;
  if (ri >= nrows) return;
  const int64_t row = mcgs_order_at(order, o64, row_lo + ri);
  const int64_t pe = indptr[row + 1];
  T acc = ZeroOf<T>::value();
  for (int64_t p = indptr[row]; p < pe; ++p) {
    const int64_t j = (int64_t)indices[p];
    if (j != row) acc += values[p] * x[j * k + c];
  }
  x[row * k + c] = (b[row * k + c] - acc) / diag[row];
}

}  // namespace

// sched: host (CPU) int64 tensor (ncolors, 3), one row {row_lo, row_hi, G}
// per colour: rows order[row_lo:row_hi], G lanes per row.  One pass over all
// colours, ascending or (backward) descending, one launch per non-empty
// colour on the current stream.
void mcgs_sweep_hip(at::Tensor indptr, at::Tensor indices, at::Tensor values,
                    at::Tensor diag, at::Tensor order, at::Tensor sched,
                    at::Tensor b, at::Tensor x, bool backward) {
  const int64_t n = indptr.numel() - 1;
  TORCH_CHECK(!sched.is_cuda() && sched.scalar_type() == at::kLong &&
                  sched.dim() == 2 && sched.size(1) == 3 &&
                  sched.is_contiguous(),
              "mcgs_sweep: sched must be a contiguous CPU int64 (ncolors, 3)");
  for (const at::Tensor& t : {indptr, indices, values, diag, order, b})
    TORCH_CHECK(t.is_cuda() && t.device() == x.device() && t.is_contiguous(),
                "mcgs_sweep: operands must be contiguous and on x's device");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(),
              "mcgs_sweep: x must be a contiguous device tensor");
  TORCH_CHECK(x.dim() >= 1 && x.size(0) == n && b.sizes() == x.sizes(),
              "mcgs_sweep: b/x shape mismatch");
  TORCH_CHECK(values.scalar_type() == x.scalar_type() &&
                  diag.scalar_type() == x.scalar_type() &&
                  b.scalar_type() == x.scalar_type(),
              "mcgs_sweep: value dtype mismatch");
  TORCH_CHECK(diag.numel() == n && order.numel() == n &&
                  indices.numel() == values.numel() &&
                  indptr.scalar_type() == at::kLong &&
                  (indices.scalar_type() == at::kInt ||
                   indices.scalar_type() == at::kLong),
              "mcgs_sweep: bad analysis tensors");
  const bool o64 = order.scalar_type() == at::kLong;
  TORCH_CHECK(o64 || order.scalar_type() == at::kInt,
              "mcgs_sweep: order must be int32 or int64");
  const int64_t ncolors = sched.size(0);
  if (n == 0 || ncolors == 0) return;
  const int64_t k = x.numel() / n;
  if (k == 0) return;
  const int64_t* sc = sched.data_ptr<int64_t>();
  // validate the whole schedule before the first launch: the kernels index
  // `order` with these bounds unchecked
  for (int64_t c = 0; c < ncolors; ++c) {
    const int64_t lo = sc[3 * c], hi = sc[3 * c + 1], G = sc[3 * c + 2];
    TORCH_CHECK(0 <= lo && lo <= hi && hi <= n &&
                    (G == 1 || G == 8 || G == 64),
                "mcgs_sweep: bad colour segment");
  }
  hipStream_t stream = cur_stream();
  DISPATCH_VALUES(values.scalar_type(), "mcgs_sweep", [&] {
    using T = scalar_t;
    DISPATCH_INDEX(indices.scalar_type(), "mcgs_sweep", [&] {
      const int64_t* ip = indptr.data_ptr<int64_t>();
      const index_t* ix = indices.data_ptr<index_t>();
      const T* av = values.data_ptr<T>();
      const T* dg = diag.data_ptr<T>();
      const void* ord = order.data_ptr();
      const T* bp = b.data_ptr<T>();
      T* xp = x.data_ptr<T>();
      for (int64_t s = 0; s < ncolors; ++s) {
        const int64_t c = backward ? ncolors - 1 - s : s;
        const int64_t lo = sc[3 * c], hi = sc[3 * c + 1], G = sc[3 * c + 2];
        if (hi <= lo) continue;  // empty colour: no launch
        const int64_t nrows = hi - lo;
        if (k > 1) {
          const int64_t blocks = (nrows * k + MCGS_BLOCK - 1) / MCGS_BLOCK;
          hipLaunchKernelGGL((mcgs_rows_multi_kernel<T, index_t>),
                             dim3(blocks), dim3(MCGS_BLOCK), 0, stream, ip, ix,
                             av, dg, ord, o64, lo, nrows, k, bp, xp);
          continue;
        }
        const int64_t blocks = (nrows * G + MCGS_BLOCK - 1) / MCGS_BLOCK;
        auto rows = [&](auto gg) {
          constexpr int GG = decltype(gg)::value;
          hipLaunchKernelGGL((mcgs_rows_kernel<T, index_t, GG>), dim3(blocks),
                             dim3(MCGS_BLOCK), 0, stream, ip, ix, av, dg, ord,
                             o64, lo, nrows, bp, xp);
        };
        if (G == 1) rows(std::integral_constant<int, 1>{});
        else if (G == 8) rows(std::integral_constant<int, 8>{});
        else rows(std::integral_constant<int, 64>{});
      }
    });
  });
  SPARSE_CHECK_HIP(hipGetLastError());
}
