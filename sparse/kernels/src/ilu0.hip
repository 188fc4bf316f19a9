// ILU(0) numeric factorisation by level scheduling (sparse/ilu.py).
//
// The factor is computed IN PLACE in `vals`, a copy of A's values on A's CSR
// pattern (rows column-sorted and duplicate-free, every diagonal stored;
// diag_ptr[i] is the position of a_ii).  Row-wise IKJ: for row i and every
// stored k < i in ascending order
//
//   a_ik /= u_kk                                    (a true division)
//   a_ij -= a_ik * a_kj   for every stored j > k of row i also stored in row k
//
// Row k is in the strict lower pattern of row i, so it belongs to an earlier
// level of the lower-triangle level schedule (the one the L solver uses:
// `order`, `level_ptr`, same chain cut), and rows of one level never read
// each other.  As in relax.hip the levels run as
//  - ilu0_level_kernel   one launch per WIDE level; the rows it reads were
//                        finished by earlier launches on the stream.
//  - ilu0_chain_kernel   one launch, ONE 1024-thread workgroup, for a run of
//                        narrow levels with a workgroup barrier between them.
// There is no waiting between workgroups anywhere: ordering between rows
// comes from kernel boundaries and, inside the chain kernel's single
// workgroup, from __syncthreads() (same CU, same L1, so plain loads see the
// earlier level's stores).
//
// Inside a row the k loop is sequential by nature (a_ik for a later k may
// have been updated by an earlier k).  Lane mapping, "owner computes": G
// consecutive lanes take row i and lane g owns positions g, g+G, ... of the
// row.  For each k the owner of a_ik forms the multiplier, stores it and
// broadcasts it with a width-G shuffle (registers, no memory hand-off); every
// lane then updates only positions it owns.  So every value of row i is read
// and written by ONE lane for the whole factorisation of the row: its loads
// follow its own stores in program order, no fence or barrier is needed
// inside a row, and the k order of the updates to each entry is the
// sequential reference's.  Values of row k are only read.
//
// The owned updates of one k are found either way round, chosen per k by a
// group-uniform test on the two lengths:
//  - scan:  each lane walks its owned positions past k and looks the column
//           up in row k's upper part by binary search (work split G ways);
//  - walk:  row k's upper part is much shorter than the rest of row i: every
//           lane walks row k (same addresses in all lanes) and looks each
//           column up in row i by binary search; the lane owning the hit
//           updates it.  This keeps a row of thousands of entries with short
//           rows k (an arrow's last row) from scanning itself once per k.
// Rows of any length work in both.
//
// A pivot u_ii that is exactly zero when row i is finished is recorded by an
// ordinary vector atomicMin of i into one int64 word; the host reads it once
// after the phase.  Rows that divide by it produce inf/nan, nothing faults.
//
// `vals` is deliberately NOT __restrict__ / const: rows read earlier rows of
// the array they write.
#include "rowsched.h"

namespace {

// value of lane `src` of the G-lane row group, in every lane of the group
template <int G, typename T>
__device__ __forceinline__ T group_bcast(T v, int src) {
  return __shfl(v, src, G);
}
template <int G, typename T>
__device__ __forceinline__ c10::complex<T> group_bcast(c10::complex<T> v,
                                                       int src) {
  return {__shfl(v.real(), src, G), __shfl(v.imag(), src, G)};
}

// first position in [lo, hi) whose column is >= j (columns sorted)
template <typename I>
__device__ __forceinline__ int64_t col_lower_bound(const I* indices,
                                                   int64_t lo, int64_t hi,
                                                   int64_t j) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(indices[mid]) < j) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Factorise row i with the G lanes of one row group (g = lane in the group).
// All G lanes call it together and take the same branches: every condition
// below depends on the row only, except the ownership tests.
template <typename T, typename I, int G>
__device__ __forceinline__ void ilu0_row(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    T* vals, const int64_t* __restrict__ diag_ptr, int64_t n, int64_t i, int g,
    long long* flag) {
  if (i < 0 || i >= n) return;
  const int64_t ps = indptr[i], pe = indptr[i + 1], dp = diag_ptr[i];
  if (dp < ps || dp >= pe) return;  // the analysis guarantees a diagonal
  for (int64_t q = ps; q < dp; ++q) {
    const int64_t k = static_cast<int64_t>(indices[q]);
    if (k < 0 || k >= i) return;  // not a strict-lower entry: bad structure
    const int64_t kd = diag_ptr[k], ke = indptr[k + 1];
    const int owner = static_cast<int>((q - ps) & (G - 1));
    T m = ZeroOf<T>::value();
    if (g == owner) {
      m = vals[q] / vals[kd];
      vals[q] = m;
    }
    if constexpr (G > 1) m = group_bcast<G>(m, owner);
    const int64_t rest = pe - q - 1;   // entries of row i past k
    const int64_t lk = ke - kd - 1;    // entries of row k past its diagonal
    if (lk <= 0 || rest <= 0) continue;
    if (lk * (4 * G) <= rest) {
      // walk row k, look up in row i; hits go to their owner
      int64_t from = q + 1;
      for (int64_t t = kd + 1; t < ke; ++t) {
        const int64_t j = static_cast<int64_t>(indices[t]);
        const int64_t p = col_lower_bound(indices, from, pe, j);
        if (p >= pe) break;
        from = p;  // columns of row k ascend, so do the hits
        if (static_cast<int64_t>(indices[p]) == j &&
            static_cast<int>((p - ps) & (G - 1)) == g)
          vals[p] -= m * vals[t];
      }
    } else {
      // scan the owned positions past k, look up in row k's upper part
      int64_t p = q + 1 + ((g - (q + 1 - ps)) & (G - 1));
      for (; p < pe; p += G) {
        const int64_t j = static_cast<int64_t>(indices[p]);
        const int64_t t = col_lower_bound(indices, kd + 1, ke, j);
        if (t < ke && static_cast<int64_t>(indices[t]) == j)
          vals[p] -= m * vals[t];
      }
    }
  }
  if (g == static_cast<int>((dp - ps) & (G - 1)) &&
      vals[dp] == ZeroOf<T>::value())
    atomicMin(flag, static_cast<long long>(i));
}

// One wide level: rows order[row_lo + ri], ri < nrows, G lanes per row.
template <typename T, typename I, int G>
__global__ __launch_bounds__(ROWSCHED_BLOCK) void ilu0_level_kernel(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    T* vals, const int64_t* __restrict__ diag_ptr,
    const void* __restrict__ order, bool o64, int64_t n, int64_t row_lo,
    int64_t nrows, long long* flag) {
  const int64_t tid = (int64_t)blockIdx.x * ROWSCHED_BLOCK + threadIdx.x;
  const int64_t ri = tid / G;
  const int g = (int)(tid % G);
  if (ri >= nrows) return;  // the G lanes of a group leave together
  ilu0_row<T, I, G>(indptr, indices, vals, diag_ptr, n,
                    order_at(order, o64, row_lo + ri), g, flag);
}

// Levels [level_lo, level_hi), each at most ROWSCHED_CHAIN_THREADS rows, in
// ONE workgroup: the group of G threads starting at thread t takes row t / G of
// the level and strides by the block size; a workgroup barrier separates
// levels.  Launched with a grid of exactly one block.
template <typename T, typename I, int G>
__global__ __launch_bounds__(ROWSCHED_CHAIN_THREADS) void ilu0_chain_kernel(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    T* vals, const int64_t* __restrict__ diag_ptr,
    const void* __restrict__ order, bool o64, int64_t n,
    const int64_t* __restrict__ level_ptr, int64_t level_lo, int64_t level_hi,
    long long* flag) {
  const int g = (int)(threadIdx.x % G);
  for (int64_t l = level_lo; l < level_hi; ++l) {
    const int64_t base = level_ptr[l];
    const int64_t width = level_ptr[l + 1] - base;
    // ROWSCHED_CHAIN_THREADS is a multiple of G: a group is whole in or out
    for (int64_t ri = threadIdx.x / G; ri < width;
         ri += ROWSCHED_CHAIN_THREADS / G)
      ilu0_row<T, I, G>(indptr, indices, vals, diag_ptr, n,
                        order_at(order, o64, base + ri), g, flag);
    // all threads of the block reach this barrier every level (the loop
    // bounds are uniform); it orders this level's value stores before the
    // next level's loads of them within the workgroup
    __syncthreads();
  }
}

}  // namespace

// sched: the level schedule of rowsched.h, G used by wide and chain segments
// alike.
// flag: one int64 word on the device, pre-set by the caller to a value >= n;
// the smallest row index with a zero pivot is atomicMin'ed into it.
// All launches go to the current stream in schedule order; nothing here
// synchronises with the host.
void ilu0_factor_hip(at::Tensor indptr, at::Tensor indices, at::Tensor values,
                     at::Tensor diag_ptr, at::Tensor order,
                     at::Tensor level_ptr, at::Tensor sched, at::Tensor flag) {
  constexpr const char* OP = "ilu0_factor";
  const int64_t n = indptr.numel() - 1;
  const bool o64 = rowsched_check_operands(
      OP, values, {indptr, indices, diag_ptr, order, flag}, indptr, indices,
      values, order, level_ptr);
  TORCH_CHECK(diag_ptr.numel() == n && diag_ptr.scalar_type() == at::kLong &&
                  flag.scalar_type() == at::kLong && flag.numel() == 1,
              OP, ": bad analysis tensors");
  // (row indices, diag_ptr and lower columns are checked in the kernel)
  rowsched_check_schedule(OP, sched, n, level_ptr, true);
  if (n == 0 || sched.size(0) == 0) return;
  hipStream_t stream = cur_stream();
  DISPATCH_VALUES(values.scalar_type(), OP, [&] {
    using T = scalar_t;
    DISPATCH_INDEX(indices.scalar_type(), OP, [&] {
      const int64_t* ip = indptr.data_ptr<int64_t>();
      const index_t* ix = indices.data_ptr<index_t>();
      T* av = values.data_ptr<T>();
      const int64_t* dg = diag_ptr.data_ptr<int64_t>();
      const void* ord = order.data_ptr();
      const int64_t* lp = level_ptr.data_ptr<int64_t>();
      long long* fl = reinterpret_cast<long long*>(flag.data_ptr<int64_t>());
      rowsched_for_each(sched, false, [&](int64_t kind, int64_t lo,
                                          int64_t hi, int64_t G) {
        rowsched_with_group(G, [&](auto gg) {
          constexpr int GG = decltype(gg)::value;
          if (kind == 1) {
            hipLaunchKernelGGL((ilu0_chain_kernel<T, index_t, GG>), dim3(1),
                               dim3(ROWSCHED_CHAIN_THREADS), 0, stream, ip, ix,
                               av, dg, ord, o64, n, lp, lo, hi, fl);
          } else {
            const int64_t nrows = hi - lo;
            const int64_t blocks =
                (nrows * GG + ROWSCHED_BLOCK - 1) / ROWSCHED_BLOCK;
            hipLaunchKernelGGL((ilu0_level_kernel<T, index_t, GG>),
                               dim3(blocks), dim3(ROWSCHED_BLOCK), 0, stream,
                               ip, ix, av, dg, ord, o64, n, lo, nrows, fl);
          }
        });
      });
    });
  });
  SPARSE_CHECK_HIP(hipGetLastError());
}
