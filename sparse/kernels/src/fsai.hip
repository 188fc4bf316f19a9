// FSAI numeric phase (sparse/fsai.py): one small dense Hermitian positive
// definite solve per row of the lower-triangular pattern P.
//
// For row i with the sorted columns J = P[i, :] (m entries, the last one i):
//   S = A[J, J]            only stored entries of A on and below the diagonal
//                          are read; an absent position counts as 0
//   S = C C^H              Cholesky, in place in the packed lower triangle
//   C^H g = e_m            one back substitution
//   G[i, J] = conj(g)      written into P's layout
// so (G A)[i, j] = 0 on the row's pattern, (G A G^H)[i, i] = 1 and the
// diagonal g_m = 1 / c_mm is real and positive.  A pivot that is not finite
// and > 0 is a breakdown: the row index goes into one int64 word by a vector
// atomicMin (the only atomic here) and the row is left unwritten.
//
// Rows are independent: no workgroup waits for another, and the host launches
// one kernel per length class over that class's row list (fsai.py builds the
// lists once per structure):
//   fsai_group_kernel<G>  m <= G, G = 4, 8, 16 or 64 lanes per row, 256 / G
//                         rows per 256-thread workgroup (G = 64: one wave,
//                         one row, a 64-thread workgroup).  S and the
//                         substitution vector live in LDS: G (G + 1) / 2 + G
//                         values per row, at most 34304 B per workgroup
//                         (complex128, G = 64), 38912 B (complex128, G = 16,
//                         16 rows).  Nothing opts into more than 64 KiB.
//   fsai_block_kernel     G < m <= FSAI_MAX_ROW: one 256-thread workgroup per
//                         row at a time, the same algorithm on a slot of a
//                         global-memory workspace (it stays in L2); the
//                         workgroups stride over the row list.
// A row group lies inside one wave, its lanes take the same branches (every
// trip count depends on the row only), and LDS serves one wave's accesses in
// issue order; between a store and another lane's load of it the group
// "barrier" is therefore a workgroup-scope fence pair with no s_barrier.  The
// workgroup-per-row kernel uses __syncthreads(); the loops around it are
// uniform over the workgroup.
//
// Work split inside a row, NL lanes (NL = G or 256), LW = min(NL, 64):
//   gather   lane a merges the sorted lower part of A's row J[a] against the
//            sorted J[0..a]
//   factor   right-looking; per column k the lanes scale the column, then
//            sub-group l / LW takes every (NL / LW)-th row a of the trailing
//            triangle and its LW lanes the columns b <= a
//   solve    column-oriented: lane a owns w[a]; per step one value is
//            published and every lane updates its own entries
#include <algorithm>

#include "common.h"

constexpr int FSAI_BLOCK = 256;

namespace {

template <typename T> struct RealOf { using type = T; };
template <typename T> struct RealOf<c10::complex<T>> { using type = T; };

template <typename T>
__device__ __forceinline__ T real_of(T v) { return v; }
template <typename T>
__device__ __forceinline__ T real_of(c10::complex<T> v) { return v.real(); }
template <typename T>
__device__ __forceinline__ T conj_of(T v) { return v; }
template <typename T>
__device__ __forceinline__ c10::complex<T> conj_of(c10::complex<T> v) {
  return {v.real(), -v.imag()};
}

// the barrier of the NL lanes working on one row
template <int NL>
__device__ __forceinline__ void row_sync() {
  if constexpr (NL > WAVE) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

__device__ __forceinline__ int tri(int a) { return a * (a + 1) / 2; }

// One row with NL lanes (l = lane in the group).  S: m (m + 1) / 2 + m values
// of storage private to the group (LDS or global): the packed lower triangle,
// row a at tri(a), then the substitution vector w.  Every lane of the group
// calls it with the same row and returns together.
template <typename T, typename I, int NL>
__device__ __forceinline__ void fsai_row(
    const int64_t* __restrict__ a_indptr, const I* __restrict__ a_indices,
    const T* __restrict__ a_values, const int64_t* __restrict__ p_indptr,
    const I* __restrict__ p_indices, T* __restrict__ g_values, int64_t n,
    int64_t i, int l, T* S, int max_m, long long* flag) {
  using R = typename RealOf<T>::type;
  constexpr int LW = NL < WAVE ? NL : WAVE;  // lanes across a trailing row
  constexpr int NS = NL / LW;                // trailing rows in flight
  const int64_t ps = p_indptr[i];
  const int64_t ml = p_indptr[i + 1] - ps;
  if (ml <= 0 || ml > max_m) return;  // the host sorted the rows by length
  const int m = static_cast<int>(ml);
  const I* J = p_indices + ps;
  T* w = S + tri(m);

  // 1. gather: lane a merges A's row J[a] (columns <= J[a]) against J[0..a]
  for (int a = l; a < m; a += NL) {
    const int64_t r = static_cast<int64_t>(J[a]);
    int64_t p = 0, pe = 0;
    if (r >= 0 && r < n) { p = a_indptr[r]; pe = a_indptr[r + 1]; }
    T* Sa = S + tri(a);
    for (int b = 0; b <= a; ++b) {
      const int64_t jb = static_cast<int64_t>(J[b]);
      while (p < pe && static_cast<int64_t>(a_indices[p]) < jb) ++p;
      Sa[b] = (p < pe && static_cast<int64_t>(a_indices[p]) == jb)
                  ? a_values[p] : ZeroOf<T>::value();
    }
    w[a] = ZeroOf<T>::value();
  }
  row_sync<NL>();

  // 2. S = C C^H in place.  `bad` is uniform over the group: every lane
  // reads the same pivot.
  bool bad = false;
  for (int k = 0; k < m; ++k) {
    const R d = real_of(S[tri(k) + k]);
    if (!(d > R(0)) || isinf(d)) { bad = true; break; }
    const R c = sqrt(d);
    row_sync<NL>();  // every lane has read the pivot
    for (int a = k + 1 + l; a < m; a += NL) S[tri(a) + k] = S[tri(a) + k] / c;
    if (l == 0) S[tri(k) + k] = T(c);
    row_sync<NL>();
    for (int a = k + 1 + l / LW; a < m; a += NS) {
      T* Sa = S + tri(a);
      const T sak = Sa[k];
      for (int b = k + 1 + l % LW; b <= a; b += LW)
        Sa[b] -= sak * conj_of(S[tri(b) + k]);
    }
    row_sync<NL>();
  }
  if (bad) {
    if (l == 0) atomicMin(flag, static_cast<long long>(i));
    return;
  }

  // 3. C^H g = e_m, column by column from the last; w starts as e_m, and
  // g[b] replaces w[b].  C[b][a], a < b, is row b of the packed triangle.
  if (l == (m - 1) % NL) w[m - 1] = T(R(1));
  row_sync<NL>();
  for (int b = m - 1; b >= 0; --b) {
    if (l == b % NL) w[b] = w[b] / real_of(S[tri(b) + b]);
    row_sync<NL>();
    const T gb = w[b];
    const T* Sb = S + tri(b);
    for (int a = l; a < b; a += NL) w[a] -= conj_of(Sb[a]) * gb;
    // w[b - 1] is complete in its owner lane: that lane made every update
  }
  row_sync<NL>();

  // 4. G[i, J] = conj(g)
  for (int a = l; a < m; a += NL) g_values[ps + a] = conj_of(w[a]);
}

// m <= G: G lanes per row; rows[0:nrows] is the class's row list
template <typename T, typename I, int G>
__global__ __launch_bounds__(G == WAVE ? WAVE : FSAI_BLOCK)
void fsai_group_kernel(
    const int64_t* __restrict__ a_indptr, const I* __restrict__ a_indices,
    const T* __restrict__ a_values, const int64_t* __restrict__ p_indptr,
    const I* __restrict__ p_indices, T* __restrict__ g_values,
    const int64_t* __restrict__ rows, int64_t nrows, int64_t n,
    long long* flag) {
  constexpr int THREADS = G == WAVE ? WAVE : FSAI_BLOCK;
  constexpr int RPB = THREADS / G;              // rows per workgroup
  constexpr int SLOT = G * (G + 1) / 2 + G;     // values per row
  __shared__ __align__(16) char raw[RPB * SLOT * sizeof(T)];
  T* lds = reinterpret_cast<T*>(raw);
  const int slot = threadIdx.x / G;
  const int64_t ri = (int64_t)blockIdx.x * RPB + slot;
  if (ri >= nrows) return;  // the G lanes of a group leave together
  const int64_t i = rows[ri];
  if (i < 0 || i >= n) return;
  fsai_row<T, I, G>(a_indptr, a_indices, a_values, p_indptr, p_indices,
                    g_values, n, i, threadIdx.x % G, lds + slot * SLOT, G,
                    flag);
}

// m <= max_m: one workgroup per row at a time on its own workspace slot of
// max_m (max_m + 1) / 2 + max_m values; the grid strides over the row list
template <typename T, typename I>
__global__ __launch_bounds__(FSAI_BLOCK) void fsai_block_kernel(
    const int64_t* __restrict__ a_indptr, const I* __restrict__ a_indices,
    const T* __restrict__ a_values, const int64_t* __restrict__ p_indptr,
    const I* __restrict__ p_indices, T* __restrict__ g_values,
    const int64_t* __restrict__ rows, int64_t nrows, int64_t n, T* work,
    int64_t slot_size, int max_m, long long* flag) {
  T* S = work + (int64_t)blockIdx.x * slot_size;
  for (int64_t ri = blockIdx.x; ri < nrows; ri += gridDim.x) {
    const int64_t i = rows[ri];  // uniform over the workgroup
    if (i >= 0 && i < n)
      fsai_row<T, I, FSAI_BLOCK>(a_indptr, a_indices, a_values, p_indptr,
                                 p_indices, g_values, n, i, threadIdx.x, S,
                                 max_m, flag);
    __syncthreads();  // the slot is reused by the next row
  }
}

}  // namespace

// G values of one length class.  rows: the class's row list (int64, device);
// lanes: 4, 8, 16 or 64 for the LDS kernels (every listed row has at most
// `lanes` pattern entries — longer ones are skipped, never overrun), 0 for
// the workspace kernel with rows of at most max_m entries; `work` then holds
// a whole number of slots of max_m (max_m + 1) / 2 + max_m values, one per
// workgroup.  flag: one int64 word preset >= n, receives the smallest row
// index that broke down.  Launches on the current stream; no host
// synchronisation.
void fsai_factor_hip(at::Tensor a_indptr, at::Tensor a_indices,
                     at::Tensor a_values, at::Tensor p_indptr,
                     at::Tensor p_indices, at::Tensor g_values,
                     at::Tensor rows, int64_t lanes, int64_t max_m,
                     at::Tensor work, at::Tensor flag) {
  constexpr const char* OP = "fsai_factor";
  for (const at::Tensor& t : {a_indptr, a_indices, a_values, p_indptr,
                              p_indices, g_values, rows, work, flag})
    TORCH_CHECK(t.is_cuda() && t.device() == g_values.device() &&
                    t.is_contiguous(),
                OP, ": operands must be contiguous and on one device");
  const int64_t n = a_indptr.numel() - 1;
  TORCH_CHECK(n >= 0 && p_indptr.numel() == n + 1 &&
                  a_indptr.scalar_type() == at::kLong &&
                  p_indptr.scalar_type() == at::kLong &&
                  rows.scalar_type() == at::kLong &&
                  flag.scalar_type() == at::kLong && flag.numel() == 1 &&
                  a_indices.numel() == a_values.numel() &&
                  p_indices.numel() == g_values.numel() &&
                  a_indices.scalar_type() == p_indices.scalar_type() &&
                  (a_indices.scalar_type() == at::kInt ||
                   a_indices.scalar_type() == at::kLong) &&
                  a_values.scalar_type() == g_values.scalar_type() &&
                  work.scalar_type() == g_values.scalar_type(),
              OP, ": bad operand types or sizes");
  TORCH_CHECK(lanes == 0 || lanes == 4 || lanes == 8 || lanes == 16 ||
                  lanes == 64,
              OP, ": lanes per row must be 0, 4, 8, 16 or 64");
  const int64_t nrows = rows.numel();
  if (n == 0 || nrows == 0) return;
  int64_t slot_size = 0, nslots = 0;
  if (lanes == 0) {
    TORCH_CHECK(max_m >= 1 && max_m <= (1 << 15), OP, ": bad max_m");
    slot_size = max_m * (max_m + 1) / 2 + max_m;
    nslots = std::min<int64_t>(work.numel() / slot_size, nrows);
    TORCH_CHECK(nslots >= 1, OP, ": workspace smaller than one slot");
  }
  hipStream_t stream = cur_stream();
  DISPATCH_VALUES(g_values.scalar_type(), OP, [&] {
    using T = scalar_t;
    DISPATCH_INDEX(a_indices.scalar_type(), OP, [&] {
      const int64_t* aip = a_indptr.data_ptr<int64_t>();
      const index_t* aix = a_indices.data_ptr<index_t>();
      const T* av = a_values.data_ptr<T>();
      const int64_t* pip = p_indptr.data_ptr<int64_t>();
      const index_t* pix = p_indices.data_ptr<index_t>();
      T* gv = g_values.data_ptr<T>();
      const int64_t* rl = rows.data_ptr<int64_t>();
      long long* fl = reinterpret_cast<long long*>(flag.data_ptr<int64_t>());
      auto group = [&](auto gg) {
        constexpr int G = decltype(gg)::value;
        constexpr int THREADS = G == WAVE ? WAVE : FSAI_BLOCK;
        const int64_t rpb = THREADS / G;
        hipLaunchKernelGGL((fsai_group_kernel<T, index_t, G>),
                           dim3((nrows + rpb - 1) / rpb), dim3(THREADS), 0,
                           stream, aip, aix, av, pip, pix, gv, rl, nrows, n,
                           fl);
      };
      if (lanes == 4) group(std::integral_constant<int, 4>{});
      else if (lanes == 8) group(std::integral_constant<int, 8>{});
      else if (lanes == 16) group(std::integral_constant<int, 16>{});
      else if (lanes == 64) group(std::integral_constant<int, 64>{});
      else
        hipLaunchKernelGGL((fsai_block_kernel<T, index_t>), dim3(nslots),
                           dim3(FSAI_BLOCK), 0, stream, aip, aix, av, pip,
                           pix, gv, rl, nrows, n, work.data_ptr<T>(),
                           slot_size, static_cast<int>(max_m), fl);
    });
  });
  SPARSE_CHECK_HIP(hipGetLastError());
}
