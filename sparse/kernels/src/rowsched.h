// Row schedules: what the level- and colour-scheduled kernels share
// (relax.hip: triangular solve and Gauss-Seidel sweeps; ilu0.hip).
//
// The analysis (sparse/rowsched.py) sorts the rows by an integer class, a
// dependency level or a colour, into `order`, cut at the class boundaries
// `level_ptr`, and hands the op a host-side schedule: a CPU int64 tensor
// (nseg, 4), one row per segment and launch,
//   wide  {0, row_lo, row_hi, G}      rows order[row_lo:row_hi] of ONE class,
//                                     G lanes per row
//   chain {1, level_lo, level_hi, G}  classes [level_lo, level_hi), each at
//                                     most ROWSCHED_CHAIN_THREADS rows, in
//                                     one launch of ONE workgroup (G is 0
//                                     where the chain kernel has no row
//                                     groups)
// All launches of a schedule go to the current stream in schedule order (or
// in reverse); nothing synchronises with the host, and there is no waiting
// between workgroups anywhere: ordering comes from kernel boundaries and,
// inside a chain kernel's single workgroup, from __syncthreads().
#pragma once

#include <initializer_list>

#include "common.h"

constexpr int ROWSCHED_BLOCK = 256;
constexpr int ROWSCHED_CHAIN_THREADS = 1024;

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

// The checks every op makes on its operands.  `target` is the tensor the op
// writes (x, or the factor's values); `others` are its remaining device
// operands, the four named ones included, level_ptr apart: that is an
// undefined tensor for an op without chain segments.  Returns whether
// `order` is int64.
inline bool rowsched_check_operands(const char* op, const at::Tensor& target,
                                    std::initializer_list<at::Tensor> others,
                                    const at::Tensor& indptr,
                                    const at::Tensor& indices,
                                    const at::Tensor& values,
                                    const at::Tensor& order,
                                    const at::Tensor& level_ptr) {
  TORCH_CHECK(target.is_cuda() && target.is_contiguous(), op, ": ",
              "the tensor written must be a contiguous device tensor");
  auto with_target = [&](const at::Tensor& t) {
    TORCH_CHECK(t.is_cuda() && t.device() == target.device() &&
                    t.is_contiguous(),
                op, ": operands must be contiguous and on one device");
  };
  for (const at::Tensor& t : others) with_target(t);
  if (level_ptr.defined()) with_target(level_ptr);
  const int64_t n = indptr.numel() - 1;
  TORCH_CHECK(n >= 0 && order.numel() == n &&
                  indices.numel() == values.numel() &&
                  indptr.scalar_type() == at::kLong &&
                  (indices.scalar_type() == at::kInt ||
                   indices.scalar_type() == at::kLong) &&
                  (!level_ptr.defined() ||
                   (level_ptr.scalar_type() == at::kLong &&
                    level_ptr.numel() >= 1)),
              op, ": bad analysis tensors");
  const bool o64 = order.scalar_type() == at::kLong;
  TORCH_CHECK(o64 || order.scalar_type() == at::kInt, op,
              ": order must be int32 or int64");
  return o64;
}

// Validate the whole schedule against the analysis sizes before the first
// launch: the kernels index order/level_ptr with these bounds unchecked.
// An undefined level_ptr: the op has no chain kernel and every chain segment
// is refused.  chain_groups: the op's chain kernel uses G as well.
inline void rowsched_check_schedule(const char* op, const at::Tensor& sched,
                                    int64_t n, const at::Tensor& level_ptr,
                                    bool chain_groups) {
  const int64_t nlevels = level_ptr.defined() ? level_ptr.numel() - 1 : -1;
  TORCH_CHECK(!sched.is_cuda() && sched.scalar_type() == at::kLong &&
                  sched.dim() == 2 && sched.size(1) == 4 &&
                  sched.is_contiguous(),
              op, ": sched must be a contiguous CPU int64 (nseg, 4)");
  const int64_t* sc = sched.data_ptr<int64_t>();
  for (int64_t s = 0; s < sched.size(0); ++s) {
    const int64_t kind = sc[4 * s], lo = sc[4 * s + 1], hi = sc[4 * s + 2],
                  G = sc[4 * s + 3];
    TORCH_CHECK(G == 1 || G == 8 || G == 64 || (kind == 1 && !chain_groups),
                op, ": bad row group");
    if (kind == 0) {
      TORCH_CHECK(0 <= lo && lo <= hi && hi <= n, op, ": bad wide segment");
    } else {
      TORCH_CHECK(kind == 1 && 0 <= lo && lo <= hi && hi <= nlevels, op,
                  ": bad chain segment");
    }
  }
}

// f(kind, lo, hi, G) for every non-empty segment of a validated schedule, in
// schedule order or in reverse; an empty segment (a colour no row has) is
// skipped: no launch.
template <typename F>
inline void rowsched_for_each(const at::Tensor& sched, bool reverse, F&& f) {
  const int64_t* sc = sched.data_ptr<int64_t>();
  const int64_t nseg = sched.size(0);
  for (int64_t i = 0; i < nseg; ++i) {
    const int64_t* r = sc + 4 * (reverse ? nseg - 1 - i : i);
    if (r[2] <= r[1]) continue;
    f(r[0], r[1], r[2], r[3]);
  }
}

// the run-time lanes per row (1, 8 or 64, validated) as a compile-time one:
// f(std::integral_constant<int, G>{})
template <typename F>
inline void rowsched_with_group(int64_t G, F&& f) {
  if (G == 1) f(std::integral_constant<int, 1>{});
  else if (G == 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 64>{});
}
