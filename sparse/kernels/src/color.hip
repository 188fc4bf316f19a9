// Greedy graph colouring by Jones-Plassmann rounds (sparse/gauss_seidel.py).
//
// The graph has one vertex per row of a structurally symmetric CSR pattern
// (the caller symmetrises); diagonal entries are skipped and duplicates are
// harmless.  Vertex i has the priority (h(i), i), h a 32-bit integer hash of
// i and the seed, and the result is DEFINED as the colouring of sequential
// greedy in decreasing priority: every vertex takes the smallest colour that
// none of its higher-priority neighbours has.
//
// One launch is one round over a compacted list of uncoloured vertices, one
// thread per vertex.  A vertex colours itself once ALL its higher-priority
// neighbours are coloured and looks at no other neighbour: lower-priority
// neighbours are never coloured before it, so this is the Jones-Plassmann
// rule (priority above every uncoloured neighbour, smallest colour absent
// among the coloured ones) without a dependence on when a store becomes
// visible.  colors[] goes from -1 to its final value in one 32-bit store, so
// a load returns either; seeing a neighbour's colour from the same launch
// only colours a vertex a round earlier, and the colours are the same
// however the rounds fall.  Nothing waits or spins: a vertex that is not
// ready is appended to the next round's list, whose length the host reads
// after the launch.  The highest-priority uncoloured vertex is always ready,
// so every round makes progress.
#include "common.h"

namespace {

constexpr int COLOR_BLOCK = 256;

__device__ __forceinline__ uint32_t color_hash(uint32_t i, uint32_t seed) {
  uint32_t x = i ^ seed;
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

template <typename I>
__global__ __launch_bounds__(COLOR_BLOCK) void color_round_kernel(
    const int64_t* __restrict__ indptr, const I* __restrict__ indices,
    const int64_t* __restrict__ work_in, int64_t nwork, uint32_t seed,
    int32_t* colors, int64_t* __restrict__ work_out,
    unsigned long long* count) {
  const int64_t tid = (int64_t)blockIdx.x * COLOR_BLOCK + threadIdx.x;
  if (tid >= nwork) return;
  const int64_t i = work_in[tid];
  const uint32_t hi = color_hash((uint32_t)i, seed);
  const int64_t ps = indptr[i], pe = indptr[i + 1];
  // smallest free colour through a 64-colour window [base, base + 64) that
  // moves up while it is full
  int32_t mine = -1;
  bool ready = true;
  for (int32_t base = 0; ready && mine < 0; base += 64) {
    uint64_t used = 0;
    for (int64_t p = ps; p < pe; ++p) {
      const int64_t j = (int64_t)indices[p];
      if (j == i) continue;
      const uint32_t hj = color_hash((uint32_t)j, seed);
      if (hj < hi || (hj == hi && j < i)) continue;  // lower priority
      // written by other workgroups of this launch: a relaxed device-scope
      // load, never a value the compiler or the L1 kept
      const int32_t c = __hip_atomic_load(colors + j, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
      if (c < 0) {
        ready = false;
        break;
      }
      const int32_t d = c - base;
      if (d >= 0 && d < 64) used |= 1ull << d;
    }
    if (ready && used != ~0ull) mine = base + __builtin_ctzll(~used);
  }
  if (mine >= 0) {
    __hip_atomic_store(colors + i, mine, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  } else {
    // at most nwork appends: work_out holds at least nwork entries
    work_out[atomicAdd(count, 1ull)] = i;
  }
}

}  // namespace

// One round over work_in[0:nwork].  colors (int32, -1 = uncoloured) is
// updated in place, the vertices left uncoloured are appended to work_out
// and counted in count[0], which the caller zeroes before the call and reads
// after it.  One launch on the current stream.
void color_round_hip(at::Tensor indptr, at::Tensor indices, at::Tensor work_in,
                     int64_t nwork, int64_t seed, at::Tensor colors,
                     at::Tensor work_out, at::Tensor count) {
  const int64_t n = indptr.numel() - 1;
  for (const at::Tensor& t : {indptr, indices, work_in, work_out, count})
    TORCH_CHECK(t.is_cuda() && t.device() == colors.device() &&
                    t.is_contiguous(),
                "color_round: operands must be contiguous and on one device");
  TORCH_CHECK(colors.is_cuda() && colors.is_contiguous() &&
                  colors.scalar_type() == at::kInt && colors.numel() == n,
              "color_round: colors must be a contiguous int32 (n,)");
  TORCH_CHECK(indices.scalar_type() == at::kInt ||
                  indices.scalar_type() == at::kLong,
              "color_round: indices must be int32 or int64");
  TORCH_CHECK(indptr.scalar_type() == at::kLong &&
                  work_in.scalar_type() == at::kLong &&
                  work_out.scalar_type() == at::kLong &&
                  count.scalar_type() == at::kLong && count.numel() == 1,
              "color_round: indptr, work lists and count must be int64");
  TORCH_CHECK(0 <= nwork && nwork <= n && work_in.numel() >= nwork &&
                  work_out.numel() >= nwork,
              "color_round: work lists shorter than nwork");
  if (nwork == 0) return;
  hipStream_t stream = cur_stream();
  const int64_t blocks = (nwork + COLOR_BLOCK - 1) / COLOR_BLOCK;
  DISPATCH_INDEX(indices.scalar_type(), "color_round", [&] {
    hipLaunchKernelGGL(
        (color_round_kernel<index_t>), dim3(blocks), dim3(COLOR_BLOCK), 0,
        stream, indptr.data_ptr<int64_t>(), indices.data_ptr<index_t>(),
        work_in.data_ptr<int64_t>(), nwork, (uint32_t)seed,
        colors.data_ptr<int32_t>(), work_out.data_ptr<int64_t>(),
        reinterpret_cast<unsigned long long*>(count.data_ptr<int64_t>()));
  });
  SPARSE_CHECK_HIP(hipGetLastError());
}
