// CSR SpMV, nnz-split with LDS-staged products — MI355X (gfx950) native.
//
// Replaces reference CSR_SPMV_ROW_SPLIT (src/sparse/array/csr/spmv.cu:25-123,
// cuSPARSE-backed there).  Design for CDNA4 (measured on MI355X):
//  - each 256-thread block owns NNZ_PER_BLOCK consecutive nonzeros; values
//    and indices stream through 2-element vector loads (512B-1KB per wave
//    instruction, fully coalesced, read exactly once);
//  - ALL global loads (values, indices, x gathers, the block's indptr
//    segment) issue in one phase before the single barrier; the row-sum
//    phase then runs purely out of LDS — PMC showed the original
//    two-phase form 90% wave-parked because the sum phase had ~2 loads in
//    flight per wave (3.3 TB/s); this restructure lifts HBM pressure;
//  - XCD-aware block swizzle (common.h) keeps neighbouring nnz chunks on
//    one XCD's private L2 for x-gather reuse;
//  - rows cut by a block boundary produce one carry per block, combined by
//    a tiny fixup kernel (atomic-free main path);
//  - optional fused dot accumulates sum(p[r]*y[r]) per block (CG p·Ap);
//    the fixup kernel reduces the per-block partials.
//
// Below it: the padded-ELL and device-DIA mirrors and their row-pair kernel
// family (ell_spmv, ell_jacobi, dia_spmv incl. the residual, dia_jacobi,
// dia_spmv_bpdot), which share one window view, one accumulate loop per
// format, one block reduction and one host launch helper.  The DIA loop
// takes its plane values from a provider: the streamed planes, or plane
// constants plus a row mask for constant-coefficient stencils.
#include <type_traits>

#include "common.h"

namespace {

constexpr int BLK = 256;
constexpr int VT = 8;  // nnz per thread (2 vector quads)
constexpr int64_t NNZ_PER_BLOCK = (int64_t)BLK * VT;  // 2048

template <typename U>
struct alignas(4 * sizeof(U) <= 16 ? 4 * sizeof(U) : 16) Quad {
  U v[4];
};

// adjacent pair: one 2-element vector load / store per stream
template <typename U>
struct alignas(2 * sizeof(U) <= 16 ? 2 * sizeof(U) : 16) Pair {
  U a, b;
};

// 256-thread LDS tree sum of red[0..BLK) into red[0].  Every thread of the
// block must call it, with its own red[tid] already written.
template <typename T>
__device__ __forceinline__ void block_reduce_sum(T* red, int tid) {
  __syncthreads();
  for (int w = BLK / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
}

template <typename T, typename index_t, bool BETA_ZERO, bool FUSE_DOT>
__global__ __launch_bounds__(BLK) void spmv_kernel(
    const int64_t* __restrict__ indptr,  // m+1
    const index_t* __restrict__ indices,
    const T* __restrict__ vals,
    const T* __restrict__ x,  // window, indexed by (indices[p] - col_lo)
    T* __restrict__ y,
    int64_t m, int64_t nnz, int64_t col_lo, T beta,
    T* __restrict__ carry_val, int64_t* __restrict__ carry_row,
    const T* __restrict__ pvec,  // local p slab (rows align with y); FUSE_DOT
    T* __restrict__ dot_partial) {
  extern __shared__ char smem_raw[];
  T* prod = reinterpret_cast<T*>(smem_raw);  // NNZ_PER_BLOCK
  __shared__ __align__(16) char red_raw[BLK * sizeof(T)];
  T* red = reinterpret_cast<T*>(red_raw);

  const int64_t b = xcd_swizzle(blockIdx.x, gridDim.x);
  const int64_t s = b * NNZ_PER_BLOCK;
  const int64_t e = min(s + NNZ_PER_BLOCK, nnz);
  const int tid = threadIdx.x;

  // owned rows (redundant per-thread binary search; uniform -> broadcast)
  const int64_t ro0 = lb_i64(indptr, m, s);
  const int64_t ro1 = (e == nnz) ? m : lb_i64(indptr, m, e);

  // ---- phase 1: issue every global load ----------------------------------
  const bool full = (e - s) == NNZ_PER_BLOCK;
  if (full) {
    Quad<index_t> idx4[VT / 4];
    Quad<T> v4[VT / 4];
#pragma unroll
    for (int k = 0; k < VT / 4; ++k) {
      idx4[k] = *reinterpret_cast<const Quad<index_t>*>(
          &indices[s + tid * 4 + (int64_t)k * (4 * BLK)]);
    }
#pragma unroll
    for (int k = 0; k < VT / 4; ++k) {
      v4[k] = *reinterpret_cast<const Quad<T>*>(
          &vals[s + tid * 4 + (int64_t)k * (4 * BLK)]);
    }
    T xv[VT];
#pragma unroll
    for (int k = 0; k < VT / 4; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xv[k * 4 + j] = x[(int64_t)idx4[k].v[j] - col_lo];
      }
    }
#pragma unroll
    for (int k = 0; k < VT / 4; ++k) {
      Quad<T> pr;
#pragma unroll
      for (int j = 0; j < 4; ++j) pr.v[j] = v4[k].v[j] * xv[k * 4 + j];
      *reinterpret_cast<Quad<T>*>(&prod[tid * 4 + k * (4 * BLK)]) = pr;
    }
  } else {
    for (int64_t i = s + tid; i < e; i += BLK) {
      prod[i - s] = vals[i] * x[(int64_t)indices[i] - col_lo];
    }
  }
  __syncthreads();

  // ---- phase 2: per-thread row sums out of LDS ---------------------------
  T dacc = ZeroOf<T>::value();
  for (int64_t r = ro0 + tid; r < ro1; r += BLK) {
    const int64_t rs = indptr[r];
    const int64_t re = min(indptr[r + 1], e);
    T acc = ZeroOf<T>::value();
    for (int64_t p = rs; p < re; ++p) acc += prod[p - s];
    if (BETA_ZERO) {
      y[r] = acc;
    } else {
      acc = acc + beta * y[r];
      y[r] = acc;
    }
    if (FUSE_DOT) dacc += acc * pvec[r];
  }

  // continuation carry: items [s, cend) belong to row ro0-1
  bool has_carry = false;
  if (ro0 > 0) {
    int64_t cend;
    if (ro0 < m) {
      cend = min(indptr[ro0], e);
    } else {
      cend = e;
    }
    if (cend > s) {
      has_carry = true;
      T acc = ZeroOf<T>::value();
      for (int64_t p = s + tid; p < cend; p += BLK) acc += prod[p - s];
      red[tid] = acc;
      block_reduce_sum(red, tid);
      if (tid == 0) {
        carry_val[b] = red[0];
        carry_row[b] = ro0 - 1;
      }
    }
  }
  if (!has_carry && tid == 0) carry_row[b] = -1;

  if (FUSE_DOT) {
    __syncthreads();
    red[tid] = dacc;
    block_reduce_sum(red, tid);
    // per-block partial; one atomic per address would serialize at 163k
    // blocks, so the fixup kernel reduces these (nblocks/256 atomics).
    if (tid == 0) dot_partial[b] = red[0];
  }
}

template <typename T, bool FUSE_DOT>
__global__ void carry_fixup_kernel(const T* __restrict__ carry_val,
                                   const int64_t* __restrict__ carry_row,
                                   T* __restrict__ y, int64_t nblocks,
                                   const T* __restrict__ pvec,
                                   const T* __restrict__ dot_partial,
                                   T* __restrict__ dot_out) {
  __shared__ __align__(16) char red_raw[BLK * sizeof(T)];
  T* red = reinterpret_cast<T*>(red_raw);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  T dacc = ZeroOf<T>::value();
  if (i < nblocks) {
    int64_t r = carry_row[i];
    if (r >= 0) {
      T c = carry_val[i];
      atomic_add_any(&y[r], c);
      if (FUSE_DOT) dacc = c * pvec[r];
    }
    if (FUSE_DOT) dacc += dot_partial[i];
  }
  if (FUSE_DOT) {
    red[threadIdx.x] = dacc;
    block_reduce_sum(red, (int)threadIdx.x);
    if (threadIdx.x == 0) atomic_add_any(dot_out, red[0]);
  }
}

template <typename T>
__global__ void scale_kernel(T* y, int64_t n, T beta) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = beta * y[i];
}

}  // namespace

static void spmv_impl(at::Tensor indptr, at::Tensor indices, at::Tensor values,
                      at::Tensor x, at::Tensor y, int64_t col_lo, double beta,
                      const c10::optional<at::Tensor>& pvec,
                      const c10::optional<at::Tensor>& dot_out) {
  const int64_t m = indptr.numel() - 1;
  const int64_t nnz = values.numel();
  auto stream = cur_stream();
  const bool fuse_dot = pvec.has_value();
  DISPATCH_VALUES(values.scalar_type(), "spmv", [&] {
    using T = scalar_t;
    T betav = static_cast<T>(beta);
    if (nnz == 0) {
      if (beta == 0.0) {
        SPARSE_CHECK_HIP(hipMemsetAsync(y.data_ptr(), 0, m * sizeof(T), stream));
      } else if (m > 0) {
        hipLaunchKernelGGL(scale_kernel<T>, dim3((m + 255) / 256), dim3(256), 0,
                           stream, y.data_ptr<T>(), m, betav);
      }
      return;
    }
    const int64_t nblocks = (nnz + NNZ_PER_BLOCK - 1) / NNZ_PER_BLOCK;
    auto carry_val = at::empty({nblocks}, values.options());
    auto carry_row = at::empty({nblocks}, indptr.options());
    at::Tensor dot_partial;
    if (fuse_dot) dot_partial = at::empty({nblocks}, values.options());
    size_t smem = NNZ_PER_BLOCK * sizeof(T);
    const T* pp = fuse_dot ? pvec->data_ptr<T>() : nullptr;
    T* dpart = fuse_dot ? dot_partial.data_ptr<T>() : nullptr;
    T* dp = fuse_dot ? dot_out->data_ptr<T>() : nullptr;
    DISPATCH_INDEX(indices.scalar_type(), "spmv_idx", [&] {
      auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(nblocks), dim3(BLK), smem, stream,
                           indptr.data_ptr<int64_t>(), indices.data_ptr<index_t>(),
                           values.data_ptr<T>(), x.data_ptr<T>(), y.data_ptr<T>(),
                           m, nnz, col_lo, betav, carry_val.data_ptr<T>(),
                           carry_row.data_ptr<int64_t>(), pp, dpart);
      };
      if (beta == 0.0 && !fuse_dot) launch(spmv_kernel<T, index_t, true, false>);
      else if (beta == 0.0 && fuse_dot) launch(spmv_kernel<T, index_t, true, true>);
      else if (!fuse_dot) launch(spmv_kernel<T, index_t, false, false>);
      else launch(spmv_kernel<T, index_t, false, true>);
    });
    if (fuse_dot) {
      hipLaunchKernelGGL((carry_fixup_kernel<T, true>), dim3((nblocks + 255) / 256),
                         dim3(256), 0, stream, carry_val.data_ptr<T>(),
                         carry_row.data_ptr<int64_t>(), y.data_ptr<T>(), nblocks,
                         pp, dpart, dp);
    } else {
      hipLaunchKernelGGL((carry_fixup_kernel<T, false>), dim3((nblocks + 255) / 256),
                         dim3(256), 0, stream, carry_val.data_ptr<T>(),
                         carry_row.data_ptr<int64_t>(), y.data_ptr<T>(), nblocks,
                         pp, dpart, dp);
    }
  });
}

void spmv_hip(at::Tensor indptr, at::Tensor indices, at::Tensor values,
              at::Tensor x, at::Tensor y, int64_t col_lo, double beta) {
  spmv_impl(indptr, indices, values, x, y, col_lo, beta, c10::nullopt,
            c10::nullopt);
}

// fused q = A p ; dot_out += sum(p_local * q_local)
void spmv_dot_hip(at::Tensor indptr, at::Tensor indices, at::Tensor values,
                  at::Tensor x, at::Tensor y, at::Tensor pvec,
                  at::Tensor dot_out, int64_t col_lo) {
  spmv_impl(indptr, indices, values, x, y, col_lo, 0.0, pvec, dot_out);
}

// ---------------------------------------------------------------------------
// Padded-ELL fast path (column-major).  For row-uniform matrices (FD stencils,
// banded operators — the headline BASELINE workloads) the ELL mirror makes
// every value/index load perfectly coalesced with no indptr reads and no row
// search: measured 1.9x over the nnz-split CSR kernel on 5-pt Poisson fp64
// (0.94 ms vs 1.78 ms at nx=8192, ~6 TB/s effective; tools/spmv_bench.hip).
// The mirror is built once per matrix structure and cached on the csr_array.
namespace {

template <typename T, typename index_t>
__global__ void build_ell_kernel(const int64_t* __restrict__ indptr,
                                 const index_t* __restrict__ indices,
                                 const T* __restrict__ vals,
                                 index_t* __restrict__ eidx,
                                 T* __restrict__ evals, int64_t m, int64_t mp,
                                 int W, index_t pad_idx) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= mp) return;
  if (r >= m) {
    for (int k = 0; k < W; ++k) {
      eidx[(int64_t)k * mp + r] = pad_idx;
      evals[(int64_t)k * mp + r] = ZeroOf<T>::value();
    }
    return;
  }
  const int64_t rs = indptr[r];
  const int64_t cnt = indptr[r + 1] - rs;
  const index_t pi = cnt > 0 ? indices[rs] : pad_idx;
  for (int k = 0; k < W; ++k) {
    if (k < cnt) {
      eidx[(int64_t)k * mp + r] = indices[rs + k];
      evals[(int64_t)k * mp + r] = vals[rs + k];
    } else {
      eidx[(int64_t)k * mp + r] = pi;
      evals[(int64_t)k * mp + r] = ZeroOf<T>::value();
    }
  }
}

// scatter the CSR values into the padded diagonal planes (dvals assumed
// pre-zeroed): one thread per ROW walking its short slice — replaces an
// nnz-scale torch index_put_ in the mirror build (indexFuncLargeIndex was
// ~79 ms/call on the 931M-nnz 3-D GMG fine level)
template <typename T, typename index_t>
__global__ void build_dia_kernel(const int64_t* __restrict__ indptr,
                                 const index_t* __restrict__ indices,
                                 const T* __restrict__ vals,
                                 const int64_t* __restrict__ offs,
                                 T* __restrict__ dvals, int64_t m, int64_t mp,
                                 int W, int64_t row0) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const int64_t e = indptr[r + 1];
  for (int64_t p = indptr[r]; p < e; ++p) {
    const int64_t diag = (int64_t)indices[p] - (row0 + r);
    // offs sorted ascending, W <= 48: binary search
    int lo = 0, hi = W;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (offs[mid] < diag) lo = mid + 1; else hi = mid;
    }
    dvals[(int64_t)lo * mp + r] = vals[p];
  }
}

// Exact classification of the filled planes for DiaConstPlanes (below), on
// BIT PATTERNS: -0.0 is not +0.0 and a NaN constant is just a pattern.
//
// Pass 1: cbits[k] = the bits of some entry of plane k that are not +0.0
// (cbits pre-zeroed; a plane without one keeps 0).  blockIdx.y is the
// plane, the x grid strides over its rows.  The plain store races
// benignly: any winner will do, pass 2 is the check.
template <typename B>
__global__ void dia_plane_const_kernel(const B* __restrict__ dbits,
                                       B* __restrict__ cbits, int64_t mp) {
  const B* plane = dbits + (int64_t)blockIdx.y * mp;
  B seen = 0;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < mp;
       r += (int64_t)gridDim.x * blockDim.x) {
    const B b = plane[r];
    if (b != 0) seen = b;
  }
  if (seen != 0 && cbits[blockIdx.y] != seen) cbits[blockIdx.y] = seen;
}

// Pass 2, one thread per padded row: pack bit k = (entry k of the row is
// not +0.0) into the row's mask word, and clear *ok when such an entry
// differs from cbits[k].
template <typename B, typename M>
__global__ void dia_row_mask_kernel(const B* __restrict__ dbits,
                                    const B* __restrict__ cbits,
                                    M* __restrict__ mask,
                                    int32_t* __restrict__ ok, int64_t mp,
                                    int W) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= mp) return;
  uint32_t word = 0;
  bool same = true;
  for (int k = 0; k < W; ++k) {
    const B b = dbits[(int64_t)k * mp + r];
    if (b != 0) {
      word |= 1u << k;
      same = same && b == cbits[k];
    }
  }
  mask[r] = (M)word;
  if (!same && *ok != 0) *ok = 0;
}


// ---------------------------------------------------------------------------
// Row-pair core shared by the ELL and DIA kernels below.  Every thread owns
// rows r0, r0+1 (r0 even) and walks the W column-major planes; x comes from
// a window of up to three pieces.  Planes are single-use streams and take
// nt_load (common.h; measured on the 16384^2 5-pt DIA SpMV: 2.580 -> 2.474
// ms, tools/dia_nt_bench.hip); nt STORES measured slower, so outputs use
// plain stores.

// x window (halo_lo | own slab | halo_hi) — the own piece is the rank's x
// slab used IN PLACE (no per-SpMV self-copy).  SINGLE: the whole window is
// the own slab (ws=1 fast case) — no piece branch.
template <typename T>
struct XWindow {
  const T* hlo;
  const T* own;
  const T* hhi;
  int64_t nlo, nown, wsize;

  // gather at window-relative index idx (ELL)
  template <bool SINGLE>
  __device__ __forceinline__ T at(int64_t idx) const {
    if (SINGLE) return own[idx];
    if (idx < nlo) return hlo[idx];
    idx -= nlo;
    if (idx < nown) return own[idx];
    return hhi[idx - nown];
  }

  // address of window-relative index idx, chosen by selects
  __device__ __forceinline__ const T* flat_ptr(int64_t idx) const {
    const bool lo = idx < nlo, mid = idx < nlo + nown;
    const T* base = lo ? hlo : (mid ? own : hhi);
    return base + (idx - (lo ? 0 : (mid ? nlo : nlo + nown)));
  }

  // adjacent pair [c0, c0+1], clamped at the window edges (DIA: padded
  // plane entries are 0, so a clamped load is safe).  Rows r0, r0+1 of one
  // thread access consecutive columns on every diagonal, and the alignment
  // parity (c0 & 1) is uniform per diagonal (r0 is even), so the SINGLE
  // interior fast path is one 16B load (even parity) or two scalars (odd) —
  // halving the load-issue count that bounds the DIA kernels (profiled
  // 4.6 TB/s issue-bound vs 6.0 achievable).
  //
  // FLAT: the same two elements through clamped addresses and selects, no
  // branch — for callers that batch the pairs of several diagonals (a
  // branchy pair makes the compiler drain the earlier loads before it
  // forms the next addresses).
  template <bool SINGLE, bool FLAT = false>
  __device__ __forceinline__ void pair(int64_t c0, T& x0, T& x1) const {
    if (FLAT) {
      const int64_t i0 = min(max(c0, (int64_t)0), wsize - 1);
      const int64_t i1 = min(max(c0 + 1, (int64_t)0), wsize - 1);
      if (SINGLE) {
        x0 = own[i0];
        x1 = own[i1];
      } else {
        x0 = *flat_ptr(i0);
        x1 = *flat_ptr(i1);
      }
      return;
    }
    if (SINGLE) {
      if (c0 >= 0 && c0 + 1 < wsize) {
        if ((c0 & 1) == 0) {
          const Pair<T> t = *reinterpret_cast<const Pair<T>*>(&own[c0]);
          x0 = t.a;
          x1 = t.b;
        } else {
          x0 = own[c0];
          x1 = own[c0 + 1];
        }
      } else {
        x0 = own[min(max(c0, (int64_t)0), wsize - 1)];
        x1 = own[min(max(c0 + 1, (int64_t)0), wsize - 1)];
      }
    } else {
      x0 = at<false>(min(max(c0, (int64_t)0), wsize - 1));
      x1 = at<false>(min(max(c0 + 1, (int64_t)0), wsize - 1));
    }
  }
};

// a0, a1 += sum_k evals[k][r0, r0+1] * x[eidx[k][r0, r0+1] - col_lo]
template <typename T, typename index_t, bool SINGLE>
__device__ __forceinline__ void ell_accumulate(
    const index_t* __restrict__ eidx, const T* __restrict__ evals, int W,
    int64_t mp, int64_t r0, int64_t col_lo, const XWindow<T>& win, T& a0,
    T& a1) {
  for (int k = 0; k < W; ++k) {
    const int64_t base = (int64_t)k * mp + r0;
    Pair<index_t> ii;
    ii.a = nt_load(&eidx[base]);
    ii.b = nt_load(&eidx[base + 1]);
    Pair<T> vv;
    vv.a = nt_load(&evals[base]);
    vv.b = nt_load(&evals[base + 1]);
    a0 += vv.a * win.template at<SINGLE>((int64_t)ii.a - col_lo);
    a1 += vv.b * win.template at<SINGLE>((int64_t)ii.b - col_lo);
  }
}

// Plane-value providers of the DIA core: rows(r0) is the thread's view of
// rows r0, r0+1 (r0 even) and rows(r0).at(k, v0, v1) yields their entries
// on plane k.
//
// DiaPlanes streams the (W, mp) column-major padded planes.
template <typename T>
struct DiaPlanes {
  static constexpr int kBatch = 1;  // diagonals per load batch (accumulate)
  const T* __restrict__ dvals;
  int64_t mp;

  struct Rows {
    const T* __restrict__ p;
    int64_t mp;
    __device__ __forceinline__ void at(int k, T& v0, T& v1) const {
      const int64_t base = (int64_t)k * mp;
      v0 = nt_load(&p[base]);
      v1 = nt_load(&p[base + 1]);
    }
  };
  __device__ __forceinline__ Rows rows(int64_t r0) const {
    return {dvals + r0, mp};
  }
};

// DiaConstPlanes serves a mirror whose every plane k holds, bit for bit,
// only +0.0 and one constant c[k] (constant-coefficient stencils): the W
// constants plus one row-major mask word per row (bit k = plane k has c[k]
// in this row; padded rows 0) replace the W values per row.  A thread
// fetches both rows' words in one naturally aligned load (a wave reads one
// contiguous 128 * sizeof(M) bytes) and c[k] is wave-uniform like offs[k].
// A masked-out entry yields the same +0.0 the plane would hold, so the
// accumulation — x loads included — is the streamed one and the results
// are bit-identical to DiaPlanes.
template <int BYTES> struct UIntOf;
template <> struct UIntOf<2> { using type = uint16_t; };
template <> struct UIntOf<4> { using type = uint32_t; };
template <> struct UIntOf<8> { using type = uint64_t; };

template <typename T, typename M>
struct DiaConstPlanes {
  static constexpr int kBatch = 8;
  const T* __restrict__ cvals;  // W plane constants
  const M* __restrict__ mask;   // mp row mask words

  struct Rows {
    const T* __restrict__ c;
    uint32_t m0, m1;
    __device__ __forceinline__ void at(int k, T& v0, T& v1) const {
      const T ck = c[k];
      const uint32_t bit = 1u << k;
      v0 = (m0 & bit) ? ck : T(0);
      v1 = (m1 & bit) ? ck : T(0);
    }
  };
  __device__ __forceinline__ Rows rows(int64_t r0) const {
    using M2 = typename UIntOf<2 * sizeof(M)>::type;
    const M2 w = nt_load(reinterpret_cast<const M2*>(&mask[r0]));
    return {cvals, (uint32_t)(M)w, (uint32_t)(w >> (8 * sizeof(M)))};
  }
};

// a + v * x.  Real types: in ONE rounding, spelled out in every DIA kernel
// — contraction would make the same of `a += v * x`, but left to the
// compiler the vectorizer may instead split an fp32 row pair into a packed
// multiply and an add in one instantiation and not in another, and the DIA
// kernels promise the same bits from both value sources.
template <typename T>
__device__ __forceinline__ T fmadd(T v, T x, T a) {
  if constexpr (std::is_same_v<T, float>) {
    return __builtin_fmaf(v, x, a);
  } else if constexpr (std::is_same_v<T, double>) {
    return __builtin_fma(v, x, a);
  } else {
    return a + v * x;
  }
}

// a0, a1 += sum_k plane[k][r0, r0+1] * xpair(cbase + offs[k]); cbase is the
// window-relative column of row r0 on the main diagonal and xpair(c0, x0,
// x1) yields the x pair at window columns c0, c0+1.
template <typename T, typename Planes, typename XPair>
__device__ __forceinline__ void dia_accumulate(
    const Planes& planes, const int64_t* __restrict__ offs, int W, int64_t r0,
    int64_t cbase, XPair xpair, T& a0, T& a1) {
  const auto rows = planes.rows(r0);
  constexpr int U = Planes::kBatch;
  if constexpr (U == 1) {
    for (int k = 0; k < W; ++k) {
      T v0, v1;
      rows.at(k, v0, v1);
      T x0, x1;
      xpair(cbase + offs[k], x0, x1);
      a0 = fmadd(v0, x0, a0);
      a1 = fmadd(v1, x1, a1);
    }
  } else {
    // fetch the x pairs of up to U diagonals before the first use, then
    // accumulate in the same k order (same arithmetic, same bits): without
    // a plane stream a thread has only its x loads to keep in flight, and
    // one diagonal per round trip leaves the kernel latency-bound
    for (int k = 0; k < W; k += U) {
      T x0[U], x1[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        if (k + j < W) xpair(cbase + offs[k + j], x0[j], x1[j]);
      }
#pragma unroll
      for (int j = 0; j < U; ++j) {
        if (k + j < W) {
          T v0, v1;
          rows.at(k + j, v0, v1);
          a0 = fmadd(v0, x0[j], a0);
          a1 = fmadd(v1, x1[j], a1);
        }
      }
    }
  }
}

// rows r0, r0+1 of an output: one pair store, or the lone tail row
template <typename T>
__device__ __forceinline__ void store_pair_or_tail(T* __restrict__ dst,
                                                   int64_t r0, int64_t m,
                                                   int64_t rhi, T v0, T v1) {
  if (r0 + 1 < min(m, rhi)) {
    *reinterpret_cast<Pair<T>*>(&dst[r0]) = Pair<T>{v0, v1};
  } else if (r0 < m) {
    dst[r0] = v0;
  }
}

// x_out = x + omega * dinv * (b - A x) for rows r0, r0+1 (a0, a1 = A x)
template <typename T>
__device__ __forceinline__ void jacobi_update(
    const T* __restrict__ xloc, const T* __restrict__ b,
    const T* __restrict__ dinv, T* __restrict__ xout, T omega, int64_t r0,
    int64_t m, int64_t rhi, T a0, T a1) {
  if (r0 + 1 < min(m, rhi)) {
    const Pair<T> xv = *reinterpret_cast<const Pair<T>*>(&xloc[r0]);
    const Pair<T> bv = *reinterpret_cast<const Pair<T>*>(&b[r0]);
    const Pair<T> dv = *reinterpret_cast<const Pair<T>*>(&dinv[r0]);
    *reinterpret_cast<Pair<T>*>(&xout[r0]) =
        Pair<T>{fmadd(omega * dv.a, bv.a - a0, xv.a),
                fmadd(omega * dv.b, bv.b - a1, xv.b)};
  } else if (r0 < m) {
    xout[r0] = fmadd(omega * dinv[r0], b[r0] - a0, xloc[r0]);
  }
}

// fused-dot epilogue: every thread of the block contributes d; slot
// blockIdx.x of dot_partial receives the block sum (one barrier, common.h)
template <typename T>
__device__ __forceinline__ void block_dot_partial(T d,
                                                  T* __restrict__ dot_partial) {
  const T part[1] = {d};
  const T sum = block_sums_256(part);
  if (threadIdx.x == 0) dot_partial[blockIdx.x] = sum;
}

// [rbase, rhi): row sub-range (rbase even) — the interior/boundary split
// that overlaps halo exchange with interior compute at ws>1 (ell_spmv,
// dia_spmv, dia_jacobi share this contract)
template <typename T, typename index_t, bool FUSE_DOT, bool SINGLE>
__global__ __launch_bounds__(BLK) void ell_spmv_kernel(
    const index_t* __restrict__ eidx, const T* __restrict__ evals,
    const XWindow<T> win, T* __restrict__ y, const T* __restrict__ pvec,
    T* __restrict__ dot_partial, int64_t m, int64_t mp, int W, int64_t col_lo,
    int64_t rbase, int64_t rhi) {
  const int64_t r0 = rbase + 2 * ((int64_t)blockIdx.x * BLK + threadIdx.x);
  T a0 = ZeroOf<T>::value(), a1 = ZeroOf<T>::value();
  if (r0 < rhi) {
    ell_accumulate<T, index_t, SINGLE>(eidx, evals, W, mp, r0, col_lo, win,
                                       a0, a1);
    store_pair_or_tail(y, r0, m, rhi, a0, a1);
  }
  if (FUSE_DOT) {
    T d = ZeroOf<T>::value();
    if (r0 < min(m, rhi)) d += a0 * pvec[r0];
    if (r0 + 1 < min(m, rhi)) d += a1 * pvec[r0 + 1];
    block_dot_partial(d, dot_partial);
  }
}

// Fused weighted-Jacobi sweep on the ELL mirror:
//   x_out[r] = x[r] + omega * dinv[r] * (b[r] - (A x)[r])
// One pass over A + 4 vector streams instead of spmv + 2 elementwise
// kernels (the GMG/AMG smoother, reference WeightedJacobi gmg.py:247-285).
template <typename T, typename index_t, bool SINGLE>
__global__ __launch_bounds__(BLK) void ell_jacobi_kernel(
    const index_t* __restrict__ eidx, const T* __restrict__ evals,
    const XWindow<T> win, const T* __restrict__ xloc,
    const T* __restrict__ b, const T* __restrict__ dinv,
    T* __restrict__ xout, int64_t m, int64_t mp, int W, int64_t col_lo,
    T omega) {
  const int64_t r0 = 2 * ((int64_t)blockIdx.x * BLK + threadIdx.x);
  if (r0 >= mp) return;
  T a0 = ZeroOf<T>::value(), a1 = ZeroOf<T>::value();
  ell_accumulate<T, index_t, SINGLE>(eidx, evals, W, mp, r0, col_lo, win, a0,
                                     a1);
  jacobi_update(xloc, b, dinv, xout, omega, r0, m, m, a0, a1);
}

// Device-DIA fast path: when the matrix has few distinct diagonals
// (col - row values), store ONLY the padded value planes column-major plus
// the W offsets — the index stream disappears (12 -> 8 B/nnz for
// fp64+int32).  Invalid/padded entries hold 0 and their x loads are clamped
// into the window.  When every plane is one constant wherever it is not
// +0.0 (constant-coefficient stencils: Poisson, banded, the GMG fine
// levels) the planes themselves disappear too: the kernels take their
// values from W constants and one mask word per row (DiaConstPlanes;
// classified exactly at mirror build, dia_classify) — 1-4 B/row instead of
// W values, same bits out.  Every kernel below is instantiated for both
// value sources.  Reference context: the dia format (sparse/dia.py) is a
// host/conversion format there; here it is the SpMV execution format for
// banded operators (Poisson, dot_microbenchmark).
template <typename T, typename Planes, bool FUSE_DOT, bool SINGLE,
          bool RESID = false>
__global__ __launch_bounds__(BLK) void dia_spmv_kernel(
    const Planes planes,               // plane values (provider, above)
    const int64_t* __restrict__ offs,  // W diagonal offsets
    const XWindow<T> win, T* __restrict__ y, const T* __restrict__ pvec,
    T* __restrict__ dot_partial, int64_t m, int64_t mp, int W, int64_t col_lo,
    int64_t row0, int64_t rbase, int64_t rhi) {
  const int64_t r0 = rbase + 2 * ((int64_t)blockIdx.x * BLK + threadIdx.x);
  T a0 = ZeroOf<T>::value(), a1 = ZeroOf<T>::value();
  if (r0 < rhi) {
    dia_accumulate(
        planes, offs, W, r0, row0 + r0 - col_lo,
        [&](int64_t c0, T& x0, T& x1) {
          win.template pair<SINGLE, Planes::kBatch != 1>(c0, x0, x1);
        },
        a0, a1);
    if (!RESID) {
      store_pair_or_tail(y, r0, m, rhi, a0, a1);
    } else if (r0 + 1 < min(m, rhi)) {
      // y = b - A x (pvec carries b): the V-cycle residual fused into
      // the SpMV — saves the separate 3-pass pointwise kernel
      const Pair<T> bv = *reinterpret_cast<const Pair<T>*>(&pvec[r0]);
      *reinterpret_cast<Pair<T>*>(&y[r0]) = Pair<T>{bv.a - a0, bv.b - a1};
    } else if (r0 < m) {
      y[r0] = pvec[r0] - a0;
    }
  }
  if (FUSE_DOT) {
    T d = ZeroOf<T>::value();
    if (r0 < min(m, rhi)) d = fmadd(a0, pvec[r0], d);
    if (r0 + 1 < min(m, rhi)) d = fmadd(a1, pvec[r0 + 1], d);
    block_dot_partial(d, dot_partial);
  }
}

template <typename T, typename Planes, bool SINGLE>
__global__ __launch_bounds__(BLK) void dia_jacobi_kernel(
    const Planes planes, const int64_t* __restrict__ offs,
    const XWindow<T> win, const T* __restrict__ xloc,
    const T* __restrict__ b, const T* __restrict__ dinv,
    T* __restrict__ xout, int64_t m, int64_t mp, int W, int64_t col_lo,
    int64_t row0, T omega, int64_t rbase, int64_t rhi) {
  const int64_t r0 = rbase + 2 * ((int64_t)blockIdx.x * BLK + threadIdx.x);
  if (r0 >= rhi) return;
  T a0 = ZeroOf<T>::value(), a1 = ZeroOf<T>::value();
  dia_accumulate(
      planes, offs, W, r0, row0 + r0 - col_lo,
      [&](int64_t c0, T& x0, T& x1) {
        win.template pair<SINGLE, Planes::kBatch != 1>(c0, x0, x1);
      },
      a0, a1);
  jacobi_update(xloc, b, dinv, xout, omega, r0, m, rhi, a0, a1);
}

// Fully-fused CG K1 on the DIA mirror (two-kernel CG iteration):
//   p_new = r + beta * p_old   (beta = *beta_num / *beta_den, device scalars)
//   q     = A p_new
//   pq    = p_new . q          (per-block partials)
// p_new at neighbor columns is recomputed on the fly from the r / p_old
// windows (deterministic IEEE => identical to the stored value), so the
// separate p-update pass over 3 vector streams disappears.  p_old and
// p_new MUST be distinct buffers (double-buffered by the caller).
// Reference context: this is the MI355X fusion of the reference CG loop's
// AXPBY + SpMV + dot task chain (linalg.py:499-565).
template <typename T, typename Planes, bool SINGLE>
__global__ __launch_bounds__(BLK) void dia_spmv_bpdot_kernel(
    const Planes planes, const int64_t* __restrict__ offs,
    const XWindow<T> rwin, const XWindow<T> pwin, T* __restrict__ pnew,
    T* __restrict__ q, const T* __restrict__ beta_num,
    const T* __restrict__ beta_den, T* __restrict__ dot_partial, int64_t m,
    int64_t mp, int W, int64_t col_lo, int64_t row0) {
  const T beta = (*beta_num) / (*beta_den);
  const int64_t r0 = 2 * ((int64_t)blockIdx.x * BLK + threadIdx.x);
  T a0 = ZeroOf<T>::value(), a1 = ZeroOf<T>::value();
  T p0 = ZeroOf<T>::value(), p1 = ZeroOf<T>::value();
  if (r0 < mp) {
    auto pnew_pair = [&](int64_t c0, T& x0, T& x1) {
      T r0v, r1v, p0v, p1v;
      rwin.template pair<SINGLE, Planes::kBatch != 1>(c0, r0v, r1v);
      pwin.template pair<SINGLE, Planes::kBatch != 1>(c0, p0v, p1v);
      x0 = fmadd(beta, p0v, r0v);
      x1 = fmadd(beta, p1v, r1v);
    };
    // window index of own row r0: row0 - col_lo + r0
    const int64_t cbase = row0 + r0 - col_lo;
    dia_accumulate(planes, offs, W, r0, cbase, pnew_pair, a0, a1);
    // own-row p_new (same formula as the window recompute => identical fp);
    // p1 of a lone tail row is a clamped load that is never used
    pnew_pair(cbase, p0, p1);
    store_pair_or_tail(pnew, r0, m, m, p0, p1);
    store_pair_or_tail(q, r0, m, m, a0, a1);
  }
  T d = ZeroOf<T>::value();
  if (r0 < m) d = fmadd(a0, p0, d);
  if (r0 + 1 < m) d = fmadd(a1, p1, d);
  block_dot_partial(d, dot_partial);
}

// ---------------------------------------------------------------------------
// Constant-plane kernels.  Without a plane stream a wave moves ~2 KB per trip
// through its dependent chain (mask -> x -> operands -> reduction), so these
// kernels are bound by latency per wave and by the number of vector loads a
// wave issues, not by HBM (profiles/dia_core_chain_profile.md,
// profiles/dia_lane_exchange_profile.md).  dia_const_rows shortens the chain:
//  - a thread owns R row pairs, block-strided (pair j of thread t is rows
//    rb + 2 * (t + j * BLK), so every wave instruction still touches one
//    contiguous run) and issues the loads of all of them — mask words, the x
//    pairs of every diagonal, the caller's operands — before the first use;
//  - offs[] and c[] are fetched up front into registers; W <= 8 (the u8
//    mask) is a compile-time WC so the diagonal loop unrolls fully and no
//    scalar wait sits between the x loads;
//  - a block whose rows are all below min(m, rhi) and whose columns all lie
//    in the own piece of the window (block-uniform test, scalar branch) uses
//    plain addresses (dia_const_interior): one 16-byte load per x pair where
//    the pair is aligned (uniform per diagonal, see XWindow::pair), two
//    8-byte loads otherwise, and no load at all for an unaligned pair next
//    to an aligned one (lane exchange, below) or for a row operand that is
//    the x slab itself.  The 5-pt stencil's fused p . A p so issues 10 loads
//    per row-pair couple instead of 14.
//    The other (edge) blocks run the clamped dia_accumulate above.
// Per-row arithmetic is dia_accumulate's (a += v_k * x_k, k ascending): same
// bits as the streamed planes.  The fused dot keeps ONE partial per 2 * BLK
// rows, i.e. R per block, summed exactly like a block of the streamed
// kernel: both value sources return the same dot bits, whatever R is.
// R: with the lane exchange in, R = 4 beats R = 2 on the 16384^2 5-pt SpMV
// and its fused dot although it halves the occupancy (102 VGPRs, 4
// waves/SIMD against 57 and 8); the residual and the Jacobi sweep carry
// more operands per row (135 VGPRs at R = 4) and lose 7 % on the GMG
// V-cycle there, so they stay at 2 (profiles/dia_lane_exchange_bench.txt).
// More than 5 diagonals were not measured at R = 4 (W = 8 would need about
// 150 VGPRs) and stay at 2 as well.
constexpr int kDiaPairs = 4;        // R of dia_spmv and dia_spmv_dot, W <= 5
constexpr int kDiaSmoothPairs = 2;  // R of dia_residual, dia_jacobi, W > 5
constexpr int kDiaBpdotPairs = 1;   // R of dia_spmv_bpdot (two windows)

// R of dia_const_spmv_kernel
constexpr int dia_spmv_pairs(int WC, bool resid) {
  return (!resid && WC >= 1 && WC <= 5) ? kDiaPairs : kDiaSmoothPairs;
}

// v of the next higher / lower lane of the wave (the last / first lane keeps
// its own): one v_mov_b32 with a DPP wave shift per 32 bits.  Every lane of
// the wave must be active.
template <int CTRL, typename T>
__device__ __forceinline__ T lane_shift(T v) {
  static_assert(sizeof(T) % 4 == 0, "whole dwords expected");
  int w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 4); ++i) {
    w[i] = __builtin_amdgcn_update_dpp(w[i], w[i], CTRL, 0xf, 0xf, false);
  }
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}
template <typename T>
__device__ __forceinline__ T lane_above(T v) {
  return lane_shift<0x130>(v);  // wave_shl:1
}
template <typename T>
__device__ __forceinline__ T lane_below(T v) {
  return lane_shift<0x138>(v);  // wave_shr:1
}

// Lane exchange.  Diagonals at consecutive offsets read overlapping pairs:
// with (A_t, B_t) the pair of offset d in lane t, the pair of d + 1 is
// (B_t, A_{t+1}) and that of d - 1 is (B_{t-1}, A_t).  Pairs alternate
// between aligned and unaligned along such a run, so the unaligned ones
// (a 16-byte load across two lines) are not loaded but taken from the
// aligned neighbour's registers with a wave shift.  Only the wave's last
// (first) lane lacks A_{t+1} (B_{t-1}); it fetches that one element with a
// load in which no other lane is active.
// ADJ is the compile-time plan: bit i says offs[i + 1] == offs[i] + 1, and
// the set bits form one run (dispatch_dia_wc picks it from the mirror's
// adjacency word; the kernel checks it against offs[] and sends a block
// whose offsets disagree down the clamped path).  P is the run-time parity
// of the run's first pair (0 aligned, 1 unaligned; -1 no exchange: ADJ == 0,
// or two windows of different parity), resolved by one block-uniform branch
// around the whole interior body so that every source below is static.
enum DiaSrc { kDiaLoad, kDiaLoadAligned, kDiaFromLo, kDiaFromHi };

template <uint32_t ADJ>
struct DiaRun {
  static constexpr int start = ADJ ? __builtin_ctz(ADJ) : 0;
  static constexpr int len = ADJ ? __builtin_popcount(ADJ) + 1 : 1;
  static_assert(ADJ == 0 || (ADJ >> start) + 1 == (1u << (len - 1)),
                "the adjacent diagonals must form one run");
  // where diagonal i's pair comes from
  __host__ __device__ static constexpr DiaSrc src(int P, int i) {
    const int q = i - start;
    if (ADJ == 0 || P < 0 || q < 0 || q >= len) return kDiaLoad;
    if (((P + q) & 1) == 0) return kDiaLoadAligned;
    return q > 0 ? kDiaFromLo : kDiaFromHi;  // q == 0 borrows from q == 1
  }
  // diagonals i (from hi) and i + 2 (from lo) share one two-lane load
  __host__ __device__ static constexpr bool two(int P, int i) {
    return src(P, i) == kDiaFromHi && len >= 3;
  }
};

// Interior block of dia_const_rows: rows rb .. rb + S - 1 are all below
// min(m, rhi) and all their columns lie in the own piece, so addresses are
// plain.  own[w] + cb is the address of row rb's main-diagonal column.
template <int WC, int R, int NWIN, uint32_t ADJ, int P, typename T,
          typename M, typename Comb, typename Pre, typename Post>
__device__ __forceinline__ void dia_const_interior(
    const DiaConstPlanes<T, M>& planes, const int64_t* __restrict__ offs,
    int W, const T* const* own, Comb comb, bool ctr, int64_t rb,
    int64_t cb, int64_t (&o)[WC ? WC : 8], T (&c)[WC ? WC : 8], Pre pre,
    Post post) {
  constexpr int KB = WC ? WC : 8;
  using Run = DiaRun<ADJ>;
  using M2 = typename UIntOf<2 * sizeof(M)>::type;
  const int64_t t2 = 2 * (int64_t)threadIdx.x;
  const int lane = threadIdx.x & 63;
  M2 mw[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    mw[j] = nt_load(
        reinterpret_cast<const M2*>(planes.mask + rb + t2 + j * 2 * BLK));
  }
  T a[R][2];
  Pair<T> cx[R];  // the offset-0 pair, for post (ctr)
#pragma unroll
  for (int j = 0; j < R; ++j) {
    a[j][0] = a[j][1] = ZeroOf<T>::value();
    cx[j] = Pair<T>{T(0), T(0)};
  }
  for (int k0 = 0; k0 < W; k0 += KB) {
    if (k0 > 0) {
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        if (k0 + i < W) {
          o[i] = offs[k0 + i];
          c[i] = planes.cvals[k0 + i];
        }
      }
    }
    T xv[NWIN][R][KB][2];
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      if (k0 + i < W) {
        const DiaSrc src = Run::src(P, i);
#pragma unroll
        for (int w = 0; w < NWIN; ++w) {
          // block-uniform address of the block's first column
          const T* ub = own[w] + (cb + o[i]);
          const bool aligned =
              src == kDiaLoadAligned ||
              (reinterpret_cast<uintptr_t>(ub) % sizeof(Pair<T>)) == 0;
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const T* p = ub + t2 + j * 2 * BLK;
            if (src == kDiaFromHi) {
              // element 0 of the first lane; p[3] is element 1 of diagonal
              // i + 2's pair, which the last lane lacks
              if (lane == 0 || (Run::two(P, i) && lane == 63)) {
                xv[w][j][i][0] = p[lane == 0 ? 0 : 3];
              }
            } else if (src == kDiaFromLo) {
              if (!(i >= 2 && Run::two(P, i - 2)) && lane == 63) {
                xv[w][j][i][0] = p[1];
              }
            } else if (aligned) {
              const Pair<T> t = *reinterpret_cast<const Pair<T>*>(p);
              xv[w][j][i][0] = t.a;
              xv[w][j][i][1] = t.b;
            } else {
              xv[w][j][i][0] = p[0];
              xv[w][j][i][1] = p[1];
            }
          }
        }
      }
    }
    if (k0 == 0) {
#pragma unroll
      for (int j = 0; j < R; ++j) pre(j, rb + t2 + j * 2 * BLK, true, ctr);
      // keep the scheduler from sinking loads below the first use
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ADJ != 0 && P >= 0) {
      // borrowed pairs; their neighbours are loaded pairs and stay as they are
#pragma unroll
      for (int w = 0; w < NWIN; ++w) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
          T edge[KB];  // what the one- or two-lane load of diagonal i brought
#pragma unroll
          for (int i = 0; i < KB; ++i) {
            edge[i] = xv[w][j][i][0];
            if (Run::src(P, i) == kDiaFromLo) {
              const bool shared = i >= 2 && Run::two(P, i - 2);
              const T e = shared ? edge[i >= 2 ? i - 2 : 0] : edge[i];
              const T up = lane_above(xv[w][j][i > 0 ? i - 1 : 0][0]);
              xv[w][j][i][0] = xv[w][j][i > 0 ? i - 1 : 0][1];
              xv[w][j][i][1] = lane == 63 ? e : up;
            } else if (Run::src(P, i) == kDiaFromHi) {
              const T dn = lane_below(xv[w][j][i + 1 < KB ? i + 1 : i][1]);
              xv[w][j][i][1] = xv[w][j][i + 1 < KB ? i + 1 : i][0];
              xv[w][j][i][0] = lane == 0 ? edge[i] : dn;
            }
          }
        }
      }
    }
    if (WC > 0 && ctr) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        cx[j] = Pair<T>{xv[0][j][(KB - 1) / 2][0], xv[0][j][(KB - 1) / 2][1]};
      }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const uint32_t m0 = (uint32_t)(M)mw[j];
      const uint32_t m1 = (uint32_t)(mw[j] >> (8 * sizeof(M)));
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        if (k0 + i < W) {
          T v0[NWIN], v1[NWIN];
#pragma unroll
          for (int w = 0; w < NWIN; ++w) {
            v0[w] = xv[w][j][i][0];
            v1[w] = xv[w][j][i][1];
          }
          const uint32_t bit = 1u << (k0 + i);
          a[j][0] = fmadd((m0 & bit) ? c[i] : T(0), comb(v0), a[j][0]);
          a[j][1] = fmadd((m1 & bit) ? c[i] : T(0), comb(v1), a[j][1]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < R; ++j) {
    post(j, rb + t2 + j * 2 * BLK, a[j][0], a[j][1], true, ctr, cx[j]);
  }
}

// offs must be ascending (build_dia: torch.unique).  win0 and (NWIN == 2)
// win1 share one geometry; comb(v) folds the NWIN loaded values of a column
// into its x.  pre(j, r0, full, ctr) issues the caller's operand loads of
// pair j and post(j, r0, a0, a1, full, ctr, cx) consumes its sums; full =
// rows r0, r0+1 are both below min(m, rhi).  Edge blocks skip pairs with
// r0 >= rhi.
// rowvec (or null) is an operand the caller reads at rows r0, r0+1.  Where
// it is the own x slab at the rows' own columns (CG's p in p . A p, the
// Jacobi iterate) and the middle diagonal of a compile-time W has offset 0,
// an interior block sets ctr: pre must then not load that operand, and post
// finds its pair in cx, the offset-0 pair the core holds anyway.
template <int WC, int R, bool SINGLE, int NWIN, uint32_t ADJ, typename T,
          typename M, typename Comb, typename Pre, typename Post>
__device__ __forceinline__ void dia_const_rows(
    const DiaConstPlanes<T, M>& planes, const int64_t* __restrict__ offs,
    int Wrt, const XWindow<T>& win0, const XWindow<T>& win1, Comb comb,
    const T* rowvec, int64_t m, int64_t row0, int64_t col_lo, int64_t rbase,
    int64_t rhi, Pre pre, Post post) {
  constexpr int KB = WC ? WC : 8;  // diagonals per load batch
  constexpr int64_t S = 2 * (int64_t)BLK * R;
  static_assert(ADJ == 0 || (WC > 0 && (ADJ >> (KB - 1)) == 0),
                "a plan needs a compile-time W");
  using Run = DiaRun<ADJ>;
  const int W = WC ? WC : Wrt;
  const int64_t lim = min(m, rhi);
  const int64_t rb = rbase + (int64_t)blockIdx.x * S;
  // own-piece index of row rb's main-diagonal column
  const int64_t cb = row0 + rb - col_lo - win0.nlo;
  const int64_t own_end = min(win0.nown, win0.wsize - win0.nlo);
  // the first batch's offsets and constants, in registers before any load
  int64_t o[KB];
  T c[KB];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    if (i < W) {
      o[i] = offs[i];
      c[i] = planes.cvals[i];
    }
  }
  bool interior = rb + S <= lim && cb + o[0] >= 0 &&
                  cb + (S - 1) + (WC ? o[KB - 1] : offs[W - 1]) < own_end;
#pragma unroll
  for (int q = 1; q < Run::len; ++q) {
    interior = interior && o[Run::start + q] == o[Run::start] + q;
  }
  if (interior) {
    const T* own[NWIN];
    own[0] = win0.own;
    own[NWIN - 1] = (NWIN == 2 ? win1 : win0).own;
    const bool ctr = WC > 0 && NWIN == 1 && rowvec != nullptr &&
                     rowvec + rb == win0.own + cb && o[(KB - 1) / 2] == 0;
    auto body = [&](auto par) {
      dia_const_interior<WC, R, NWIN, ADJ, decltype(par)::value>(
          planes, offs, W, own, comb, ctr, rb, cb, o, c, pre, post);
    };
    if (ADJ == 0) {
      body(std::integral_constant<int, -1>{});
    } else {
      const T* u0 = own[0] + (cb + o[Run::start]);
      const T* u1 = own[NWIN - 1] + (cb + o[Run::start]);
      const bool un0 = reinterpret_cast<uintptr_t>(u0) % sizeof(Pair<T>) != 0;
      const bool un1 = reinterpret_cast<uintptr_t>(u1) % sizeof(Pair<T>) != 0;
      if (un0 != un1) {
        body(std::integral_constant<int, -1>{});
      } else if (un0) {
        body(std::integral_constant<int, 1>{});
      } else {
        body(std::integral_constant<int, 0>{});
      }
    }
  } else {
    const int64_t t2 = 2 * (int64_t)threadIdx.x;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int64_t r0 = rb + t2 + j * 2 * BLK;
      if (r0 < rhi) {
        T a0 = ZeroOf<T>::value(), a1 = ZeroOf<T>::value();
        pre(j, r0, r0 + 1 < lim, false);
        dia_accumulate(
            planes, offs, W, r0, row0 + r0 - col_lo,
            [&](int64_t c0, T& x0, T& x1) {
              T v0[NWIN], v1[NWIN];
#pragma unroll
              for (int w = 0; w < NWIN; ++w) {
                (w == 0 ? win0 : win1)
                    .template pair<SINGLE, true>(c0, v0[w], v1[w]);
              }
              x0 = comb(v0);
              x1 = comb(v1);
            },
            a0, a1);
        post(j, r0, a0, a1, r0 + 1 < lim, false, Pair<T>{T(0), T(0)});
      }
    }
  }
}

template <typename T, typename M, int WC, uint32_t ADJ, bool FUSE_DOT,
          bool SINGLE, bool RESID>
__global__ __launch_bounds__(BLK) void dia_const_spmv_kernel(
    const DiaConstPlanes<T, M> planes, const int64_t* __restrict__ offs,
    const XWindow<T> win, T* __restrict__ y, const T* __restrict__ pvec,
    T* __restrict__ dot_partial, int64_t m, int W, int64_t col_lo,
    int64_t row0, int64_t rbase, int64_t rhi) {
  constexpr int R = dia_spmv_pairs(WC, RESID);
  const int64_t lim = min(m, rhi);
  Pair<T> pv[R];  // p (FUSE_DOT) or b (RESID) of the pair's rows
  T d[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    pv[j] = Pair<T>{T(0), T(0)};
    d[j] = T(0);
  }
  dia_const_rows<WC, R, SINGLE, 1, ADJ>(
      planes, offs, W, win, win, [](const T(&v)[1]) { return v[0]; },
      (FUSE_DOT || RESID) ? pvec : nullptr, m, row0, col_lo, rbase, rhi,
      [&](int j, int64_t r0, bool full, bool ctr) {
        if ((FUSE_DOT || RESID) && !ctr) {
          if (full) {
            pv[j] = *reinterpret_cast<const Pair<T>*>(&pvec[r0]);
          } else if (r0 < lim) {
            pv[j].a = pvec[r0];
          }
        }
      },
      [&](int j, int64_t r0, T a0, T a1, bool full, bool ctr, Pair<T> cx) {
        if (ctr) pv[j] = cx;
        if (RESID) {
          // y = b - A x: the V-cycle residual fused into the SpMV
          a0 = pv[j].a - a0;
          a1 = pv[j].b - a1;
        }
        if (full) {
          *reinterpret_cast<Pair<T>*>(&y[r0]) = Pair<T>{a0, a1};
        } else {
          store_pair_or_tail(y, r0, m, rhi, a0, a1);
        }
        if (FUSE_DOT) {
          T dd = T(0);
          if (full || r0 < lim) dd = fmadd(a0, pv[j].a, dd);
          if (full) dd = fmadd(a1, pv[j].b, dd);
          d[j] = dd;
        }
      });
  if (FUSE_DOT) {
    const T sum = block_sums_256<R>(d);
    const int64_t slot = (int64_t)blockIdx.x * R + threadIdx.x;
    if (threadIdx.x < R && slot * (2 * BLK) < rhi - rbase) {
      dot_partial[slot] = sum;
    }
  }
}

template <typename T, typename M, int WC, uint32_t ADJ, bool SINGLE>
__global__ __launch_bounds__(BLK) void dia_const_jacobi_kernel(
    const DiaConstPlanes<T, M> planes, const int64_t* __restrict__ offs,
    const XWindow<T> win, const T* __restrict__ xloc,
    const T* __restrict__ b, const T* __restrict__ dinv,
    T* __restrict__ xout, int64_t m, int W, int64_t col_lo, int64_t row0,
    T omega, int64_t rbase, int64_t rhi) {
  constexpr int R = kDiaSmoothPairs;
  Pair<T> xv[R], bv[R], dv[R];
  dia_const_rows<WC, R, SINGLE, 1, ADJ>(
      planes, offs, W, win, win, [](const T(&v)[1]) { return v[0]; }, xloc,
      m, row0, col_lo, rbase, rhi,
      [&](int j, int64_t r0, bool full, bool ctr) {
        if (full) {
          if (!ctr) xv[j] = *reinterpret_cast<const Pair<T>*>(&xloc[r0]);
          bv[j] = *reinterpret_cast<const Pair<T>*>(&b[r0]);
          dv[j] = *reinterpret_cast<const Pair<T>*>(&dinv[r0]);
        }
      },
      [&](int j, int64_t r0, T a0, T a1, bool full, bool ctr, Pair<T> cx) {
        if (ctr) xv[j] = cx;
        if (full) {
          *reinterpret_cast<Pair<T>*>(&xout[r0]) =
              Pair<T>{fmadd(omega * dv[j].a, bv[j].a - a0, xv[j].a),
                      fmadd(omega * dv[j].b, bv[j].b - a1, xv[j].b)};
        } else {
          jacobi_update(xloc, b, dinv, xout, omega, r0, m, rhi, a0, a1);
        }
      });
}

// dia_spmv_bpdot_kernel on the constant-plane source
template <typename T, typename M, int WC, uint32_t ADJ, bool SINGLE>
__global__ __launch_bounds__(BLK) void dia_const_bpdot_kernel(
    const DiaConstPlanes<T, M> planes, const int64_t* __restrict__ offs,
    const XWindow<T> rwin, const XWindow<T> pwin, T* __restrict__ pnew,
    T* __restrict__ q, const T* __restrict__ beta_num,
    const T* __restrict__ beta_den, T* __restrict__ dot_partial, int64_t m,
    int64_t mp, int W, int64_t col_lo, int64_t row0) {
  constexpr int R = kDiaBpdotPairs;
  const T beta = (*beta_num) / (*beta_den);
  auto comb = [&](const T(&v)[2]) { return fmadd(beta, v[1], v[0]); };
  T rr[R][2], pp[R][2];  // own rows of r and p_old
  T d[R];
#pragma unroll
  for (int j = 0; j < R; ++j) d[j] = T(0);
  dia_const_rows<WC, R, SINGLE, 2, ADJ>(
      planes, offs, W, rwin, pwin, comb, (const T*)nullptr, m, row0, col_lo,
      0, mp,
      [&](int j, int64_t r0, bool, bool) {
        // clamped like the streamed kernel's: offset 0 need not be a
        // diagonal, and row r0 + 1 of a lone tail is loaded but never used
        const int64_t c0 = row0 + r0 - col_lo;
        rwin.template pair<SINGLE, true>(c0, rr[j][0], rr[j][1]);
        pwin.template pair<SINGLE, true>(c0, pp[j][0], pp[j][1]);
      },
      [&](int j, int64_t r0, T a0, T a1, bool full, bool, Pair<T>) {
        // own-row p_new: the formula of the window recompute, same bits
        const T v0[2] = {rr[j][0], pp[j][0]}, v1[2] = {rr[j][1], pp[j][1]};
        const T p0 = comb(v0), p1 = comb(v1);
        if (full) {
          *reinterpret_cast<Pair<T>*>(&pnew[r0]) = Pair<T>{p0, p1};
          *reinterpret_cast<Pair<T>*>(&q[r0]) = Pair<T>{a0, a1};
        } else {
          store_pair_or_tail(pnew, r0, m, m, p0, p1);
          store_pair_or_tail(q, r0, m, m, a0, a1);
        }
        T dd = T(0);
        if (full || r0 < m) dd = fmadd(a0, p0, dd);
        if (full) dd = fmadd(a1, p1, dd);
        d[j] = dd;
      });
  const T sum = block_sums_256<R>(d);
  const int64_t slot = (int64_t)blockIdx.x * R + threadIdx.x;
  if (threadIdx.x < R && slot * (2 * BLK) < mp) dot_partial[slot] = sum;
}

// blocks of BLK threads covering `span` rows, two rows per thread
inline int64_t pair_blocks(int64_t span) {
  return (span + 2 * BLK - 1) / (2 * BLK);
}

template <typename F>
void dispatch_bool(bool v, F&& f) {
  if (v) f(std::true_type{}); else f(std::false_type{});
}

// Launch geometry shared by every row-pair launcher: padded row count, the
// resolved row range (rhi < 0 = all rows), window piece sizes and the grid.
struct RowPairLaunch {
  int64_t mp, rbase, rhi, nlo, nown, wsize, nblocks;
  bool single;  // no halo pieces: the own slab is the whole window

  RowPairLaunch(int64_t mp_, const at::Tensor& hlo, const at::Tensor& own,
                const at::Tensor& hhi, int64_t wsize_, int64_t rbase_ = 0,
                int64_t rhi_ = -1)
      : mp(mp_), rbase(rbase_), rhi(rhi_ < 0 ? mp : rhi_),
        nlo(hlo.numel()), nown(own.numel()), wsize(wsize_),
        nblocks(rhi > rbase ? pair_blocks(rhi - rbase) : 0),
        single(nlo == 0 && hhi.numel() == 0) {}

  bool empty() const { return nblocks == 0; }

  // window view of one vector's pieces; an empty halo piece is never read,
  // its pointer only has to be valid
  template <typename T>
  XWindow<T> window(const at::Tensor& hlo, const at::Tensor& own,
                    const at::Tensor& hhi) const {
    const T* o = own.data_ptr<T>();
    return {hlo.numel() ? hlo.data_ptr<T>() : o, o,
            hhi.numel() ? hhi.data_ptr<T>() : o, nlo, nown, wsize};
  }

  template <typename... P, typename... A>
  void launch(void (*kern)(P...), A... args) const {
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(BLK), 0, cur_stream(),
                       static_cast<P>(args)...);
  }

  // kernels whose threads own R row pairs: nblocks stays the number of
  // 2 * BLK row groups (and of dot partials), the grid shrinks by R
  template <int R, typename... P, typename... A>
  void launch_pairs(void (*kern)(P...), A... args) const {
    hipLaunchKernelGGL(kern, dim3((nblocks + R - 1) / R), dim3(BLK), 0,
                       cur_stream(), static_cast<P>(args)...);
  }
};

// A DIA op's value source is (planes, mask): without a mask `planes` holds
// the (W, mp) streamed planes; with one it holds the W plane constants and
// `mask` the mp row words (DiaConstPlanes; real types, W <= 32).
using OptTensor = c10::optional<at::Tensor>;

inline int64_t dia_mp(const at::Tensor& planes, const OptTensor& mask,
                      int64_t W) {
  return mask ? mask->numel() : planes.numel() / W;
}

// f(provider) for the value source of a DIA op
template <typename T, typename F>
void dispatch_dia_planes(const at::Tensor& planes, const OptTensor& mask,
                         int64_t W, F&& f) {
  if (!mask) {
    f(DiaPlanes<T>{planes.data_ptr<T>(), planes.numel() / W});
    return;
  }
  if constexpr (std::is_floating_point_v<T>) {
    TORCH_CHECK(planes.numel() == W && W <= 8 * (int64_t)mask->element_size() &&
                    mask->numel() % 2 == 0,
                "dia: W constants and an even number of mask words of at "
                "least W bits expected");
    const T* c = planes.data_ptr<T>();
    const void* mw = mask->data_ptr();
    switch (mask->scalar_type()) {
      case at::kByte:
        f(DiaConstPlanes<T, uint8_t>{c, static_cast<const uint8_t*>(mw)});
        return;
      case at::kUInt16:
        f(DiaConstPlanes<T, uint16_t>{c, static_cast<const uint16_t*>(mw)});
        return;
      case at::kUInt32:
        f(DiaConstPlanes<T, uint32_t>{c, static_cast<const uint32_t*>(mw)});
        return;
      default:
        break;
    }
  }
  TORCH_CHECK(false, "dia: constant planes need a real value type and a "
                     "uint8/uint16/uint32 row mask");
}

template <typename P>
struct DiaConstOf : std::false_type {};
template <typename T, typename M>
struct DiaConstOf<DiaConstPlanes<T, M>> : std::true_type {
  using mask_t = M;
};

// The lane-exchange plans a compile-time W = N is built for, chosen from the
// mirror's adjacency word (bit i: offs[i + 1] == offs[i] + 1): the whole
// band (tridiagonal, pentadiagonal, ...), else the three middle diagonals
// of an odd W >= 5 (the -1, 0, +1 of a 5-pt or 7-pt stencil), else none.
// Any other adjacency loads every pair, which is always correct.
template <int N, typename F>
void dispatch_dia_adj(int64_t adj, F&& f) {
  constexpr uint32_t band = (1u << (N - 1)) - 1;
  constexpr uint32_t mid = (N % 2 == 1 && N >= 5) ? 3u << (N / 2 - 1) : 0;
  const std::integral_constant<int, N> wc;
  if constexpr (band != 0) {
    if ((adj & band) == band) {
      f(wc, std::integral_constant<uint32_t, band>{});
      return;
    }
  }
  if constexpr (mid != 0) {
    if ((adj & mid) == mid) {
      f(wc, std::integral_constant<uint32_t, mid>{});
      return;
    }
  }
  f(wc, std::integral_constant<uint32_t, 0>{});
}

// f(integral_constant WC, integral_constant ADJ) for the constant-plane
// kernels: W itself under a u8 mask (1 <= W <= 8) with its lane-exchange
// plan, 0 (run-time W, no plan) under the wider masks
template <typename M, typename F>
void dispatch_dia_wc(int64_t W, int64_t adj, F&& f) {
  TORCH_CHECK(W >= 1, "dia: at least one diagonal expected");
  if constexpr (std::is_same_v<M, uint8_t>) {
    switch (W) {
#define SPARSE_DIA_WC(N) \
  case N: dispatch_dia_adj<N>(adj, f); return;
      SPARSE_DIA_WC(1) SPARSE_DIA_WC(2) SPARSE_DIA_WC(3) SPARSE_DIA_WC(4)
      SPARSE_DIA_WC(5) SPARSE_DIA_WC(6) SPARSE_DIA_WC(7) SPARSE_DIA_WC(8)
#undef SPARSE_DIA_WC
      default: break;
    }
  }
  f(std::integral_constant<int, 0>{}, std::integral_constant<uint32_t, 0>{});
}

}  // namespace

void build_ell_hip(at::Tensor indptr, at::Tensor indices, at::Tensor values,
                   at::Tensor eidx, at::Tensor evals, int64_t W,
                   int64_t pad_idx) {
  const int64_t m = indptr.numel() - 1;
  const int64_t mp = evals.numel() / W;
  DISPATCH_VALUES(values.scalar_type(), "build_ell", [&] {
    using T = scalar_t;
    DISPATCH_INDEX(indices.scalar_type(), "build_ell_idx", [&] {
      hipLaunchKernelGGL((build_ell_kernel<T, index_t>), dim3((mp + 255) / 256),
                         dim3(256), 0, cur_stream(), indptr.data_ptr<int64_t>(),
                         indices.data_ptr<index_t>(), values.data_ptr<T>(),
                         eidx.data_ptr<index_t>(), evals.data_ptr<T>(), m, mp,
                         (int)W, (index_t)pad_idx);
    });
  });
}

void build_dia_hip(at::Tensor indptr, at::Tensor indices, at::Tensor values,
                   at::Tensor offs, at::Tensor dvals, int64_t W,
                   int64_t row0) {
  const int64_t m = indptr.numel() - 1;
  const int64_t mp = dvals.numel() / W;
  if (m == 0) return;
  DISPATCH_VALUES(values.scalar_type(), "build_dia", [&] {
    using T = scalar_t;
    DISPATCH_INDEX(indices.scalar_type(), "build_dia_idx", [&] {
      hipLaunchKernelGGL((build_dia_kernel<T, index_t>),
                         dim3((m + 255) / 256), dim3(256), 0, cur_stream(),
                         indptr.data_ptr<int64_t>(),
                         indices.data_ptr<index_t>(), values.data_ptr<T>(),
                         offs.data_ptr<int64_t>(), dvals.data_ptr<T>(), m, mp,
                         (int)W, row0);
    });
  });
}

// Classify the filled planes (fp32/fp64) for the constant-plane source:
// cvals (W, pre-zeroed) receives the plane constants, mask (mp words) the
// row masks, and ok[0] (preset to 1) is cleared unless every plane holds
// only +0.0 and its constant.  One extra read of the planes at mirror
// build; nothing here runs per SpMV.
void dia_classify_hip(at::Tensor dvals, at::Tensor cvals, at::Tensor mask,
                      at::Tensor ok, int64_t W) {
  const int64_t mp = mask.numel();
  TORCH_CHECK(dvals.numel() == W * mp && cvals.numel() == W &&
                  cvals.scalar_type() == dvals.scalar_type() &&
                  ok.scalar_type() == at::kInt &&
                  W <= 8 * (int64_t)mask.element_size(),
              "dia_classify: inconsistent arguments");
  if (mp == 0) return;
  const dim3 g1((unsigned)std::min<int64_t>((mp + 255) / 256, 1024),
                (unsigned)W);
  auto run = [&](auto bits, auto word) {
    using B = decltype(bits);
    using M = decltype(word);
    const B* d = static_cast<const B*>(dvals.data_ptr());
    B* c = static_cast<B*>(cvals.data_ptr());
    hipLaunchKernelGGL((dia_plane_const_kernel<B>), g1, dim3(256), 0,
                       cur_stream(), d, c, mp);
    hipLaunchKernelGGL((dia_row_mask_kernel<B, M>), dim3((mp + 255) / 256),
                       dim3(256), 0, cur_stream(), d, c,
                       static_cast<M*>(mask.data_ptr()),
                       ok.data_ptr<int32_t>(), mp, (int)W);
  };
  auto by_word = [&](auto bits) {
    switch (mask.scalar_type()) {
      case at::kByte: run(bits, uint8_t{}); break;
      case at::kUInt16: run(bits, uint16_t{}); break;
      case at::kUInt32: run(bits, uint32_t{}); break;
      default: TORCH_CHECK(false, "dia_classify: mask must be uint8/16/32");
    }
  };
  switch (dvals.scalar_type()) {
    case at::kFloat: by_word(uint32_t{}); break;
    case at::kDouble: by_word(uint64_t{}); break;
    default: TORCH_CHECK(false, "dia_classify: fp32/fp64 planes only");
  }
}

// The fused-dot ops own their per-block partials: one slot per launched
// block, every block writes its slot, and the 0-dim sum is returned (an
// empty row range is an exact zero).
static at::Tensor sum_or_zero(const at::Tensor& partial,
                              const at::Tensor& like) {
  return partial.defined() ? partial.sum() : at::zeros({}, like.options());
}

// y = A x on rows [rbase, rhi); with pvec also the partials of pvec . y
static at::Tensor ell_spmv_impl(const at::Tensor& eidx, const at::Tensor& evals,
                                const at::Tensor& hlo, const at::Tensor& own,
                                const at::Tensor& hhi, at::Tensor& y,
                                const at::Tensor* pvec, int64_t W, int64_t m,
                                int64_t col_lo, int64_t rbase, int64_t rhi) {
  const RowPairLaunch L(evals.numel() / W, hlo, own, hhi, 0, rbase, rhi);
  at::Tensor partial;
  if (L.empty()) return partial;
  if (pvec) partial = at::empty({L.nblocks}, evals.options());
  DISPATCH_VALUES(evals.scalar_type(), "ell_spmv", [&] {
    using T = scalar_t;
    DISPATCH_INDEX(eidx.scalar_type(), "ell_spmv_idx", [&] {
      dispatch_bool(pvec != nullptr, [&](auto fuse) {
        dispatch_bool(L.single, [&](auto single) {
          L.launch(ell_spmv_kernel<T, index_t, decltype(fuse)::value,
                                   decltype(single)::value>,
                   eidx.data_ptr<index_t>(), evals.data_ptr<T>(),
                   L.window<T>(hlo, own, hhi), y.data_ptr<T>(),
                   pvec ? pvec->data_ptr<T>() : nullptr,
                   pvec ? partial.data_ptr<T>() : nullptr, m, L.mp, W, col_lo,
                   L.rbase, L.rhi);
        });
      });
    });
  });
  return partial;
}

void ell_spmv_plain_hip(at::Tensor eidx, at::Tensor evals, at::Tensor hlo,
                        at::Tensor own, at::Tensor hhi, at::Tensor y,
                        int64_t W, int64_t m, int64_t col_lo,
                        int64_t rbase, int64_t rhi) {
  ell_spmv_impl(eidx, evals, hlo, own, hhi, y, nullptr, W, m, col_lo, rbase,
                rhi);
}

at::Tensor ell_spmv_dot_hip(at::Tensor eidx, at::Tensor evals, at::Tensor hlo,
                            at::Tensor own, at::Tensor hhi, at::Tensor y,
                            at::Tensor pvec, int64_t W, int64_t m,
                            int64_t col_lo, int64_t rbase, int64_t rhi) {
  return sum_or_zero(ell_spmv_impl(eidx, evals, hlo, own, hhi, y, &pvec, W, m,
                                   col_lo, rbase, rhi),
                     evals);
}

void ell_jacobi_hip(at::Tensor eidx, at::Tensor evals, at::Tensor hlo,
                    at::Tensor own, at::Tensor hhi, at::Tensor xloc,
                    at::Tensor b, at::Tensor dinv, at::Tensor xout,
                    int64_t W, int64_t m, int64_t col_lo, double omega) {
  const RowPairLaunch L(evals.numel() / W, hlo, own, hhi, 0);
  if (L.empty()) return;
  DISPATCH_VALUES(evals.scalar_type(), "ell_jacobi", [&] {
    using T = scalar_t;
    DISPATCH_INDEX(eidx.scalar_type(), "ell_jacobi_idx", [&] {
      dispatch_bool(L.single, [&](auto single) {
        L.launch(ell_jacobi_kernel<T, index_t, decltype(single)::value>,
                 eidx.data_ptr<index_t>(), evals.data_ptr<T>(),
                 L.window<T>(hlo, own, hhi), xloc.data_ptr<T>(),
                 b.data_ptr<T>(), dinv.data_ptr<T>(), xout.data_ptr<T>(), m,
                 L.mp, W, col_lo, omega);
      });
    });
  });
}

// y = A x on rows [rbase, rhi); with pvec also the partials of pvec . y;
// RESID: y = b - A x, the fused V-cycle residual (the pvec slot carries b)
template <bool RESID>
static at::Tensor dia_spmv_impl(const at::Tensor& planes, const OptTensor& mask,
                                const at::Tensor& offs, const at::Tensor& hlo,
                                const at::Tensor& own, const at::Tensor& hhi,
                                at::Tensor& y, const at::Tensor* pvec,
                                int64_t W, int64_t m, int64_t col_lo,
                                int64_t row0, int64_t wsize, int64_t rbase,
                                int64_t rhi, int64_t adj) {
  const RowPairLaunch L(dia_mp(planes, mask, W), hlo, own, hhi, wsize, rbase,
                        rhi);
  const bool fuse_dot = pvec && !RESID;
  at::Tensor partial;
  if (L.empty()) return partial;
  if (fuse_dot) partial = at::empty({L.nblocks}, planes.options());
  DISPATCH_VALUES(planes.scalar_type(), "dia_spmv", [&] {
    using T = scalar_t;
    dispatch_dia_planes<T>(planes, mask, W, [&](auto pl) {
      dispatch_bool(fuse_dot, [&](auto fuse) {
        dispatch_bool(L.single, [&](auto single) {
          using PL = decltype(pl);
          const T* pp = pvec ? pvec->data_ptr<T>() : nullptr;
          T* dp = fuse_dot ? partial.data_ptr<T>() : nullptr;
          if constexpr (RESID && decltype(fuse)::value) {
          } else if constexpr (DiaConstOf<PL>::value) {
            using M = typename DiaConstOf<PL>::mask_t;
            dispatch_dia_wc<M>(W, adj, [&](auto wc, auto plan) {
              L.launch_pairs<dia_spmv_pairs(decltype(wc)::value, RESID)>(
                  dia_const_spmv_kernel<T, M, decltype(wc)::value,
                                        decltype(plan)::value,
                                        decltype(fuse)::value,
                                        decltype(single)::value, RESID>,
                  pl, offs.data_ptr<int64_t>(), L.window<T>(hlo, own, hhi),
                  y.data_ptr<T>(), pp, dp, m, W, col_lo, row0, L.rbase,
                  L.rhi);
            });
          } else {
            L.launch(dia_spmv_kernel<T, PL, decltype(fuse)::value,
                                     decltype(single)::value, RESID>,
                     pl, offs.data_ptr<int64_t>(), L.window<T>(hlo, own, hhi),
                     y.data_ptr<T>(), pp, dp, m, L.mp, W, col_lo, row0,
                     L.rbase, L.rhi);
          }
        });
      });
    });
  });
  return partial;
}

void dia_spmv_plain_hip(at::Tensor planes, OptTensor mask, at::Tensor offs,
                        at::Tensor hlo, at::Tensor own, at::Tensor hhi,
                        at::Tensor y, int64_t W, int64_t m, int64_t col_lo,
                        int64_t row0, int64_t wsize, int64_t rbase,
                        int64_t rhi, int64_t adj) {
  dia_spmv_impl<false>(planes, mask, offs, hlo, own, hhi, y, nullptr, W, m,
                       col_lo, row0, wsize, rbase, rhi, adj);
}

at::Tensor dia_spmv_dot_hip(at::Tensor planes, OptTensor mask, at::Tensor offs,
                            at::Tensor hlo, at::Tensor own, at::Tensor hhi,
                            at::Tensor y, at::Tensor pvec, int64_t W,
                            int64_t m, int64_t col_lo, int64_t row0,
                            int64_t wsize, int64_t rbase, int64_t rhi,
                            int64_t adj) {
  return sum_or_zero(dia_spmv_impl<false>(planes, mask, offs, hlo, own, hhi, y,
                                          &pvec, W, m, col_lo, row0, wsize,
                                          rbase, rhi, adj),
                     planes);
}

void dia_residual_hip(at::Tensor planes, OptTensor mask, at::Tensor offs,
                      at::Tensor hlo, at::Tensor own, at::Tensor hhi,
                      at::Tensor b, at::Tensor y, int64_t W, int64_t m,
                      int64_t col_lo, int64_t row0, int64_t wsize,
                      int64_t rbase, int64_t rhi, int64_t adj) {
  dia_spmv_impl<true>(planes, mask, offs, hlo, own, hhi, y, &b, W, m, col_lo,
                      row0, wsize, rbase, rhi, adj);
}

void dia_jacobi_hip(at::Tensor planes, OptTensor mask, at::Tensor offs,
                    at::Tensor hlo, at::Tensor own, at::Tensor hhi,
                    at::Tensor xloc, at::Tensor b, at::Tensor dinv,
                    at::Tensor xout, int64_t W, int64_t m, int64_t col_lo,
                    int64_t row0, int64_t wsize, double omega, int64_t rbase,
                    int64_t rhi, int64_t adj) {
  const RowPairLaunch L(dia_mp(planes, mask, W), hlo, own, hhi, wsize, rbase,
                        rhi);
  if (L.empty()) return;
  DISPATCH_VALUES(planes.scalar_type(), "dia_jacobi", [&] {
    using T = scalar_t;
    dispatch_dia_planes<T>(planes, mask, W, [&](auto pl) {
      dispatch_bool(L.single, [&](auto single) {
        using PL = decltype(pl);
        if constexpr (DiaConstOf<PL>::value) {
          using M = typename DiaConstOf<PL>::mask_t;
          dispatch_dia_wc<M>(W, adj, [&](auto wc, auto plan) {
            L.launch_pairs<kDiaSmoothPairs>(
                dia_const_jacobi_kernel<T, M, decltype(wc)::value,
                                        decltype(plan)::value,
                                        decltype(single)::value>,
                pl, offs.data_ptr<int64_t>(), L.window<T>(hlo, own, hhi),
                xloc.data_ptr<T>(), b.data_ptr<T>(), dinv.data_ptr<T>(),
                xout.data_ptr<T>(), m, W, col_lo, row0, omega, L.rbase,
                L.rhi);
          });
        } else {
          L.launch(dia_jacobi_kernel<T, PL, decltype(single)::value>, pl,
                   offs.data_ptr<int64_t>(), L.window<T>(hlo, own, hhi),
                   xloc.data_ptr<T>(), b.data_ptr<T>(), dinv.data_ptr<T>(),
                   xout.data_ptr<T>(), m, L.mp, W, col_lo, row0, omega,
                   L.rbase, L.rhi);
        }
      });
    });
  });
}

at::Tensor dia_spmv_bpdot_hip(at::Tensor planes, OptTensor mask,
                              at::Tensor offs, at::Tensor r_hlo,
                              at::Tensor r_own, at::Tensor r_hhi,
                              at::Tensor p_hlo, at::Tensor p_own,
                              at::Tensor p_hhi, at::Tensor pnew, at::Tensor q,
                              at::Tensor beta_num, at::Tensor beta_den,
                              int64_t W, int64_t m, int64_t col_lo,
                              int64_t row0, int64_t wsize, int64_t adj) {
  TORCH_CHECK(pnew.data_ptr() != p_own.data_ptr(),
              "dia_spmv_bpdot: pnew must not alias p_own (double-buffer)");
  const RowPairLaunch L(dia_mp(planes, mask, W), r_hlo, r_own, r_hhi, wsize);
  at::Tensor partial;
  if (L.empty()) return sum_or_zero(partial, planes);
  partial = at::empty({L.nblocks}, planes.options());
  DISPATCH_VALUES(planes.scalar_type(), "dia_spmv_bpdot", [&] {
    using T = scalar_t;
    dispatch_dia_planes<T>(planes, mask, W, [&](auto pl) {
      dispatch_bool(L.single, [&](auto single) {
        using PL = decltype(pl);
        auto go = [&](auto launch, auto kern) {
          launch(kern, pl, offs.data_ptr<int64_t>(),
                 L.window<T>(r_hlo, r_own, r_hhi),
                 L.window<T>(p_hlo, p_own, p_hhi), pnew.data_ptr<T>(),
                 q.data_ptr<T>(), beta_num.data_ptr<T>(),
                 beta_den.data_ptr<T>(), partial.data_ptr<T>(), m, L.mp, W,
                 col_lo, row0);
        };
        if constexpr (DiaConstOf<PL>::value) {
          using M = typename DiaConstOf<PL>::mask_t;
          dispatch_dia_wc<M>(W, adj, [&](auto wc, auto plan) {
            go([&](auto... a) { L.launch_pairs<kDiaBpdotPairs>(a...); },
               dia_const_bpdot_kernel<T, M, decltype(wc)::value,
                                      decltype(plan)::value,
                                      decltype(single)::value>);
          });
        } else {
          go([&](auto... a) { L.launch(a...); },
             dia_spmv_bpdot_kernel<T, PL, decltype(single)::value>);
        }
      });
    });
  });
  return partial.sum();
}
