// torch.ops bindings for the sparse HIP (gfx950) kernels.
//
// Loaded via torch.ops.load_library from sparse/kernels/_build/sparse_hip.so;
// Python wrappers live in sparse/kernels/__init__.py.
#include <algorithm>
#include <cstdint>
#include <vector>

#include <torch/library.h>

#include <ATen/ATen.h>

// launchers defined in the .hip translation units
void spmv_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
              int64_t, double);
void spmv_dot_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                  at::Tensor, at::Tensor, int64_t);
void axpby_norm2_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, bool,
                     bool, at::Tensor);
void build_ell_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                   int64_t, int64_t);
void build_dia_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                   int64_t, int64_t);
void ell_spmv_plain_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                        at::Tensor, at::Tensor, int64_t, int64_t, int64_t,
                        int64_t, int64_t);
at::Tensor ell_spmv_dot_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                            at::Tensor, at::Tensor, at::Tensor, int64_t,
                            int64_t, int64_t, int64_t, int64_t);
void ell_jacobi_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                    at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                    at::Tensor, int64_t, int64_t, int64_t, double);
void cg_xr_norm2_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                     at::Tensor, at::Tensor, at::Tensor, int64_t);
// DIA ops: (planes, mask) is the value source — the streamed planes and no
// mask, or the W plane constants and the row mask words
using OptTensor = c10::optional<at::Tensor>;
void dia_classify_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, int64_t);
at::Tensor dia_spmv_bpdot_hip(at::Tensor, OptTensor, at::Tensor, at::Tensor,
                              at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                              at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                              at::Tensor, int64_t, int64_t, int64_t, int64_t,
                              int64_t, int64_t);
void dia_spmv_plain_hip(at::Tensor, OptTensor, at::Tensor, at::Tensor,
                        at::Tensor, at::Tensor, at::Tensor, int64_t, int64_t,
                        int64_t, int64_t, int64_t, int64_t, int64_t, int64_t);
at::Tensor dia_spmv_dot_hip(at::Tensor, OptTensor, at::Tensor, at::Tensor,
                            at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                            int64_t, int64_t, int64_t, int64_t, int64_t,
                            int64_t, int64_t, int64_t);
void dia_residual_hip(at::Tensor, OptTensor, at::Tensor, at::Tensor,
                      at::Tensor, at::Tensor, at::Tensor, at::Tensor, int64_t,
                      int64_t, int64_t, int64_t, int64_t, int64_t, int64_t,
                      int64_t);
void dia_jacobi_hip(at::Tensor, OptTensor, at::Tensor, at::Tensor, at::Tensor,
                    at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                    at::Tensor, int64_t, int64_t, int64_t, int64_t, int64_t,
                    double, int64_t, int64_t, int64_t);
void add_nnz_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor);
void add_compute_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                     at::Tensor, at::Tensor, at::Tensor, at::Tensor, double,
                     double);
void mult_nnz_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor);
void mult_compute_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                      at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                      at::Tensor);
void mult_dense_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor);
void axpby_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, bool, bool,
               int64_t);
void spmm_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
              int64_t);
void rspmm_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor);
void bsr_spmm_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                  int64_t);
void sddmm_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
               at::Tensor, int64_t);
void csr_to_dense_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor);
void coo_to_csr_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                    at::Tensor, at::Tensor, at::Tensor, at::Tensor);
void dense_to_csr_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, bool);
void csr_diagonal_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, int64_t);
void csc_spmv_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                  int64_t);
void csc_spmm_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                  int64_t);
void tropical_spmv_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, int64_t);
void rk_calc_dy_hip(at::Tensor, at::Tensor, double, at::Tensor);
void cdist_hip(at::Tensor, at::Tensor, at::Tensor);
void spgemm_nnz_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                    at::Tensor, int64_t, int64_t);
void spgemm_compute_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                        at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                        at::Tensor, at::Tensor, int64_t, int64_t);
void trsv_solve_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                    at::Tensor, at::Tensor, at::Tensor, at::Tensor);
void ilu0_factor_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                     at::Tensor, at::Tensor, at::Tensor, at::Tensor);
void fsai_factor_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                     at::Tensor, at::Tensor, at::Tensor, int64_t, int64_t,
                     at::Tensor, at::Tensor);
void color_round_hip(at::Tensor, at::Tensor, at::Tensor, int64_t, int64_t,
                     at::Tensor, at::Tensor, at::Tensor);
void mcgs_sweep_hip(at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                    at::Tensor, at::Tensor, at::Tensor, bool);

// Dependency levels of a strict-triangle CSR, one sequential O(nnz) pass on
// the host (setup path of sparse/trisolve.py): levels[i] = 0 for a row with
// no strict entries, else 1 + max(levels[j]) over its columns j.  Rows are
// walked top-down for a lower triangle and bottom-up for an upper one, so
// every levels[j] read is final.  A device relaxation or frontier peeling
// would cost nlevels passes, and nlevels can equal n.
template <typename I>
static void trsv_levels_impl(const int64_t* ip, const I* ix, int64_t n,
                             bool lower, int64_t* lv) {
  for (int64_t s = 0; s < n; ++s) {
    const int64_t i = lower ? s : n - 1 - s;
    int64_t l = 0;
    for (int64_t p = ip[i]; p < ip[i + 1]; ++p) {
      const int64_t j = static_cast<int64_t>(ix[p]);
      TORCH_CHECK(lower ? (0 <= j && j < i) : (i < j && j < n),
                  "trsv_levels: entry outside the strict triangle");
      l = std::max(l, lv[j] + 1);
    }
    lv[i] = l;
  }
}

at::Tensor trsv_levels_cpu(at::Tensor indptr, at::Tensor indices, bool lower) {
  TORCH_CHECK(indptr.scalar_type() == at::kLong && indptr.numel() >= 1 &&
                  indptr.is_contiguous() && indices.is_contiguous(),
              "trsv_levels: bad structure tensors");
  const int64_t n = indptr.numel() - 1;
  const int64_t* ip = indptr.data_ptr<int64_t>();
  TORCH_CHECK(ip[0] == 0 && ip[n] == indices.numel(),
              "trsv_levels: indptr does not match indices");
  for (int64_t i = 0; i < n; ++i)
    TORCH_CHECK(ip[i] <= ip[i + 1], "trsv_levels: indptr not monotone");
  at::Tensor levels = at::zeros({n}, indptr.options());
  if (indices.scalar_type() == at::kInt) {
    trsv_levels_impl(ip, indices.data_ptr<int32_t>(), n, lower,
                     levels.data_ptr<int64_t>());
  } else {
    TORCH_CHECK(indices.scalar_type() == at::kLong,
                "trsv_levels: indices must be int32 or int64");
    trsv_levels_impl(ip, indices.data_ptr<int64_t>(), n, lower,
                     levels.data_ptr<int64_t>());
  }
  return levels;
}

// Sequential greedy colouring in priority order on the host (the host twin
// of color.hip; backs sparse/gauss_seidel.py without a GPU).  The pattern is
// structurally symmetric (the caller symmetrises), diagonal entries are
// skipped.  Vertices are visited by decreasing (h(i), i), h the 32-bit hash
// of color.hip, and each takes the smallest colour no coloured neighbour has.
static inline uint32_t color_hash_host(uint32_t i, uint32_t seed) {
  uint32_t x = i ^ seed;
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

template <typename I>
static void color_greedy_impl(const int64_t* ip, const I* ix, int64_t n,
                              uint32_t seed, int32_t* color) {
  std::vector<int64_t> visit(n);
  std::vector<uint32_t> h(n);
  for (int64_t i = 0; i < n; ++i) {
    visit[i] = i;
    h[i] = color_hash_host(static_cast<uint32_t>(i), seed);
  }
  std::sort(visit.begin(), visit.end(), [&](int64_t a, int64_t b) {
    return h[a] != h[b] ? h[a] > h[b] : a > b;
  });
  // stamp[c] == s + 1: colour c is taken around the s-th visited vertex; a
  // vertex of degree d finds a free colour among 0..d
  std::vector<int64_t> stamp(n + 1, 0);
  for (int64_t s = 0; s < n; ++s) {
    const int64_t i = visit[s];
    for (int64_t p = ip[i]; p < ip[i + 1]; ++p) {
      const int64_t j = static_cast<int64_t>(ix[p]);
      TORCH_CHECK(0 <= j && j < n, "color_greedy: column outside the matrix");
      if (j != i && color[j] >= 0) stamp[color[j]] = s + 1;
    }
    int32_t c = 0;
    while (stamp[c] == s + 1) ++c;
    color[i] = c;
  }
}

at::Tensor color_greedy_cpu(at::Tensor indptr, at::Tensor indices,
                            int64_t seed) {
  TORCH_CHECK(indptr.scalar_type() == at::kLong && indptr.numel() >= 1 &&
                  indptr.is_contiguous() && indices.is_contiguous(),
              "color_greedy: bad structure tensors");
  const int64_t n = indptr.numel() - 1;
  const int64_t* ip = indptr.data_ptr<int64_t>();
  TORCH_CHECK(ip[0] == 0 && ip[n] == indices.numel(),
              "color_greedy: indptr does not match indices");
  for (int64_t i = 0; i < n; ++i)
    TORCH_CHECK(ip[i] <= ip[i + 1], "color_greedy: indptr not monotone");
  at::Tensor colors = at::full({n}, -1, indptr.options().dtype(at::kInt));
  if (indices.scalar_type() == at::kInt) {
    color_greedy_impl(ip, indices.data_ptr<int32_t>(), n,
                      static_cast<uint32_t>(seed), colors.data_ptr<int32_t>());
  } else {
    TORCH_CHECK(indices.scalar_type() == at::kLong,
                "color_greedy: indices must be int32 or int64");
    color_greedy_impl(ip, indices.data_ptr<int64_t>(), n,
                      static_cast<uint32_t>(seed), colors.data_ptr<int32_t>());
  }
  return colors;
}

// Sequential IKJ ILU(0) on the host, in place in v (the host twin of
// ilu0.hip; backs sparse/ilu.py without a GPU).  Rows are column-sorted and
// duplicate-free with a stored diagonal at dp[i]; the update of one k is a
// two-pointer merge of row i past k with row k past its diagonal.  Returns
// the first row whose pivot is exactly zero, or n.
template <typename T, typename I>
static int64_t ilu0_factor_impl(const int64_t* ip, const I* ix, T* v,
                                const int64_t* dp, int64_t n) {
  int64_t bad = n;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t pe = ip[i + 1];
    TORCH_CHECK(ip[i] <= dp[i] && dp[i] < pe &&
                    static_cast<int64_t>(ix[dp[i]]) == i,
                "ilu0_factor: diag_ptr does not point at the diagonal");
    for (int64_t q = ip[i]; q < dp[i]; ++q) {
      const int64_t k = static_cast<int64_t>(ix[q]);
      TORCH_CHECK(0 <= k && k < i, "ilu0_factor: rows must be column-sorted");
      const T m = v[q] / v[dp[k]];
      v[q] = m;
      int64_t p = q + 1;
      for (int64_t t = dp[k] + 1; t < ip[k + 1] && p < pe; ++t) {
        while (p < pe && ix[p] < ix[t]) ++p;
        if (p < pe && ix[p] == ix[t]) v[p] -= m * v[t];
      }
    }
    if (bad == n && v[dp[i]] == T(0)) bad = i;
  }
  return bad;
}

void ilu0_factor_cpu(at::Tensor indptr, at::Tensor indices, at::Tensor values,
                     at::Tensor diag_ptr, at::Tensor /*order*/,
                     at::Tensor /*level_ptr*/, at::Tensor /*sched*/,
                     at::Tensor flag) {
  TORCH_CHECK(indptr.scalar_type() == at::kLong && indptr.numel() >= 1 &&
                  indptr.is_contiguous() && indices.is_contiguous() &&
                  values.is_contiguous() && diag_ptr.is_contiguous() &&
                  diag_ptr.scalar_type() == at::kLong &&
                  flag.scalar_type() == at::kLong && flag.numel() == 1,
              "ilu0_factor: bad structure tensors");
  const int64_t n = indptr.numel() - 1;
  const int64_t* ip = indptr.data_ptr<int64_t>();
  TORCH_CHECK(ip[0] == 0 && ip[n] == indices.numel() &&
                  indices.numel() == values.numel() && diag_ptr.numel() == n,
              "ilu0_factor: indptr does not match indices");
  for (int64_t i = 0; i < n; ++i)
    TORCH_CHECK(ip[i] <= ip[i + 1], "ilu0_factor: indptr not monotone");
  const bool i32 = indices.scalar_type() == at::kInt;
  TORCH_CHECK(i32 || indices.scalar_type() == at::kLong,
              "ilu0_factor: indices must be int32 or int64");
  int64_t bad = n;
  AT_DISPATCH_FLOATING_AND_COMPLEX_TYPES(
      values.scalar_type(), "ilu0_factor", [&] {
        scalar_t* v = values.data_ptr<scalar_t>();
        const int64_t* dp = diag_ptr.data_ptr<int64_t>();
        bad = i32 ? ilu0_factor_impl(ip, indices.data_ptr<int32_t>(), v, dp, n)
                  : ilu0_factor_impl(ip, indices.data_ptr<int64_t>(), v, dp, n);
      });
  int64_t* fl = flag.data_ptr<int64_t>();
  if (bad < n) fl[0] = std::min(fl[0], bad);
}

TORCH_LIBRARY(sparse_hip, m) {
  m.def("spmv(Tensor indptr, Tensor indices, Tensor values, Tensor x, "
        "Tensor(a!) y, int col_lo, float beta) -> ()");
  m.def("add_nnz(Tensor aip, Tensor aix, Tensor bip, Tensor bix, "
        "Tensor(a!) out) -> ()");
  m.def("add_compute(Tensor aip, Tensor aix, Tensor av, Tensor bip, "
        "Tensor bix, Tensor bv, Tensor cip, Tensor(a!) cix, Tensor(b!) cv, "
        "float alpha, float beta) -> ()");
  m.def("mult_nnz(Tensor aip, Tensor aix, Tensor bip, Tensor bix, "
        "Tensor(a!) out) -> ()");
  m.def("mult_compute(Tensor aip, Tensor aix, Tensor av, Tensor bip, "
        "Tensor bix, Tensor bv, Tensor cip, Tensor(a!) cix, Tensor(b!) cv) -> ()");
  m.def("mult_dense(Tensor indptr, Tensor indices, Tensor vals, Tensor D, "
        "Tensor(a!) out) -> ()");
  m.def("axpby(Tensor(a!) y, Tensor x, Tensor a, Tensor b, bool isalpha, "
        "bool negate, int nt=-1) -> ()");
  m.def("spmv_dot(Tensor indptr, Tensor indices, Tensor values, Tensor x, "
        "Tensor(a!) y, Tensor pvec, Tensor(b!) dot_out, int col_lo) -> ()");
  m.def("axpby_norm2(Tensor(a!) y, Tensor x, Tensor a, Tensor b, bool isalpha, "
        "bool negate, Tensor(b!) dot_out) -> ()");
  m.def("build_ell(Tensor indptr, Tensor indices, Tensor values, "
        "Tensor(a!) eidx, Tensor(b!) evals, int W, int pad_idx) -> ()");
  m.def("build_dia(Tensor indptr, Tensor indices, Tensor values, "
        "Tensor offs, Tensor(a!) dvals, int W, int row0) -> ()");
  m.def("ell_spmv(Tensor eidx, Tensor evals, Tensor hlo, Tensor own, "
        "Tensor hhi, Tensor(a!) y, int W, int m, int col_lo, "
        "int rbase, int rhi) -> ()");
  m.def("ell_spmv_dot(Tensor eidx, Tensor evals, Tensor hlo, Tensor own, "
        "Tensor hhi, Tensor(a!) y, Tensor pvec, int W, int m, int col_lo, "
        "int rbase, int rhi) -> Tensor");
  m.def("ell_jacobi(Tensor eidx, Tensor evals, Tensor hlo, Tensor own, "
        "Tensor hhi, Tensor xloc, Tensor b, Tensor dinv, Tensor(a!) xout, "
        "int W, int m, int col_lo, float omega) -> ()");
  m.def("cg_xr_norm2(Tensor(a!) x, Tensor p, Tensor(b!) r, Tensor q, "
        "Tensor a, Tensor b, Tensor(c!) dot_out, int nt=-1) -> ()");
  m.def("dia_classify(Tensor dvals, Tensor(a!) cvals, Tensor(b!) mask, "
        "Tensor(c!) ok, int W) -> ()");
  m.def("dia_spmv_bpdot(Tensor planes, Tensor? mask, Tensor offs, "
        "Tensor r_hlo, Tensor r_own, "
        "Tensor r_hhi, Tensor p_hlo, Tensor p_own, Tensor p_hhi, "
        "Tensor(a!) pnew, Tensor(b!) q, Tensor beta_num, Tensor beta_den, "
        "int W, int m, int col_lo, int row0, int wsize, int adj=0) "
        "-> Tensor");
  m.def("dia_spmv(Tensor planes, Tensor? mask, Tensor offs, Tensor hlo, "
        "Tensor own, "
        "Tensor hhi, Tensor(a!) y, int W, int m, int col_lo, int row0, "
        "int wsize, int rbase, int rhi, int adj=0) -> ()");
  m.def("dia_spmv_dot(Tensor planes, Tensor? mask, Tensor offs, Tensor hlo, "
        "Tensor own, "
        "Tensor hhi, Tensor(a!) y, Tensor pvec, int W, int m, int col_lo, "
        "int row0, int wsize, int rbase, int rhi, int adj=0) -> Tensor");
  m.def("dia_residual(Tensor planes, Tensor? mask, Tensor offs, Tensor hlo, "
        "Tensor own, "
        "Tensor hhi, Tensor b, Tensor(a!) y, int W, int m, int col_lo, "
        "int row0, int wsize, int rbase, int rhi, int adj=0) -> ()");
  m.def("dia_jacobi(Tensor planes, Tensor? mask, Tensor offs, Tensor hlo, "
        "Tensor own, "
        "Tensor hhi, Tensor xloc, Tensor b, Tensor dinv, Tensor(a!) xout, "
        "int W, int m, int col_lo, int row0, int wsize, float omega, "
        "int rbase, int rhi, int adj=0) -> ()");
  m.def("spmm(Tensor indptr, Tensor indices, Tensor vals, Tensor B, "
        "Tensor(a!) C, int col_lo) -> ()");
  m.def("rspmm(Tensor indptr, Tensor indices, Tensor vals, Tensor A, "
        "Tensor(a!) C) -> ()");
  m.def("bsr_spmm(Tensor bptr, Tensor bcol, Tensor bvals, Tensor B, "
        "Tensor(a!) C, int col_lo) -> ()");
  m.def("sddmm(Tensor indptr, Tensor indices, Tensor vals, Tensor C, "
        "Tensor D, Tensor(a!) out, int col_lo) -> ()");
  m.def("csr_to_dense(Tensor indptr, Tensor indices, Tensor vals, "
        "Tensor(a!) out) -> ()");
  m.def("coo_to_csr(Tensor rows, Tensor cols, Tensor vals, Tensor(a!) cursor, "
        "Tensor indptr, Tensor(b!) out_idx, Tensor(c!) out_vals, "
        "Tensor(d!) flags) -> ()");
  m.def("dense_to_csr(Tensor D, Tensor(a!) indptr_or_counts, "
        "Tensor(b!) indices, Tensor(c!) vals, bool fill) -> ()");
  m.def("csr_diagonal(Tensor indptr, Tensor indices, Tensor vals, "
        "Tensor(a!) out, int row_offset) -> ()");
  m.def("csc_spmv(Tensor colptr, Tensor rowidx, Tensor vals, Tensor x, "
        "Tensor(a!) y, int rlo) -> ()");
  m.def("csc_spmm(Tensor colptr, Tensor rowidx, Tensor vals, Tensor B, "
        "Tensor(a!) C, int rlo) -> ()");
  m.def("tropical_spmv(Tensor indptr, Tensor indices, Tensor x, "
        "Tensor(a!) y, int col_lo) -> ()");
  m.def("rk_calc_dy(Tensor K, Tensor avec, float h, Tensor(a!) dy) -> ()");
  m.def("cdist(Tensor XA, Tensor XB, Tensor(a!) out) -> ()");
  m.def("spgemm_nnz(Tensor aip, Tensor aix, Tensor bip, Tensor bix, "
        "Tensor rowlist, Tensor(a!) nnz_out, int a_col_lo, int hash_size) -> ()");
  m.def("spgemm_compute(Tensor aip, Tensor aix, Tensor av, Tensor bip, "
        "Tensor bix, Tensor bv, Tensor rowlist, Tensor cip, Tensor(a!) cix, "
        "Tensor(b!) cv, int a_col_lo, int hash_size) -> ()");
  m.def("trsv_solve(Tensor indptr, Tensor indices, Tensor values, "
        "Tensor diag, Tensor order, Tensor level_ptr, Tensor sched, Tensor b, "
        "Tensor(a!) x) -> ()");
  m.def("trsv_levels(Tensor indptr, Tensor indices, bool lower) -> Tensor");
  m.def("ilu0_factor(Tensor indptr, Tensor indices, Tensor(a!) values, "
        "Tensor diag_ptr, Tensor order, Tensor level_ptr, Tensor sched, "
        "Tensor(b!) flag) -> ()");
  m.def("fsai_factor(Tensor a_indptr, Tensor a_indices, Tensor a_values, "
        "Tensor p_indptr, Tensor p_indices, Tensor(a!) g_values, Tensor rows, "
        "int lanes, int max_m, Tensor work, Tensor(b!) flag) -> ()");
  m.def("color_round(Tensor indptr, Tensor indices, Tensor work_in, "
        "int nwork, int seed, Tensor(a!) colors, Tensor(b!) work_out, "
        "Tensor(c!) count) -> ()");
  m.def("color_greedy(Tensor indptr, Tensor indices, int seed) -> Tensor");
  m.def("mcgs_sweep(Tensor indptr, Tensor indices, Tensor values, "
        "Tensor diag, Tensor order, Tensor sched, Tensor b, Tensor(a!) x, "
        "bool backward) -> ()");
}

TORCH_LIBRARY_IMPL(sparse_hip, CUDA, m) {
  m.impl("spmv", spmv_hip);
  m.impl("add_nnz", add_nnz_hip);
  m.impl("add_compute", add_compute_hip);
  m.impl("mult_nnz", mult_nnz_hip);
  m.impl("mult_compute", mult_compute_hip);
  m.impl("mult_dense", mult_dense_hip);
  m.impl("axpby", axpby_hip);
  m.impl("spmv_dot", spmv_dot_hip);
  m.impl("axpby_norm2", axpby_norm2_hip);
  m.impl("build_ell", build_ell_hip);
  m.impl("build_dia", build_dia_hip);
  m.impl("ell_spmv", ell_spmv_plain_hip);
  m.impl("ell_spmv_dot", ell_spmv_dot_hip);
  m.impl("ell_jacobi", ell_jacobi_hip);
  m.impl("cg_xr_norm2", cg_xr_norm2_hip);
  m.impl("dia_classify", dia_classify_hip);
  m.impl("dia_spmv_bpdot", dia_spmv_bpdot_hip);
  m.impl("dia_spmv", dia_spmv_plain_hip);
  m.impl("dia_spmv_dot", dia_spmv_dot_hip);
  m.impl("dia_residual", dia_residual_hip);
  m.impl("dia_jacobi", dia_jacobi_hip);
  m.impl("spmm", spmm_hip);
  m.impl("rspmm", rspmm_hip);
  m.impl("bsr_spmm", bsr_spmm_hip);
  m.impl("sddmm", sddmm_hip);
  m.impl("csr_to_dense", csr_to_dense_hip);
  m.impl("coo_to_csr", coo_to_csr_hip);
  m.impl("dense_to_csr", dense_to_csr_hip);
  m.impl("csr_diagonal", csr_diagonal_hip);
  m.impl("csc_spmv", csc_spmv_hip);
  m.impl("csc_spmm", csc_spmm_hip);
  m.impl("tropical_spmv", tropical_spmv_hip);
  m.impl("rk_calc_dy", rk_calc_dy_hip);
  m.impl("cdist", cdist_hip);
  m.impl("spgemm_nnz", spgemm_nnz_hip);
  m.impl("spgemm_compute", spgemm_compute_hip);
  m.impl("trsv_solve", trsv_solve_hip);
  m.impl("ilu0_factor", ilu0_factor_hip);
  m.impl("fsai_factor", fsai_factor_hip);
  m.impl("color_round", color_round_hip);
  m.impl("mcgs_sweep", mcgs_sweep_hip);
}

TORCH_LIBRARY_IMPL(sparse_hip, CPU, m) {
  m.impl("trsv_levels", trsv_levels_cpu);
  m.impl("ilu0_factor", ilu0_factor_cpu);
  m.impl("color_greedy", color_greedy_cpu);
}
