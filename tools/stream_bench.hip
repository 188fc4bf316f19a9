// CG vector-kernel shapes A/B at fp64: what the streaming kernels of the CG
// step gain from (1) issuing the vector loads ahead of the scalar preamble
// (two dependent scalar loads + the fp64 divide), (2) U chunks of 256 x 16 B
// per block, (3) no preamble at all, (4) non-temporal loads / stores.
//   K3: y = x + (a/b) y                       (2 reads, 1 write)
//   K2: x += (a/b) p ; r -= (a/b) q ; partial (4 reads, 2 writes, block sums)
// a, b are read through device pointers and divided in the kernel, as in the
// product.  Variants:
//   parent  the product's order: divide first, then the loads, U = 1
//   lfU     loads first, U chunks per block (chunks 4 KB apart)
//   nopre   lf1 with s handed in by value (no scalar loads, no divide):
//           the most that any treatment of the preamble can give
//   ntr     lf1, non-temporal loads of the read-only streams
//   ntl     lf1, non-temporal loads of every stream
//   ntls    lf1, non-temporal loads and stores
//   ntrs    lf1, non-temporal loads of the read-only streams and stores
//   nts     lf1, non-temporal stores alone
// and the pair K2 then K3 on the CG step's vectors, as parent, as ntr, and
// with only one of the two as ntr (K2/K3).
// Interleaved rounds; median, min and max over the rounds are printed.
//   hipcc -O3 --offload-arch=gfx950 tools/stream_bench.hip -o stream_bench
//   ./stream_bench [rounds]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>
#define CHECK(c) do { hipError_t e=(c); if(e!=hipSuccess){printf("ERR %s %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while(0)

struct alignas(16) D2 { double v[2]; };
typedef double v2d __attribute__((ext_vector_type(2)));

template <bool NT>
__device__ __forceinline__ D2 ld(const D2* p) {
  if constexpr (NT) {
    const v2d t = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p));
    return D2{{t.x, t.y}};
  } else {
    return *p;
  }
}
template <bool NT>
__device__ __forceinline__ void st(D2* p, const D2& d) {
  if constexpr (NT) {
    v2d t; t.x = d.v[0]; t.y = d.v[1];
    __builtin_nontemporal_store(t, reinterpret_cast<v2d*>(p));
  } else {
    *p = d;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
template <int N>
__device__ __forceinline__ double block_sums(const double (&v)[N]) {
  __shared__ double ws[N * 4];
  const int lane = threadIdx.x % 64, wid = threadIdx.x / 64;
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const double s = wave_sum(v[n]);
    if (lane == 0) ws[n * 4 + wid] = s;
  }
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x < N) {
    const double* w = ws + threadIdx.x * 4;
    s = ((w[0] + w[1]) + w[2]) + w[3];
  }
  return s;
}

// ---- parent order: scalars and divide first, then the loads (U = 1).  The
// scalar tail in block 0 thread 0 is what keeps hipcc from sinking the
// divide below the loads, so it is part of the shape.
__global__ __launch_bounds__(256) void k3_parent(
    double* __restrict__ y, const double* __restrict__ x,
    const double* __restrict__ a, const double* __restrict__ b, int64_t n) {
  const double s = (*a) / (*b);
  const int64_t nv = n / 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nv) {
    auto* y2 = reinterpret_cast<D2*>(y);
    auto* x2 = reinterpret_cast<const D2*>(x);
    D2 yv = y2[i];
    const D2 xv = x2[i];
#pragma unroll
    for (int j = 0; j < 2; ++j) yv.v[j] = xv.v[j] + s * yv.v[j];
    y2[i] = yv;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = nv * 2; t < n; ++t) y[t] = x[t] + s * y[t];
}

__global__ __launch_bounds__(256) void k2_parent(
    double* __restrict__ x, const double* __restrict__ p,
    double* __restrict__ r, const double* __restrict__ q,
    const double* __restrict__ a, const double* __restrict__ b,
    double* __restrict__ partial, int64_t n) {
  const double s = (*a) / (*b);
  double acc = 0.0;
  const int64_t nv = n / 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nv) {
    auto* x2 = reinterpret_cast<D2*>(x);
    auto* r2 = reinterpret_cast<D2*>(r);
    auto* p2 = reinterpret_cast<const D2*>(p);
    auto* q2 = reinterpret_cast<const D2*>(q);
    D2 xv = x2[i];
    D2 rv = r2[i];
    const D2 pv = p2[i];
    const D2 qv = q2[i];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      xv.v[j] += s * pv.v[j];
      rv.v[j] -= s * qv.v[j];
      acc += rv.v[j] * rv.v[j];
    }
    x2[i] = xv;
    r2[i] = rv;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = nv * 2; t < n; ++t) {
      x[t] += s * p[t];
      const double rt = r[t] - s * q[t];
      r[t] = rt;
      acc += rt * rt;
    }
  const double part[1] = {acc};
  const double sum = block_sums(part);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// ---- loads first, U chunks of 256 vectors per block.
// NT, what is non-temporal: bit 0 the loads of the read-only streams, bit 1
// the loads of the streams written back, bit 2 the stores.
// PRE: s = *a / *b in the kernel, else sval.
template <int U, int NT, bool PRE>
__global__ __launch_bounds__(256) void k3_lf(
    double* __restrict__ y, const double* __restrict__ x,
    const double* __restrict__ a, const double* __restrict__ b, double sval,
    int64_t n) {
  const int64_t nv = n / 2;
  auto* y2 = reinterpret_cast<D2*>(y);
  auto* x2 = reinterpret_cast<const D2*>(x);
  const int64_t i0 = (int64_t)blockIdx.x * (U * 256) + threadIdx.x;
  D2 yv[U], xv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = i0 + u * 256;
    if (i < nv) {
      yv[u] = ld<(NT & 2) != 0>(y2 + i);
      xv[u] = ld<(NT & 1) != 0>(x2 + i);
    }
  }
  const double s = PRE ? (*a) / (*b) : sval;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = i0 + u * 256;
    if (i < nv) {
#pragma unroll
      for (int j = 0; j < 2; ++j) yv[u].v[j] = xv[u].v[j] + s * yv[u].v[j];
      st<(NT & 4) != 0>(y2 + i, yv[u]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = nv * 2; t < n; ++t) y[t] = x[t] + s * y[t];
}

template <int U, int NT, bool PRE>
__global__ __launch_bounds__(256) void k2_lf(
    double* __restrict__ x, const double* __restrict__ p,
    double* __restrict__ r, const double* __restrict__ q,
    const double* __restrict__ a, const double* __restrict__ b, double sval,
    double* __restrict__ partial, int64_t n, int64_t slots) {
  const int64_t nv = n / 2;
  auto* x2 = reinterpret_cast<D2*>(x);
  auto* r2 = reinterpret_cast<D2*>(r);
  auto* p2 = reinterpret_cast<const D2*>(p);
  auto* q2 = reinterpret_cast<const D2*>(q);
  const int64_t i0 = (int64_t)blockIdx.x * (U * 256) + threadIdx.x;
  D2 xv[U], rv[U], pv[U], qv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = i0 + u * 256;
    if (i < nv) {
      xv[u] = ld<(NT & 2) != 0>(x2 + i);
      rv[u] = ld<(NT & 2) != 0>(r2 + i);
      pv[u] = ld<(NT & 1) != 0>(p2 + i);
      qv[u] = ld<(NT & 1) != 0>(q2 + i);
    }
  }
  const double s = PRE ? (*a) / (*b) : sval;
  double acc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    acc[u] = 0.0;
    const int64_t i = i0 + u * 256;
    if (i < nv) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        xv[u].v[j] += s * pv[u].v[j];
        rv[u].v[j] -= s * qv[u].v[j];
        acc[u] += rv[u].v[j] * rv[u].v[j];
      }
      st<(NT & 4) != 0>(x2 + i, xv[u]);
      st<(NT & 4) != 0>(r2 + i, rv[u]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t t = nv * 2; t < n; ++t) {
      x[t] += s * p[t];
      const double rt = r[t] - s * q[t];
      r[t] = rt;
      acc[0] += rt * rt;
    }
  const double sum = block_sums<U>(acc);
  const int64_t slot = (int64_t)blockIdx.x * U + threadIdx.x;
  if (threadIdx.x < U && slot < slots) partial[slot] = sum;
}

__global__ void fill(double* p, int64_t n, double base) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = base + 1e-3 * (double)(i % 1021);
}

struct Bufs { double *x, *p, *r, *q, *a, *b, *partial; };
struct Variant { const char* name; std::function<void(int64_t)> run; };

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 9;
  const int64_t nmax = 268435456;
  // the headline vector, the matched configuration, and two that fit the
  // Infinity Cache and the L2s
  const int64_t sizes[4] = {268435456, 36000000, 8388608, 1048576};
  Bufs B;
  CHECK(hipMalloc(&B.x, nmax * 8)); CHECK(hipMalloc(&B.p, nmax * 8));
  CHECK(hipMalloc(&B.r, nmax * 8)); CHECK(hipMalloc(&B.q, nmax * 8));
  CHECK(hipMalloc(&B.a, 8)); CHECK(hipMalloc(&B.b, 8));
  CHECK(hipMalloc(&B.partial, ((nmax / 2 + 255) / 256 + 1) * 8));
  // s = a/b = 1e-3: p = r + s p stays bounded, x and r drift slowly
  const double ha = 1e-3, hb = 1.0, hs = ha / hb;
  CHECK(hipMemcpy(B.a, &ha, 8, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(B.b, &hb, 8, hipMemcpyHostToDevice));
  const dim3 fg((unsigned)((nmax + 255) / 256));
  hipLaunchKernelGGL(fill, fg, dim3(256), 0, 0, B.x, nmax, 0.5);
  hipLaunchKernelGGL(fill, fg, dim3(256), 0, 0, B.p, nmax, 1.0);
  hipLaunchKernelGGL(fill, fg, dim3(256), 0, 0, B.r, nmax, 2.0);
  hipLaunchKernelGGL(fill, fg, dim3(256), 0, 0, B.q, nmax, 0.25);
  CHECK(hipDeviceSynchronize());

  // one partial slot per chunk plus one, as the product sizes it
  auto slots_of = [](int64_t n) { return (n / 2 + 255) / 256 + 1; };
  auto grid = [&](int64_t n, int U) {
    return dim3((unsigned)((slots_of(n) + U - 1) / U));
  };
#define K3(U, NT, PRE)                                                      \
  [&](int64_t n) {                                                          \
    hipLaunchKernelGGL((k3_lf<U, NT, PRE>), grid(n, U), dim3(256), 0, 0,    \
                       B.p, B.r, B.a, B.b, hs, n);                          \
  }
#define K2(U, NT, PRE)                                                      \
  [&](int64_t n) {                                                          \
    hipLaunchKernelGGL((k2_lf<U, NT, PRE>), grid(n, U), dim3(256), 0, 0,    \
                       B.x, B.p, B.r, B.q, B.a, B.b, hs, B.partial, n,      \
                       slots_of(n));                                        \
  }
  std::vector<Variant> k3 = {
      {"parent", [&](int64_t n) {
         hipLaunchKernelGGL(k3_parent, grid(n, 1), dim3(256), 0, 0, B.p, B.r,
                            B.a, B.b, n); }},
      {"lf1", K3(1, 0, true)},   {"lf2", K3(2, 0, true)},
      {"lf4", K3(4, 0, true)},   {"lf8", K3(8, 0, true)},
      {"nopre", K3(1, 0, false)}, {"ntr", K3(1, 1, true)},
      {"ntl", K3(1, 3, true)},   {"ntls", K3(1, 7, true)},
      {"ntrs", K3(1, 5, true)},  {"nts", K3(1, 4, true)}};
  std::vector<Variant> k2 = {
      {"parent", [&](int64_t n) {
         hipLaunchKernelGGL(k2_parent, grid(n, 1), dim3(256), 0, 0, B.x, B.p,
                            B.r, B.q, B.a, B.b, B.partial, n); }},
      {"lf1", K2(1, 0, true)},   {"lf2", K2(2, 0, true)},
      {"lf4", K2(4, 0, true)},   {"nopre", K2(1, 0, false)},
      {"ntr", K2(1, 1, true)},   {"ntl", K2(1, 3, true)},
      {"ntls", K2(1, 7, true)},  {"ntrs", K2(1, 5, true)},
      {"nts", K2(1, 4, true)}};
  // K2 then K3 on the CG step's own vectors: K3 reads the r that K2 wrote and
  // the p that K2 read, so a cache that holds them shows here and only here
  std::vector<Variant> k23 = {
      {"parent", [&](int64_t n) { k2[0].run(n); k3[0].run(n); }},
      {"ntr", [&](int64_t n) { k2[5].run(n); k3[6].run(n); }},
      {"ntr/pl", [&](int64_t n) { k2[5].run(n); k3[0].run(n); }},
      {"pl/ntr", [&](int64_t n) { k2[0].run(n); k3[6].run(n); }}};

  hipEvent_t t0, t1; CHECK(hipEventCreate(&t0)); CHECK(hipEventCreate(&t1));
  for (int si = 0; si < 4; ++si) {
    const int64_t n = sizes[si];
    const int reps = n >= 32000000 ? 3 : 20;
    // kern 3: K3, 2: K2, 1: the K2+K3 pair
    for (int kern = 3; kern >= 1; --kern) {
      auto& vs = kern == 3 ? k3 : kern == 2 ? k2 : k23;
      const double bytes = (kern == 3 ? 3.0 : kern == 2 ? 6.0 : 9.0) * n * 8;
      std::vector<std::vector<float>> times(vs.size());
      for (auto& v : vs) v.run(n);  // warm-up
      CHECK(hipDeviceSynchronize());
      for (int round = 0; round < rounds; ++round)
        for (size_t vi = 0; vi < vs.size(); ++vi) {
          CHECK(hipEventRecord(t0));
          for (int rep = 0; rep < reps; ++rep) vs[vi].run(n);
          CHECK(hipEventRecord(t1)); CHECK(hipEventSynchronize(t1));
          float ms; CHECK(hipEventElapsedTime(&ms, t0, t1));
          times[vi].push_back(ms / reps);
        }
      CHECK(hipGetLastError());
      for (size_t vi = 0; vi < vs.size(); ++vi) {
        auto& t = times[vi];
        std::sort(t.begin(), t.end());
        const float med = t[t.size() / 2];
        printf("%-5s n=%-10lld %-7s med %8.1f us  min %8.1f  max %8.1f  %7.1f GB/s\n",
               kern == 3 ? "K3" : kern == 2 ? "K2" : "K2+K3", (long long)n,
               vs[vi].name, med * 1e3, t.front() * 1e3,
               t.back() * 1e3, bytes / (med * 1e6));
      }
      fflush(stdout);
    }
  }
  return 0;
}
