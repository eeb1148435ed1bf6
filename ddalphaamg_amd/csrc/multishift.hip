// multishift.hip -- see multishift.h.  Streaming kernels in the manner of blas.hip and eo_system.hip: one thread per (chunk row,
// even site), 16-byte accesses, grids capped and grid-strided; the norm is a two-stage deterministic fp64 reduction.
#include "multishift.h"
#include "blas_device.h"
#include <algorithm>
#include <cmath>

namespace ddamg {

constexpr int ROWS = 12;   // chunk rows of an fp64 fine vector: 24 reals per site in double2

void multishift_prepare(MultishiftWork& w, const std::vector<int>& parity, hipStream_t st) {
  const int V = (int)parity.size();
  if (w.ready && w.V == V) return;
  std::vector<int> even;
  even.reserve(V / 2);
  for (int s = 0; s < V; s++)
    if (parity[s] == 0) even.push_back(s);
  DDAMG_REQUIRE((int)even.size() * 2 == V, "multishift: the even sites are not half of the lattice");
  if (!w.ready) w.rw.init(3 * MS_MAX_SHIFTS + 4);
  DDAMG_REQUIRE(MS_COEF_MAX <= 2 * w.rw.max_m + 8, "multishift: coefficient buffer too small");
  w.even_site.alloc(even.size());
  DDAMG_HIP_CHECK(hipMemcpyAsync(w.even_site.get(), even.data(), sizeof(int) * even.size(), hipMemcpyHostToDevice, st));
  DDAMG_HIP_CHECK(hipStreamSynchronize(st));   // `even` leaves scope
  w.V = V;
  w.ready = true;
}

// ---- packed fields ---------------------------------------------------------------------------------
template <bool GATHER>
__global__ __launch_bounds__(BLK) void ms_pack_kernel(double* __restrict__ dst, const double* __restrict__ src, const int* __restrict__ even_site, int V) {
  const size_t Vh = (size_t)V / 2, total = ROWS * Vh;
  for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLK) {
    const size_t k = i / Vh, j = i - k * Vh;
    const size_t f = (k * (size_t)V + (size_t)even_site[j]) * 2;
    if constexpr (GATHER) stv<double>(dst + i * 2, ldv<double>(src + f));
    else stv<double>(dst + f, ldv<double>(src + i * 2));
  }
}
void multishift_gather(double* packed, const double* full, const int* even_site, int V, hipStream_t st) {
  hipLaunchKernelGGL(ms_pack_kernel<true>, dim3(grid_for((size_t)ROWS * (V / 2))), dim3(BLK), 0, st, packed, full, even_site, V);
  DDAMG_HIP_CHECK(hipGetLastError());
}
void multishift_scatter(double* full, const double* packed, const int* even_site, int V, hipStream_t st) {
  hipLaunchKernelGGL(ms_pack_kernel<false>, dim3(grid_for((size_t)ROWS * (V / 2))), dim3(BLK), 0, st, full, packed, even_site, V);
  DDAMG_HIP_CHECK(hipGetLastError());
}

// ---- the base system's residual and its norm ----------------------------------------------------------
__global__ __launch_bounds__(BLK) void ms_residual_kernel(double* __restrict__ r, const double* __restrict__ u, const double* __restrict__ p, double alpha,
                                                          double sigma, const int* __restrict__ even_site, int V, double* __restrict__ partial) {
  __shared__ double lds[4];
  double acc[1] = {0};
  const size_t Vh = (size_t)V / 2, total = ROWS * Vh;
  for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLK) {
    const size_t k = i / Vh, j = i - k * Vh;
    const size_t f = (k * (size_t)V + (size_t)even_site[j]) * 2;
    const double2 uv = ldv<double>(u + f), pv = ldv<double>(p + f);
    double2 rv = ldv<double>(r + f);
    rv.x = fma(-alpha, fma(sigma, pv.x, uv.x), rv.x);
    rv.y = fma(-alpha, fma(sigma, pv.y, uv.y), rv.y);
    stv<double>(r + f, rv);
    acc[0] += rv.x * rv.x + rv.y * rv.y;
  }
  block_sum<1>(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc[0];
}
void multishift_residual(double* r, const double* u, const double* p, double alpha, double sigma, const int* even_site, int V, ReduceWork& rw,
                         double* d_out, hipStream_t st) {
  const int gx = std::min(grid_for((size_t)ROWS * (V / 2)), std::min(rw.max_blocks, 1024));
  hipLaunchKernelGGL(ms_residual_kernel, dim3(gx), dim3(BLK), 0, st, r, u, p, alpha, sigma, even_site, V, rw.d_partial.get());
  DDAMG_HIP_CHECK(hipGetLastError());
  sum_partials(rw, gx, 1, d_out, st);
}

// ---- the update of every active shift in one pass ------------------------------------------------------
// Work item i = (chunk row k, even site j), j fastest; each thread owns one complex number (double2, 16 bytes) of every field.
// r is read once per item and serves the base system and every active shift.  The list of active shifts and their three reals
// are uniform loads from d_coef, so one compiled kernel and one launch serve any set of shifts; a shift's arithmetic is two
// fused multiply-adds and one product with its own reals only, whatever its slot and whoever else is active.
//
// Loads and stores.  x_s and p_s are streams: each 16 bytes are read once and written once per launch and not looked at again
// before the next iteration, with 2 * n_active fields of 12 * V * 8 bytes in between -- beyond any cache from 16^4 up.  Their
// LOADS are non-temporal: on this part that makes them bypass the vector L1 only (they are served by the L2 at the rate of plain
// 16-byte loads, to a few per cent), which leaves the L1 to even_site, whose every entry is read by the twelve chunk rows, and to
// the partly used lines of r and of the base p at the ends of a run of even sites (half a Schwarz block, as short as 128 bytes).
// r and the base p are loaded plainly.  All STORES are plain: plain and non-temporal 16-byte
// stores behave alike here (every byte leaves the L2 on each pass and the line stays in the L2 of the writing XCD either way),
// so a non-temporal store would buy nothing, and the write-through flavours that drop the line would make the next reader of p
// pay the cross-XCD rate.
__global__ __launch_bounds__(BLK) void multishift_update_kernel(double* __restrict__ p, const double* __restrict__ r, double* __restrict__ xs,
                                                                double* __restrict__ ps, const double* __restrict__ coef,
                                                                const int* __restrict__ even_site, int V) {
  const size_t Vh = (size_t)V / 2, total = ROWS * Vh, half = total * 2;
  const int nact = (int)coef[0];
  const double beta = coef[1], alpha = coef[2];
  const int base_slot = (int)coef[3];
  for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLK) {
    const size_t k = i / Vh, j = i - k * Vh;
    const size_t f = (k * (size_t)V + (size_t)even_site[j]) * 2;
    const double2 rv = ldv<double>(r + f);
    double2 pv = ldv<double>(p + f);
    if (base_slot >= 0) {
      double* xb = xs + (size_t)base_slot * half + i * 2;
      double2 xv = ldv_stream<double, true>(xb);
      xv.x = fma(alpha, pv.x, xv.x);
      xv.y = fma(alpha, pv.y, xv.y);
      stv<double>(xb, xv);
    }
    pv.x = fma(beta, pv.x, rv.x);
    pv.y = fma(beta, pv.y, rv.y);
    stv<double>(p + f, pv);
#pragma unroll 2
    for (int a = 0; a < nact; a++) {
      const double* cf = coef + MS_COEF_HEAD + MS_COEF_PER * a;
      const size_t o = (size_t)(int)cf[0] * half + i * 2;
      const double as = cf[1], bs = cf[2], zs = cf[3];
      double2 xv = ldv_stream<double, true>(xs + o), qv = ldv_stream<double, true>(ps + o);
      xv.x = fma(as, qv.x, xv.x);
      xv.y = fma(as, qv.y, xv.y);
      qv.x = fma(bs, qv.x, zs * rv.x);
      qv.y = fma(bs, qv.y, zs * rv.y);
      stv<double>(xs + o, xv);
      stv<double>(ps + o, qv);
    }
  }
}
void multishift_update(double* p, const double* r, double* xs, double* ps, const double* d_coef, const int* even_site, int V, hipStream_t st) {
  hipLaunchKernelGGL(multishift_update_kernel, dim3(grid_for((size_t)ROWS * (V / 2))), dim3(BLK), 0, st, p, r, xs, ps, d_coef, even_site, V);
  DDAMG_HIP_CHECK(hipGetLastError());
}

// ---- Ritz values -----------------------------------------------------------------------------------
// number of eigenvalues of the symmetric tridiagonal matrix (d, e) below x: the negative terms of the Sturm sequence
static int sturm_count(const std::vector<double>& d, const std::vector<double>& e2, double x) {
  int cnt = 0;
  double q = 1.0;
  for (size_t j = 0; j < d.size(); j++) {
    q = d[j] - x - (j > 0 ? e2[j - 1] / q : 0.0);
    if (q == 0.0) q = -1e-300;
    if (q < 0) cnt++;
  }
  return cnt;
}
void lanczos_extremes(const std::vector<double>& alpha, const std::vector<double>& beta, double out[2]) {
  const size_t n = alpha.size();
  out[0] = out[1] = 0.0;
  if (n == 0) return;
  std::vector<double> d(n), e2(n > 1 ? n - 1 : 0);
  for (size_t j = 0; j < n; j++) {
    d[j] = 1.0 / alpha[j] + (j > 0 ? beta[j - 1] / alpha[j - 1] : 0.0);
    if (j + 1 < n) e2[j] = beta[j] / (alpha[j] * alpha[j]);
  }
  double lo = d[0], hi = d[0];   // Gershgorin
  for (size_t j = 0; j < n; j++) {
    const double rad = (j > 0 ? std::sqrt(e2[j - 1]) : 0.0) + (j + 1 < n ? std::sqrt(e2[j]) : 0.0);
    lo = std::min(lo, d[j] - rad);
    hi = std::max(hi, d[j] + rad);
  }
  const double pad = 1e-12 * std::max(std::fabs(lo), std::fabs(hi));
  lo -= pad; hi += pad;
  for (int which = 0; which < 2; which++) {
    // the eigenvalue number m (0: the smallest, n-1: the largest) lies where the count passes from <= m to > m
    const int m = which == 0 ? 0 : (int)n - 1;
    double a = lo, b = hi;
    for (int it = 0; it < 200 && b - a > 4e-16 * std::max(std::fabs(a), std::fabs(b)); it++) {
      const double mid = 0.5 * (a + b);
      if (sturm_count(d, e2, mid) > m) b = mid; else a = mid;
    }
    out[which] = 0.5 * (a + b);
  }
}

}  // namespace ddamg
