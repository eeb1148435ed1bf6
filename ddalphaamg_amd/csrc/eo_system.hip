// eo_system.hip -- see eo_system.h.  Streaming kernels in the manner of blas.hip: one thread per (chunk row, site), 16-byte
// accesses, grids capped and grid-strided; the log det is a two-stage deterministic fp64 reduction.
#include "eo_system.h"
#include "blas_device.h"

namespace ddamg {

// ---- half fields ---------------------------------------------------------------------------------
// Work item i = (chunk row k, site s), s fastest: the chunked-SoA side is address i * CH, fully coalesced; the half-field side
// is the 16 (T = double) or 32 (T = float) contiguous bytes of reals k*CH .. of half site lex_of_site[s] >> 1.  A chunk never
// straddles the gamma5 boundary (12 reals: a multiple of 2 and of 4).
template <typename T, bool G5>
__global__ __launch_bounds__(BLK) void vec_from_half_kernel(T* __restrict__ dst, const double* __restrict__ half, const int* __restrict__ lex_of_site,
                                                            const unsigned char* __restrict__ parity, int par, int zero_other, int V) {
  constexpr int CH = Chunk<T>::CH;
  constexpr int ROWS = 24 / CH;
  const size_t total = (size_t)V * ROWS;
  for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLK) {
    const size_t k = i / (size_t)V, s = i - k * (size_t)V;
    typename Chunk<T>::vec v;
    if (parity[s] == par) {
      const double* p = half + (size_t)(lex_of_site[s] >> 1) * 24 + k * CH;
      const double sg = G5 && k * CH < 12 ? -1.0 : 1.0;
      const double2 a = ldv<double>(p);
      v.x = (T)(sg * a.x); v.y = (T)(sg * a.y);
      if constexpr (CH == 4) { const double2 b = ldv<double>(p + 2); v.z = (T)(sg * b.x); v.w = (T)(sg * b.y); }
    } else {
      if (!zero_other) continue;
      v.x = 0; v.y = 0;
      if constexpr (CH == 4) { v.z = 0; v.w = 0; }
    }
    stv<T>(dst + i * CH, v);
  }
}
template <typename T, bool G5>
__global__ __launch_bounds__(BLK) void vec_to_half_kernel(double* __restrict__ half, const T* __restrict__ src, const int* __restrict__ lex_of_site,
                                                          const unsigned char* __restrict__ parity, int par, int V) {
  constexpr int CH = Chunk<T>::CH;
  constexpr int ROWS = 24 / CH;
  const size_t total = (size_t)V * ROWS;
  for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLK) {
    const size_t k = i / (size_t)V, s = i - k * (size_t)V;
    if (parity[s] != par) continue;
    const typename Chunk<T>::vec v = ldv<T>(src + i * CH);
    double* p = half + (size_t)(lex_of_site[s] >> 1) * 24 + k * CH;
    const double sg = G5 && k * CH < 12 ? -1.0 : 1.0;
    stv<double>(p, make_double2(sg * (double)v.x, sg * (double)v.y));
    if constexpr (CH == 4) stv<double>(p + 2, make_double2(sg * (double)v.z, sg * (double)v.w));
  }
}

static void require_half_field(int V, int par) {
  DDAMG_REQUIRE(par == 0 || par == 1, "parity must be 0 (even) or 1 (odd)");
  DDAMG_REQUIRE(V > 0 && V % 2 == 0, "half fields need an even number of sites");
}

template <typename T>
void vec_from_half(T* dst, const double* half_dev, const int* lex_of_site, const unsigned char* parity, int par, bool zero_other, bool gamma5,
                   int V, hipStream_t st) {
  require_half_field(V, par);
  const dim3 grid(grid_for((size_t)V * (24 / Chunk<T>::CH)));
  if (gamma5) hipLaunchKernelGGL((vec_from_half_kernel<T, true>), grid, dim3(BLK), 0, st, dst, half_dev, lex_of_site, parity, par, (int)zero_other, V);
  else hipLaunchKernelGGL((vec_from_half_kernel<T, false>), grid, dim3(BLK), 0, st, dst, half_dev, lex_of_site, parity, par, (int)zero_other, V);
  DDAMG_HIP_CHECK(hipGetLastError());
}
template <typename T>
void vec_to_half(double* half_dev, const T* src, const int* lex_of_site, const unsigned char* parity, int par, bool gamma5, int V, hipStream_t st) {
  require_half_field(V, par);
  const dim3 grid(grid_for((size_t)V * (24 / Chunk<T>::CH)));
  if (gamma5) hipLaunchKernelGGL((vec_to_half_kernel<T, true>), grid, dim3(BLK), 0, st, half_dev, src, lex_of_site, parity, par, V);
  else hipLaunchKernelGGL((vec_to_half_kernel<T, false>), grid, dim3(BLK), 0, st, half_dev, src, lex_of_site, parity, par, V);
  DDAMG_HIP_CHECK(hipGetLastError());
}

// ---- updates on the sites of one parity ------------------------------------------------------------
// x and e may be one array where e is not read (Zero): no __restrict__ on x
template <typename T, ParityOp OP, bool G5>
__global__ __launch_bounds__(BLK) void parity_update_kernel(T* x, const T* __restrict__ e, const unsigned char* __restrict__ parity, int par, int V) {
  constexpr int CH = Chunk<T>::CH;
  constexpr int ROWS = 24 / CH;
  const size_t total = (size_t)V * ROWS;
  for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < total; i += (size_t)gridDim.x * BLK) {
    const size_t k = i / (size_t)V, s = i - k * (size_t)V;
    if (parity[s] != par) continue;
    typename Chunk<T>::vec v;
    if constexpr (OP == ParityOp::Zero) {
      v.x = 0; v.y = 0;
      if constexpr (CH == 4) { v.z = 0; v.w = 0; }
    } else {
      const T sg = G5 && k * CH < 12 ? (T)-1 : (T)1;
      const typename Chunk<T>::vec ev = ldv<T>(e + i * CH);
      if constexpr (OP == ParityOp::Add) {
        v = ldv<T>(x + i * CH);
        v.x += sg * ev.x; v.y += sg * ev.y;
        if constexpr (CH == 4) { v.z += sg * ev.z; v.w += sg * ev.w; }
      } else {
        v.x = -(sg * ev.x); v.y = -(sg * ev.y);
        if constexpr (CH == 4) { v.z = -(sg * ev.z); v.w = -(sg * ev.w); }
      }
    }
    stv<T>(x + i * CH, v);
  }
}
template <typename T, ParityOp OP>
static void launch_parity_update(T* x, const T* e, const unsigned char* parity, int par, bool gamma5, int V, hipStream_t st) {
  const dim3 grid(grid_for((size_t)V * (24 / Chunk<T>::CH)));
  if (gamma5) hipLaunchKernelGGL((parity_update_kernel<T, OP, true>), grid, dim3(BLK), 0, st, x, e, parity, par, V);
  else hipLaunchKernelGGL((parity_update_kernel<T, OP, false>), grid, dim3(BLK), 0, st, x, e, parity, par, V);
  DDAMG_HIP_CHECK(hipGetLastError());
}
template <typename T>
void parity_update(T* x, const T* e, const unsigned char* parity, int par, ParityOp op, bool gamma5, int V, hipStream_t st) {
  DDAMG_REQUIRE(par == 0 || par == 1, "parity must be 0 (even) or 1 (odd)");
  DDAMG_REQUIRE(parity != nullptr && (op == ParityOp::Zero || (e != nullptr && e != x)), "parity_update: no parity table, or no second vector");
  if (op == ParityOp::Zero) launch_parity_update<T, ParityOp::Zero>(x, e, parity, par, false, V, st);
  else if (op == ParityOp::Add) launch_parity_update<T, ParityOp::Add>(x, e, parity, par, gamma5, V, st);
  else launch_parity_update<T, ParityOp::MinusAssign>(x, e, parity, par, gamma5, V, st);
}

// ---- the Schur complement ------------------------------------------------------------------------
template <typename T>
static T* work_vector(DeviceBuffer<T>& b, size_t n, hipStream_t st) {
  if (!b.get()) {
    b.alloc(n);
    // hop leaves the sites of its input parity alone: they are never read, and never hold what the allocator left there either
    DDAMG_HIP_CHECK(hipMemsetAsync(b.get(), 0, sizeof(T) * n, st));
  }
  DDAMG_REQUIRE(b.bytes() == sizeof(T) * n, "even-odd workspace of another lattice");
  return b.get();
}

template <typename T>
void schur_apply(const FineOp<T>& op, T* out, const T* in, bool dagger, EoWork& w, hipStream_t st) {
  DDAMG_REQUIRE(out != in, "schur_apply: in place");
  const size_t n = (size_t)24 * op.V();
  const unsigned char* parity = op.dev().parity;
  T* t = work_vector(w.t<T>(), n, st);
  const T* src = in;
  if (dagger) {
    T* g = work_vector(w.g<T>(), n, st);
    vec_gamma5<T>(g, in, whole(n), st);
    src = g;
  }
  op.hop(t, src, 1, st, 1);          // t_o = D_oo^-1 H_oe in_e
  op.hop(out, t, 0, st, 2, src);     // out_e = D_ee in_e - H_eo t_o
  if (dagger) vec_gamma5<T>(out, out, whole(n), st);
  parity_update<T>(out, nullptr, parity, 1, ParityOp::Zero, false, op.V(), st);
}

template <typename T>
const T* schur_odd_part(const FineOp<T>& op, const T* v, bool dagger, EoWork& w, hipStream_t st) {
  const size_t n = (size_t)24 * op.V();
  T* t = work_vector(w.t<T>(), n, st);
  const T* src = v;
  if (dagger) {
    T* g = work_vector(w.g<T>(), n, st);
    vec_gamma5<T>(g, v, whole(n), st);
    src = g;
  }
  op.hop(t, src, 1, st, 1);
  return t;
}

// ---- log det of the clover blocks of one parity ----------------------------------------------------
// index of the strict-upper entry (i, j), i < j, of a Hermitian 6x6 block in the packing of fine_op.h (row-major)
__host__ __device__ constexpr int herm6_up(int i, int j) { return 5 * i - i * (i - 1) / 2 + j - i - 1; }

// The pivots of one Hermitian 6x6 block, eliminated in place without pivoting in the order k = 0..5 of invert6_in_place
// (fine_op.hip), on the upper triangle alone: the trailing block stays Hermitian, so its diagonal -- the pivots -- stays
// real, a_ii -= |a_ki|^2 / p_k and a_ij -= conj(a_ki) a_kj / p_k.  Every index is a compile-time constant: 36 doubles in
// registers.  log|det| = sum log|p_k|, the sign of det that of the product; a block whose elimination meets a zero or
// non-finite pivot is counted in `bad` (the inverse kernel leaves its register path on such a block too).
__device__ __forceinline__ void herm6_pivots(double (&d)[6], double (&ur)[15], double (&ui)[15], double& logsum, double& neg, double& bad) {
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const double p = d[k];
    const bool ok = fabs(p) > 0.0 && fabs(p) < HUGE_VAL;   // false for NaN
    bad += ok ? 0.0 : 1.0;
    neg += p < 0.0 ? 1.0 : 0.0;
    logsum += log(fabs(p));
    const double ip = 1.0 / p;
#pragma unroll
    for (int i = k + 1; i < 6; i++) {
      const double ar = ur[herm6_up(k, i)], ai = ui[herm6_up(k, i)];
      const double lr = ar * ip, li = -ai * ip;                  // conj(a_ki) / p
      d[i] -= lr * ar - li * ai;
#pragma unroll
      for (int j = i + 1; j < 6; j++) {
        const double xr = ur[herm6_up(k, j)], xi = ui[herm6_up(k, j)];
        ur[herm6_up(i, j)] -= lr * xr - li * xi;
        ui[herm6_up(i, j)] -= lr * xi + li * xr;
      }
    }
  }
}

// One thread per site and pass of the grid-stride loop; the lanes whose site has the other parity load nothing.  Sites are
// ordered block by block with the two parities of a block apart (geometry.h), so the live lanes of a wavefront form runs of at
// least half a Schwarz block: every chunk-row load is made of whole 128-byte (2^4 blocks) to 1 KiB segments.
__global__ __launch_bounds__(BLK) void clover_logdet_kernel(const double* __restrict__ clover, const unsigned char* __restrict__ parity, int par, int V,
                                                            double* __restrict__ partial) {
  __shared__ double lds[3 * 4];
  double acc[3] = {0, 0, 0};
  for (size_t s = (size_t)blockIdx.x * BLK + threadIdx.x; s < (size_t)V; s += (size_t)gridDim.x * BLK) {
    if (parity[s] != par) continue;
#pragma unroll 1
    for (int b = 0; b < 2; b++) {   // one block at a time: half the registers, three waves per SIMD instead of one
      double cl[36], d[6], ur[15], ui[15];
      load_site<double, 36, true>(clover + (size_t)36 * b * V, (size_t)V, s, cl);
#pragma unroll
      for (int i = 0; i < 6; i++) d[i] = cl[i];
#pragma unroll
      for (int k = 0; k < 15; k++) { ur[k] = cl[6 + 2 * k]; ui[k] = cl[6 + 2 * k + 1]; }
      herm6_pivots(d, ur, ui, acc[0], acc[1], acc[2]);
    }
  }
  block_sum<3>(acc, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; k++) partial[3 * blockIdx.x + k] = acc[k];
  }
}

void clover_logdet(const double* clover64, const unsigned char* parity, int par, int V, ReduceWork& rw, double* d_out, hipStream_t st) {
  DDAMG_REQUIRE(par == 0 || par == 1, "parity must be 0 (even) or 1 (odd)");
  DDAMG_REQUIRE(clover64 != nullptr && parity != nullptr, "clover_logdet: no operator uploaded");
  const int gx = std::min(grid_for((size_t)V), rw.max_blocks);
  DDAMG_REQUIRE((size_t)3 * gx <= (size_t)rw.max_blocks * 2 * (rw.max_m + 2), "clover_logdet: reduction workspace too small");
  hipLaunchKernelGGL(clover_logdet_kernel, dim3(gx), dim3(BLK), 0, st, clover64, parity, par, V, rw.d_partial.get());
  DDAMG_HIP_CHECK(hipGetLastError());
  sum_partials(rw, gx, 3, d_out, st);
}

template void vec_from_half<float>(float*, const double*, const int*, const unsigned char*, int, bool, bool, int, hipStream_t);
template void vec_from_half<double>(double*, const double*, const int*, const unsigned char*, int, bool, bool, int, hipStream_t);
template void vec_to_half<float>(double*, const float*, const int*, const unsigned char*, int, bool, int, hipStream_t);
template void vec_to_half<double>(double*, const double*, const int*, const unsigned char*, int, bool, int, hipStream_t);
template void parity_update<float>(float*, const float*, const unsigned char*, int, ParityOp, bool, int, hipStream_t);
template void parity_update<double>(double*, const double*, const unsigned char*, int, ParityOp, bool, int, hipStream_t);
template void schur_apply<float>(const FineOp<float>&, float*, const float*, bool, EoWork&, hipStream_t);
template void schur_apply<double>(const FineOp<double>&, double*, const double*, bool, EoWork&, hipStream_t);
template const float* schur_odd_part<float>(const FineOp<float>&, const float*, bool, EoWork&, hipStream_t);
template const double* schur_odd_part<double>(const FineOp<double>&, const double*, bool, EoWork&, hipStream_t);

}  // namespace ddamg
