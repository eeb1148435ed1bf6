// chrono.hip -- see chrono.h.  Bandwidth-bound streaming kernels in the manner of blas.hip: 16-byte accesses, grid-stride over a
// grid sized to the device, the column count a template parameter so that the coefficients sit in registers.
#include "chrono.h"
#include "blas_device.h"
#include <type_traits>

namespace ddamg {

// f(std::integral_constant<int, M>) for the M in 1..CHRONO_MAX that equals m
template <int M = 1, typename F>
static void with_columns(int m, F f) {
  if (m == M) f(std::integral_constant<int, M>{});
  else if constexpr (M < CHRONO_MAX) with_columns<M + 1>(m, f);
}

// r and b may be one array: no __restrict__ on them
__global__ __launch_bounds__(BLK) void chrono_residual_kernel(double* r, const double* b, const double* __restrict__ y, View v, double* __restrict__ partial) {
  __shared__ double lds[2 * 4];
  double acc[2] = {0, 0};
  const size_t nchunks = v.total() / 2;
  for (size_t c = (size_t)blockIdx.x * BLK + threadIdx.x; c < nchunks; c += (size_t)gridDim.x * BLK) {
    const size_t a = chunk_addr<double>(v, c);
    const double2 bv = ldv<double>(b + a), yv = ldv<double>(y + a);
    const double2 rv = make_double2(bv.x - yv.x, bv.y - yv.y);
    acc[0] += bv.x * bv.x + bv.y * bv.y;
    acc[1] += rv.x * rv.x + rv.y * rv.y;
    stv<double>(r + a, rv);
  }
  block_sum<2>(acc, lds);
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = acc[0]; partial[2 * blockIdx.x + 1] = acc[1]; }
}
void chrono_residual(double* r, const double* b, const double* y, View v, ReduceWork& rw, double* d_out, hipStream_t st) {
  DDAMG_REQUIRE(v.len % 2 == 0 && v.off % 2 == 0 && v.stride % 2 == 0, "vector view must be 16-byte aligned");
  const int gx = std::min(grid_for(v.total() / 2), 1024);
  hipLaunchKernelGGL(chrono_residual_kernel, dim3(gx), dim3(BLK), 0, st, r, b, y, v, rw.d_partial);
  DDAMG_HIP_CHECK(hipGetLastError());
  sum_partials(rw, gx, 2, d_out, st);
}

// t -= sum_i (hr[i], hi[i]) * X_i at one chunk
template <int M, bool NT>
__device__ __forceinline__ double2 minus_columns(double2 t, const double* __restrict__ X, size_t stride, size_t a, const double (&hr)[M], const double (&hi)[M]) {
#pragma unroll
  for (int i = 0; i < M; i++) {
    const double2 xv = ldv_stream<double, NT>(X + (size_t)i * stride + a);
    t.x -= hr[i] * xv.x - hi[i] * xv.y;
    t.y -= hr[i] * xv.y + hi[i] * xv.x;
  }
  return t;
}

template <int M, bool NT>
__global__ __launch_bounds__(BLK) void chrono_project_pair_kernel(double* __restrict__ q, const double* __restrict__ Q, double* __restrict__ w,
                                                                  const double* __restrict__ W, size_t stride, const double* __restrict__ h, View v) {
  double hr[M], hi[M];
#pragma unroll
  for (int i = 0; i < M; i++) { hr[i] = h[2 * i]; hi[i] = h[2 * i + 1]; }
  // blockIdx.y picks the family: every workgroup streams M + 2 vectors, as one of vec_multi_axpy_dev does
  double* __restrict__ t = blockIdx.y ? w : q;
  const double* __restrict__ X = blockIdx.y ? W : Q;
  const size_t nchunks = v.total() / 2;
  for (size_t c = (size_t)blockIdx.x * BLK + threadIdx.x; c < nchunks; c += (size_t)gridDim.x * BLK) {
    const size_t a = chunk_addr<double>(v, c);
    stv<double>(t + a, minus_columns<M, NT>(ldv<double>(t + a), X, stride, a, hr, hi));
  }
}
void chrono_project_pair(double* q, const double* Q, double* w, const double* W, size_t stride, int m, const double* d_h, View v, hipStream_t st) {
  DDAMG_REQUIRE(m >= 1 && m <= CHRONO_MAX, "chrono_project_pair: 1 <= columns <= 8");
  DDAMG_REQUIRE(v.len % 2 == 0 && v.off % 2 == 0 && v.stride % 2 == 0 && stride % 2 == 0, "vector view must be 16-byte aligned");
  if (v.total() == 0) return;
  const dim3 grid(grid_for(v.total() / 2), 2);
  with_columns(m, [&](auto columns) {
    constexpr int M = decltype(columns)::value;
    if (stream_sized(v, sizeof(double))) hipLaunchKernelGGL((chrono_project_pair_kernel<M, true>), grid, dim3(BLK), 0, st, q, Q, w, W, stride, d_h, v);
    else hipLaunchKernelGGL((chrono_project_pair_kernel<M, false>), grid, dim3(BLK), 0, st, q, Q, w, W, stride, d_h, v);
  });
  DDAMG_HIP_CHECK(hipGetLastError());
}

template <int M, bool NT>
__global__ __launch_bounds__(BLK) void chrono_combine_kernel(double* __restrict__ x, const double* __restrict__ W, double* __restrict__ r,
                                                             const double* __restrict__ b, const double* __restrict__ Q, size_t stride,
                                                             const double* __restrict__ coef, View v) {
  double cr[M], ci[M];
#pragma unroll
  for (int i = 0; i < M; i++) { cr[i] = coef[2 * i]; ci[i] = coef[2 * i + 1]; }
  const size_t nchunks = v.total() / 2;
  for (size_t c = (size_t)blockIdx.x * BLK + threadIdx.x; c < nchunks; c += (size_t)gridDim.x * BLK) {
    const size_t a = chunk_addr<double>(v, c);
    if (blockIdx.y) {   // the family by workgroup, as in the pair projection
      stv<double>(r + a, minus_columns<M, NT>(ldv<double>(b + a), Q, stride, a, cr, ci));
    } else {
      const double2 s = minus_columns<M, NT>(make_double2(0, 0), W, stride, a, cr, ci);
      stv<double>(x + a, make_double2(-s.x, -s.y));
    }
  }
}
void chrono_combine(double* x, const double* W, double* r, const double* b, const double* Q, size_t stride, int m, const double* d_c, View v,
                    hipStream_t st) {
  DDAMG_REQUIRE(m >= 1 && m <= CHRONO_MAX, "chrono_combine: 1 <= columns <= 8");
  DDAMG_REQUIRE(v.len % 2 == 0 && v.off % 2 == 0 && v.stride % 2 == 0 && stride % 2 == 0, "vector view must be 16-byte aligned");
  if (v.total() == 0) return;
  const dim3 grid(grid_for(v.total() / 2), 2);
  with_columns(m, [&](auto columns) {
    constexpr int M = decltype(columns)::value;
    if (stream_sized(v, sizeof(double))) hipLaunchKernelGGL((chrono_combine_kernel<M, true>), grid, dim3(BLK), 0, st, x, W, r, b, Q, stride, d_c, v);
    else hipLaunchKernelGGL((chrono_combine_kernel<M, false>), grid, dim3(BLK), 0, st, x, W, r, b, Q, stride, d_c, v);
  });
  DDAMG_HIP_CHECK(hipGetLastError());
}

}  // namespace ddamg
