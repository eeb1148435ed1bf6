// coarse_half.hip -- see coarse_half.h.  The kernels are coarse_site_kernel's hopping-term and self-coupling forms
// (coarse_op.hip) on the 16-bit copy: one workgroup per output site, one wavefront per dense n x n product, every product
// streams its matrix once, in 16-byte loads per lane, converts in registers and accumulates in fp32.
#include "coarse_half.h"
#include "coarse_half_device.h"

namespace ddamg {

enum { HALF_HOP = 1, HALF_SELF = 2, HALF_SELFINV = 3 };   // template argument of coarse_half_kernel: one instantiation, one name in kernel statistics, per product

// HALF_HOP: out(x) (+)= sign * sum of the 8 hopping terms, wavefronts 0-3 the forward links of x, 4-7 the backward couplings
// from the forward links of the neighbours (G5 U^H G5);  HALF_SELF / HALF_SELFINV: out(x) = M0 in(x) / M0^-1 in(x), one wavefront.
// The neighbour table holds sites only: the copy is not made for a level that is decomposed over processes.
template <int NT, int mode>
__global__ __launch_bounds__(mode == HALF_HOP ? 512 : 64) void coarse_half_kernel(float* __restrict__ out, const float* __restrict__ in, CoarseHalfDev op,
                                                                                  int s0, float sign, int accumulate, int swizzle) {
  constexpr int np = 8 * NT, NW = mode == HALF_HOP ? 8 : 1;
  __shared__ float res[NW * 2 * np];
  // the XCD swizzle and the alternating direction of coarse_site_kernel
  int bid = blockIdx.x;
  if (swizzle & 2) bid = gridDim.x - 1 - bid;
  if (swizzle & 1) {
    const int chunk = gridDim.x >> 3;
    if (bid < chunk * 8) bid = (bid & 7) * chunk + (bid >> 3);
  }
  const int x = s0 + bid;
  const int w = threadIdx.x >> 6;
  const int n = op.n;
  const size_t V = op.V;
  float* r = res + (size_t)w * 2 * np;
  if (mode == HALF_SELF) {
    wave_mv_half<NT, false>(op.M + (size_t)x * 5 * op.msize, op.scale[(size_t)x * 6], in + (size_t)x * n * 2, n, r);
  } else if (mode == HALF_SELFINV) {
    wave_mv_half<NT, false>(op.Minv + (size_t)x * op.msize, op.scale[(size_t)x * 6 + 5], in + (size_t)x * n * 2, n, r);
  } else if (w < 4) {
    const int mu = w;
    const int y = op.nb[(size_t)mu * V + x];
    wave_mv_half<NT, false>(op.M + ((size_t)x * 5 + 1 + mu) * op.msize, op.scale[(size_t)x * 6 + 1 + mu], in + (size_t)y * n * 2, n, r);
  } else {
    const int mu = w - 4;
    const int y = op.nb[(size_t)(4 + mu) * V + x];
    wave_mv_half<NT, true>(op.M + ((size_t)y * 5 + 1 + mu) * op.msize, op.scale[(size_t)y * 6 + 1 + mu], in + (size_t)y * n * 2, n, r);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * n; k += blockDim.x) {
    float v = accumulate ? out[(size_t)x * n * 2 + k] : 0.f;
    if (mode == HALF_HOP) {
      float s = 0;
      for (int ww = 0; ww < NW; ww++) s += res[(size_t)ww * 2 * np + k];
      v += sign * s;
    } else {
      v += res[k];
    }
    out[(size_t)x * n * 2 + k] = v;
  }
}

// one workgroup per site and matrix m (m0 + blockIdx.y: 0-4 the couplings, 5 the inverted self coupling): the largest
// |re| or |im| of the n x n entries, then the scaled entries in the order of coarse_half.h, padding as zeros
__global__ __launch_bounds__(256) void coarse_half_build_kernel(__half2* __restrict__ Mh, __half2* __restrict__ Minvh, float* __restrict__ scale,
                                                                CoarseOpDev<float> op, int m0) {
  __shared__ float red[4];
  const int x = blockIdx.x, m = m0 + blockIdx.y, n = op.n, nt = op.nt, tiles = nt * nt, grouped = tiles & ~3;
  const float2* src = reinterpret_cast<const float2*>(m < 5 ? op.M + ((size_t)x * 5 + m) * op.msize * 2 : op.Minv + (size_t)x * op.msize * 2);
  __half2* dst = m < 5 ? Mh + ((size_t)x * 5 + m) * op.msize : Minvh + (size_t)x * op.msize;
  float amax = 0.f;
  for (int e = threadIdx.x; e < tiles * 64; e += 256) {
    const int t = e >> 6, l = e & 63, i = (t / nt) * 8 + (l >> 3), j = (t % nt) * 8 + (l & 7);
    if (i < n && j < n) { const float2 z = src[e]; amax = fmaxf(amax, fmaxf(fabsf(z.x), fabsf(z.y))); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  const float s = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  for (int e = threadIdx.x; e < tiles * 64; e += 256) {
    const int t = e >> 6, l = e & 63, i = (t / nt) * 8 + (l >> 3), j = (t % nt) * 8 + (l & 7);
    __half2 h = __floats2half2_rn(0.f, 0.f);
    if (i < n && j < n && s > 0.f) { const float2 z = src[e]; h = __floats2half2_rn(z.x / s, z.y / s); }
    dst[t < grouped ? (t >> 2) * 256 + l * 4 + (t & 3) : e] = h;
  }
  if (threadIdx.x == 0) scale[(size_t)x * 6 + m] = s;
}

// matrices m0 .. m0 + count - 1 of every site (0-4 the couplings, 5 the inverted self coupling) from `op` into Mh / Minvh in the
// layout of coarse_half.h, their scales to scale[site * 6 + m].  Minvh is read only for m = 5.
static void coarse_half_build(__half2* Mh, __half2* Minvh, float* scale, const CoarseOpDev<float>& op, int m0, int count, hipStream_t st) {
  hipLaunchKernelGGL(coarse_half_build_kernel, dim3(op.V, count), dim3(256), 0, st, Mh, Minvh, scale, op, m0);
  DDAMG_HIP_CHECK(hipGetLastError());
}

// with_inverse: the caller reads Minv as well; it is allocated and built by the first such call
CoarseHalfDev CoarseHalf::refresh(const CoarseOp<float>& op, hipStream_t st, bool with_inverse) {
  DDAMG_REQUIRE(!op.distributed(), "16-bit coupling storage: the level must live on one process");
  DDAMG_REQUIRE(op.nt() >= 1 && op.nt() <= 8, "16-bit coupling storage: at most 64 dof per site");
  const size_t V = (size_t)op.V();
  if (!M_) {
    M_.alloc(V * 5 * op.msize());
    scale_.alloc(V * 6);
    valid_ = false;
  }
  const bool new_inverse = with_inverse && !Minv_;
  if (new_inverse) Minv_.alloc(V * op.msize());
  const CoarseOpDev<float> d = op.dev();
  if (!valid_ || version_ != op.version()) {
    coarse_half_build(M_, Minv_, scale_, d, 0, 5, st);
    version_ = op.version();
  }
  if (with_inverse && (new_inverse || inverse_version_ != op.inverse_version())) {
    coarse_half_build(M_, Minv_, scale_, d, 5, 1, st);
    inverse_version_ = op.inverse_version();
  }
  valid_ = true;
  return CoarseHalfDev{M_, Minv_, scale_, d.nb, op.V(), op.n(), op.msize()};
}

void CoarseHalf::release() {
  M_.reset(); Minv_.reset(); scale_.reset();
  valid_ = false;
}

static void launch_half(const CoarseHalfDev& h, int nt, float* out, const float* in, int s0, int s1, int mode, double sign, bool acc, int swz, hipStream_t st) {
  if (s1 <= s0) return;
  DDAMG_REQUIRE(s0 >= 0 && s1 <= h.V, "16-bit coarse storage: site range outside the level");
  const dim3 grid(s1 - s0), block(mode == HALF_HOP ? 512 : 64);
  if ((s1 - s0) >= 64) swz |= 1;
#define DDAMG_LAUNCH(NTV, MODEV) hipLaunchKernelGGL((coarse_half_kernel<NTV, MODEV>), grid, block, 0, st, out, in, h, s0, (float)sign, acc ? 1 : 0, swz)
#define DDAMG_CASE(NTV) case NTV: \
    if (mode == HALF_HOP) DDAMG_LAUNCH(NTV, HALF_HOP); else if (mode == HALF_SELF) DDAMG_LAUNCH(NTV, HALF_SELF); else DDAMG_LAUNCH(NTV, HALF_SELFINV); \
    break;
  switch (nt) {
    DDAMG_CASE(1) DDAMG_CASE(2) DDAMG_CASE(3) DDAMG_CASE(4) DDAMG_CASE(5) DDAMG_CASE(6) DDAMG_CASE(7) DDAMG_CASE(8)
    default: DDAMG_REQUIRE(false, "coarse operator: more than 64 dof per site are not supported");
  }
#undef DDAMG_CASE
#undef DDAMG_LAUNCH
  DDAMG_HIP_CHECK(hipGetLastError());
}

void CoarseHalf::hop(const CoarseOp<float>& op, float* out, const float* in, int s0, int s1, double sign, bool accumulate, hipStream_t st) {
  DDAMG_REQUIRE(out != in, "coarse hopping term cannot run in place");
  const CoarseHalfDev h = refresh(op, st, true);
  launch_half(h, op.nt(), out, in, s0, s1, HALF_HOP, sign, accumulate, (hop_count_++ & 1u) ? 2 : 0, st);
}

void CoarseHalf::self_mul(const CoarseOp<float>& op, float* out, const float* in, int s0, int s1, bool inverse, hipStream_t st) {
  DDAMG_REQUIRE(out != in, "coarse self coupling cannot run in place");
  const CoarseHalfDev h = refresh(op, st, true);
  launch_half(h, op.nt(), out, in, s0, s1, inverse ? HALF_SELFINV : HALF_SELF, 1.0, false, 0, st);
}

}  // namespace ddamg
