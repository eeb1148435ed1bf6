// transfer_half.hip -- see transfer_half.h.  The two solve-path kernels are restrict_kernel<float, 1> and
// interpolate_kernel<float> (transfer.hip) on the 16-bit copy of P: one workgroup per aggregate, every site vector of P read as
// three non-temporal 16-byte loads per lane instead of six, converted in registers, accumulated in fp32.
#include "transfer_half.h"

namespace ddamg {

static constexpr int TILE = 8;  // interpolation vectors handled per register tile in the restriction

typedef _Float16 half8 __attribute__((ext_vector_type(8)));   // one 16-byte row of the copy

static inline int wg_threads(int agg_sites) {
  int t = 64;
  while (t < agg_sites && t < 256) t *= 2;
  return t;
}

// the rows of vector j on aggregate a: [row r of 3][site][8 halves]
__device__ __forceinline__ const half8* half_block(const __half* P, int a, int j, int nvec, int agg_sites) {
  return reinterpret_cast<const half8*>(P) + ((size_t)a * nvec + j) * 3 * agg_sites;
}
// the 24 reals of site i of a block, each still divided by the scale of its chirality
__device__ __forceinline__ void load_site_half(const half8* __restrict__ blk, int agg_sites, int i, float (&p)[24]) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const half8 w = __builtin_nontemporal_load(blk + (size_t)r * agg_sites + i);   // read-once stream, as the fp32 kernels read P
#pragma unroll
    for (int k = 0; k < 8; k++) p[8 * r + k] = (float)w[k];
  }
}

// ---- the copy: one workgroup per aggregate.  Wavefront w finds the two block maxima of the vectors w, w + 4, ...; then all
// threads convert, a work item being one 16-byte row of the copy (two chunk rows of the fp32 block)
__global__ __launch_bounds__(256) void transfer_half_build_kernel(__half* __restrict__ Ph, float* __restrict__ scale, const float* __restrict__ P,
                                                                  int nvec, int agg_sites, int aps) {
  extern __shared__ float sc[];   // [nvec][2]
  const int a = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = wv; j < nvec; j += 4) {
    const float* blk = P + ((size_t)a * nvec + j) * 24 * aps;
    float m[2] = {0.f, 0.f};
    for (int e = lane; e < 6 * agg_sites; e += 64) {
      const int kk = e / agg_sites, i = e - kk * agg_sites;
      const float4 v = *reinterpret_cast<const float4*>(blk + ((size_t)kk * aps + i) * 4);
      const float mv = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
      if (kk < 3) m[0] = fmaxf(m[0], mv); else m[1] = fmaxf(m[1], mv);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m[0] = fmaxf(m[0], __shfl_xor(m[0], o, 64)); m[1] = fmaxf(m[1], __shfl_xor(m[1], o, 64)); }
    if (lane < 2) {
      const float s = lane ? m[1] : m[0];
      sc[2 * j + lane] = s;
      scale[((size_t)a * nvec + j) * 2 + lane] = s;
    }
  }
  __syncthreads();
  half8* out = reinterpret_cast<half8*>(Ph) + (size_t)a * nvec * 3 * agg_sites;
  const int rows = 3 * agg_sites;
  for (int e = threadIdx.x; e < nvec * rows; e += 256) {
    const int j = e / rows, q = e - j * rows, r = q / agg_sites, i = q - r * agg_sites;
    const float* blk = P + ((size_t)a * nvec + j) * 24 * aps;
    const float4 lo = *reinterpret_cast<const float4*>(blk + ((size_t)(2 * r) * aps + i) * 4);
    const float4 hi = *reinterpret_cast<const float4*>(blk + ((size_t)(2 * r + 1) * aps + i) * 4);
    const float slo = sc[2 * j + (2 * r) / 3], shi = sc[2 * j + (2 * r + 1) / 3];   // chunk rows 0-2: chirality 0, 3-5: chirality 1
    half8 w;
    for (int k = 0; k < 8; k++) w[k] = (_Float16)0.f;      // s == 0: a block of zeros
    if (slo > 0.f) { w[0] = (_Float16)(lo.x / slo); w[1] = (_Float16)(lo.y / slo); w[2] = (_Float16)(lo.z / slo); w[3] = (_Float16)(lo.w / slo); }
    if (shi > 0.f) { w[4] = (_Float16)(hi.x / shi); w[5] = (_Float16)(hi.y / shi); w[6] = (_Float16)(hi.z / shi); w[7] = (_Float16)(hi.w / shi); }
    out[e] = w;
  }
}

// ---- restriction: phi_c[a][h*N + j] = s[a][j][h] * sum_{x in a, d in chirality h} conj(Ph_j(x,d)) phi(x,d) ------
__global__ __launch_bounds__(256) void restrict_half_kernel(float* __restrict__ phi_c, const float* __restrict__ phi, const __half* __restrict__ P,
                                                            const float* __restrict__ scale, int nvec, int V, int agg_sites, const int* __restrict__ agg_csite) {
  __shared__ double red[4 * TILE * 4];  // [value][wave]
  const int a = blockIdx.x, nt = blockDim.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = nt >> 6;
  const size_t s0 = (size_t)a * agg_sites;
  // at most one site per thread (aggregates of up to 256 sites): its spinor stays in registers across the tiles of vectors
  const bool one_site = agg_sites <= nt;
  float f[24];
#pragma unroll
  for (int k = 0; k < 24; k++) f[k] = 0.f;
  if (one_site && (int)threadIdx.x < agg_sites) load_site<float, 24>(phi, V, s0 + threadIdx.x, f);
  for (int j0 = 0; j0 < nvec; j0 += TILE) {
    const int jt = min(TILE, nvec - j0);
    float acc[TILE][4];
#pragma unroll
    for (int t = 0; t < TILE; t++) { acc[t][0] = acc[t][1] = acc[t][2] = acc[t][3] = 0.f; }
    for (int i = threadIdx.x; i < agg_sites; i += nt) {
      if (!one_site) load_site<float, 24>(phi, V, s0 + i, f);
#pragma unroll
      for (int t = 0; t < TILE; t++) {
        if (t < jt) {
          float p[24];
          load_site_half(half_block(P, a, j0 + t, nvec, agg_sites), agg_sites, i, p);
#pragma unroll
          for (int h = 0; h < 2; h++)
#pragma unroll
            for (int d = 0; d < 6; d++) {
              const int k = 2 * (6 * h + d);
              acc[t][2 * h]     += p[k] * f[k] + p[k + 1] * f[k + 1];      // Re conj(p) f
              acc[t][2 * h + 1] += p[k] * f[k + 1] - p[k + 1] * f[k];      // Im conj(p) f
            }
        }
      }
    }
    // the 32 sums of a wavefront by the transposing butterfly of restrict_kernel: lanes 2i and 2i+1 end up with the sum of value i
    double v[32];
#pragma unroll
    for (int t = 0; t < TILE; t++)
#pragma unroll
      for (int q = 0; q < 4; q++) v[t * 4 + q] = (double)acc[t][q];
#pragma unroll
    for (int o = 32, nn = 32; o >= 2; o >>= 1, nn >>= 1) {
      const bool up = (lane & o) != 0;
#pragma unroll
      for (int k = 0; k < nn / 2; k++) {
        const double send = up ? v[k] : v[k + nn / 2];
        const double keep = up ? v[k + nn / 2] : v[k];
        v[k] = keep + __shfl_xor(send, o, 64);
      }
    }
    v[0] += __shfl_xor(v[0], 1, 64);
    if (!(lane & 1)) red[(lane >> 1) * 4 + wv] = v[0];
    __syncthreads();
    for (int e = threadIdx.x; e < 4 * jt; e += nt) {
      const int q = e & 3, t = e >> 2;  // q: 0 re(h=0) 1 im(h=0) 2 re(h=1) 3 im(h=1)
      double sum = 0;
      for (int w = 0; w < nw; w++) sum += red[e * 4 + w];
      const int h = q >> 1, ri = q & 1;
      phi_c[((size_t)agg_csite[a] * 2 * nvec + (size_t)h * nvec + j0 + t) * 2 + ri] = scale[((size_t)a * nvec + j0 + t) * 2 + h] * (float)sum;
    }
    __syncthreads();
  }
}

// ---- interpolation: phi(x,d) (+)= sum_j Ph_j(x,d) (s[a][j][h(d)] phi_c[a][h(d)*N + j]) -------------------------------
__global__ __launch_bounds__(256) void interpolate_half_kernel(float* __restrict__ phi, const float* __restrict__ phi_c, const __half* __restrict__ P,
                                                               const float* __restrict__ scale, int nvec, int V, int agg_sites, int add,
                                                               const int* __restrict__ agg_csite) {
  extern __shared__ float pc[];  // [2*nvec][2], the scale of the block already in it
  const int a = blockIdx.x, nt = blockDim.x;
  const size_t s0 = (size_t)a * agg_sites;
  for (int k = threadIdx.x; k < 4 * nvec; k += nt) {
    const int hj = k >> 1, h = hj >= nvec ? 1 : 0, j = hj - h * nvec;
    pc[k] = scale[((size_t)a * nvec + j) * 2 + h] * phi_c[(size_t)agg_csite[a] * 4 * nvec + k];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < agg_sites; i += nt) {
    float f[24];
    if (add) load_site<float, 24>(phi, V, s0 + i, f);
    else {
#pragma unroll
      for (int k = 0; k < 24; k++) f[k] = 0.f;
    }
#pragma unroll 4      // four vectors of P in flight per thread (12 loads, as many as interpolate_kernel keeps in flight with two)
    for (int j = 0; j < nvec; j++) {
      float p[24];
      load_site_half(half_block(P, a, j, nvec, agg_sites), agg_sites, i, p);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const float cr = pc[2 * (h * nvec + j)], ci = pc[2 * (h * nvec + j) + 1];
#pragma unroll
        for (int d = 0; d < 6; d++) {
          const int k = 2 * (6 * h + d);
          f[k]     += cr * p[k] - ci * p[k + 1];
          f[k + 1] += cr * p[k + 1] + ci * p[k];
        }
      }
    }
    store_site<float, 24>(phi, V, s0 + i, f);
  }
}

void TransferHalf::refresh(const Interpolation<float>& ip, hipStream_t st) {
  DDAMG_REQUIRE(ip.P.get() != nullptr && ip.nvec >= 1 && ip.agg_sites >= 1, "16-bit transfer storage: no interpolation operator");
  if (src_ != &ip || !P_) {
    P_.alloc(ip.p_elems());
    scale_.alloc((size_t)ip.num_aggs * ip.nvec * 2);
    src_ = &ip; valid_ = false;
  }
  if (!valid_ || version_ != ip.version()) {
    hipLaunchKernelGGL(transfer_half_build_kernel, dim3(ip.num_aggs), dim3(256), sizeof(float) * 2 * ip.nvec, st, P_.get(), scale_.get(), ip.P.get(),
                       ip.nvec, ip.agg_sites, ip.plane_sites());
    DDAMG_HIP_CHECK(hipGetLastError());
    version_ = ip.version(); valid_ = true;
  }
}

void TransferHalf::release() {
  P_.reset(); scale_.reset();
  src_ = nullptr; valid_ = false;
}

void TransferHalf::restrict_to(const Interpolation<float>& ip, float* phi_c, const float* phi, hipStream_t st) {
  refresh(ip, st);
  hipLaunchKernelGGL(restrict_half_kernel, dim3(ip.num_aggs), dim3(wg_threads(ip.agg_sites)), 0, st, phi_c, phi, P_.get(), scale_.get(), ip.nvec, ip.V, ip.agg_sites,
                     ip.agg_csite.get());
  DDAMG_HIP_CHECK(hipGetLastError());
}

void TransferHalf::interpolate(const Interpolation<float>& ip, float* phi, const float* phi_c, bool add, hipStream_t st) {
  refresh(ip, st);
  hipLaunchKernelGGL(interpolate_half_kernel, dim3(ip.num_aggs), dim3(wg_threads(ip.agg_sites)), sizeof(float) * 4 * ip.nvec, st, phi, phi_c, P_.get(), scale_.get(),
                     ip.nvec, ip.V, ip.agg_sites, add ? 1 : 0, ip.agg_csite.get());
  DDAMG_HIP_CHECK(hipGetLastError());
}

}  // namespace ddamg
