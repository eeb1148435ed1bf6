// coarse_half_device.h -- device code shared by the kernels that read couplings in the 16-bit format of coarse_half.h
// (coarse_half.hip: the coarsest level; coarse_half_level.hip: the intermediate levels).
#pragma once
#include "coarse_half.h"

namespace ddamg {

struct alignas(16) Half2x4 { __half2 e[4]; };

// one wavefront: res[0..np) = s * Mh * v   (DAG=false)   or   s * G5 Mh^H G5 v   (DAG=true)
template <int NT, bool DAG>
__device__ __forceinline__ void wave_mv_half(const __half2* __restrict__ Mbase, float s, const float* __restrict__ v, int n, float* __restrict__ res) {
  const int l = threadIdx.x & 63, a = l >> 3, b = l & 7;
  const int half = n >> 1;
  float xr[NT], xi[NT];  // input entries this lane needs
#pragma unroll
  for (int t = 0; t < NT; t++) {
    // unconditional loads with a clamped index, the padding entries zeroed by a select (coarse_op.hip, wave_mv)
    const int k = (DAG ? a : b) + 8 * t, kc = k < n ? k : n - 1;
    const float2 z = *reinterpret_cast<const float2*>(v + 2 * kc);
    const float sg = k >= n ? 0.f : (DAG && k >= half) ? -1.f : 1.f;
    xr[t] = sg * z.x; xi[t] = sg * z.y;
  }
  float ar[NT], ai[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) { ar[t] = 0; ai[t] = 0; }
  const auto fma_tile = [&](int p, int q, const __half2 h) {
    const float2 m = __half22float2(h);
    if constexpr (!DAG) {  // y_i += M_ij v_j   (i <-> p, j <-> q)
      ar[p] += m.x * xr[q] - m.y * xi[q];
      ai[p] += m.x * xi[q] + m.y * xr[q];
    } else {               // z_j += conj(M_ij) w_i
      ar[q] += m.x * xr[p] + m.y * xi[p];
      ai[q] += m.x * xi[p] - m.y * xr[p];
    }
  };
  constexpr int TILES = NT * NT, GROUPS = TILES / 4;
  const Half2x4* M4 = reinterpret_cast<const Half2x4*>(Mbase) + l;
#pragma unroll
  for (int g = 0; g < GROUPS; g++) {
    const Half2x4 w = M4[g * 64];
#pragma unroll
    for (int u = 0; u < 4; u++) fma_tile((4 * g + u) / NT, (4 * g + u) % NT, w.e[u]);
  }
  if constexpr (TILES % 4 != 0) fma_tile(NT - 1, NT - 1, Mbase[(TILES - 1) * 64 + l]);   // nt odd: the one tile outside the groups
#pragma unroll
  for (int t = 0; t < NT; t++) {
    if constexpr (!DAG) {
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) { ar[t] += __shfl_xor(ar[t], o, 64); ai[t] += __shfl_xor(ai[t], o, 64); }
      if (b == 0) { res[2 * (a + 8 * t)] = s * ar[t]; res[2 * (a + 8 * t) + 1] = s * ai[t]; }
    } else {
#pragma unroll
      for (int o = 8; o < 64; o <<= 1) { ar[t] += __shfl_xor(ar[t], o, 64); ai[t] += __shfl_xor(ai[t], o, 64); }
      if (a == 0) {
        const int k = b + 8 * t;
        const float sg = (k >= half) ? -s : s;
        res[2 * k] = sg * ar[t]; res[2 * k + 1] = sg * ai[t];
      }
    }
  }
}

}  // namespace ddamg
