// blas_device.h -- what the streaming kernels of blas.hip and chrono.hip share on the device: the launch shape, the chunk
// addressing of a View, 16-byte loads and stores, and the block sum of the two-stage reductions.
#pragma once
#include "blas.h"

namespace ddamg {

static constexpr int BLK = 256;
static constexpr int MAX_GRID = 2048;  // 256 CUs x 8 blocks (guide: cap memory-bound grids, grid-stride the rest)

static inline int grid_for(size_t nchunks) {
  size_t g = (nchunks + BLK - 1) / BLK;
  if (g < 1) g = 1;
  if (g > (size_t)MAX_GRID) g = MAX_GRID;
  return (int)g;
}

// ---- chunk addressing --------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ size_t chunk_addr(const View& v, size_t c) {
  constexpr int CH = Chunk<T>::CH;
  if (v.rows == 1) return v.off + c * CH;
  const size_t cpr = v.len / CH;
  const size_t r = c / cpr;
  return v.off + r * v.stride + (c - r * cpr) * CH;
}
template <typename T> __device__ __forceinline__ typename Chunk<T>::vec ldv(const T* p) { return *reinterpret_cast<const typename Chunk<T>::vec*>(p); }
// read-once stream (Krylov basis vectors of the fine level): non-temporal, so that it does not displace reusable lines
template <typename T, bool NT> __device__ __forceinline__ typename Chunk<T>::vec ldv_stream(const T* p) {
  if constexpr (!NT) return ldv<T>(p);
  else {
    constexpr int CH = Chunk<T>::CH;
    typedef T vecn __attribute__((ext_vector_type(CH)));
    vecn w = __builtin_nontemporal_load(reinterpret_cast<const vecn*>(p));
    typename Chunk<T>::vec v;
    v.x = w[0]; v.y = w[1];
    if constexpr (CH == 4) { v.z = w[2]; v.w = w[3]; }
    return v;
  }
}
// vectors above this size cannot live in the caches anyway
static inline bool stream_sized(const View& v, size_t elem) { return v.total() * elem > ((size_t)32 << 20); }
template <typename T> __device__ __forceinline__ void stv(T* p, typename Chunk<T>::vec x) { *reinterpret_cast<typename Chunk<T>::vec*>(p) = x; }

// ---- reductions -----------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  return x;
}
// block sum of NV values per thread; result valid in thread 0
template <int NV>
__device__ __forceinline__ void block_sum(double (&val)[NV], double* lds /* [NV*4] */) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; k++) {
    double s = wave_sum(val[k]);
    if (lane == 0) lds[k * 4 + wv] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NV; k++) val[k] = lds[k * 4] + lds[k * 4 + 1] + lds[k * 4 + 2] + lds[k * 4 + 3];
  }
  __syncthreads();
}
// second stage: d_out[k] = sum_b rw.d_partial[b * nval + k] for k < nval, summed over the processes on a grid (blas.hip)
void sum_partials(ReduceWork& rw, int nblocks, int nval, double* d_out, hipStream_t st);

}  // namespace ddamg
