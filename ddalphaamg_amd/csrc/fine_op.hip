// fine_op.hip -- fine Wilson-Clover apply (LDS-tiled, one site per lane; the fp64 operator also on fp32 inputs) + layout converters.
// Reference: d_plus_clover_PRECISION src/dirac_generic.c:159-277 (six passes + 8 half-spinor
// scratch fields there; one fused pass here), trans/trans_back src/schwarz_generic.c:1807-1846.
#include "fine_op.h"
#include "dirac_device.h"
#include <vector>
#include <complex>
#include <cstring>

#ifndef DDAMG_NT_CLOVER
#define DDAMG_NT_CLOVER true
#endif
#ifndef DDAMG_NT_STORE
#define DDAMG_NT_STORE true
#endif
namespace ddamg {

// ---- LDS-tiled variant ------------------------------------------------------------------------
// One workgroup = one tile of 256 consecutive sites (= one 4^4 Schwarz block, or several smaller
// blocks).  The tile's spinors are staged in LDS once; every link is loaded exactly once by the
// thread that owns its site and used for both of its products: the forward term of the owner and
// the backward term of the +mu neighbour, which travels through LDS as a projected half spinor
// (the scatter form of the reference's phase 3, src/dirac_generic.c:196-217, but inside a tile).
// Only couplings that leave the tile touch global memory for neighbour data.
// neighbour of the thread's site in direction d (0..7): from the global table, or arithmetically when the tile is
// one Schwarz block (no 32 B/site index traffic: a 16 B/thread tile-independent table + 8 scalars per tile)
template <bool ARITH>
__device__ __forceinline__ int tile_neighbor(const int* __restrict__ nb, size_t V, size_t s, int d, int tile0, const uint4& q,
                                             const int* __restrict__ tile_nb, int ntiles_all) {
  if constexpr (!ARITH) {
    return nb[(size_t)d * V + s];
  } else {
    const unsigned w = (d >> 1) == 0 ? q.x : (d >> 1) == 1 ? q.y : (d >> 1) == 2 ? q.z : q.w;
    const unsigned e = (d & 1) ? (w >> 16) : (w & 0xffffu);
    const int li = (int)(e & 0x7fffu);
    if (!(e & 0x8000u)) return tile0 + li;
    const int tn = tile_nb[(size_t)d * ntiles_all + (tile0 >> 8)];   // wave-uniform
    return tn >= 0 ? tn * 256 + li : nb[(size_t)d * V + s];
  }
}
// the same with the tile's neighbour tile in direction d already in a scalar register (tn; dirac_apply_lds_kernel reads the eight
// tile_nb entries of its tile once at its top: no scalar load and no wait for it in front of a face load)
template <bool ARITH>
__device__ __forceinline__ int tile_neighbor(const int* __restrict__ nb, size_t V, size_t s, int d, int tile0, const uint4& q, int tn) {
  if constexpr (!ARITH) {
    return nb[(size_t)d * V + s];
  } else {
    const unsigned w = (d >> 1) == 0 ? q.x : (d >> 1) == 1 ? q.y : (d >> 1) == 2 ? q.z : q.w;
    const unsigned e = (d & 1) ? (w >> 16) : (w & 0xffffu);
    const int li = (int)(e & 0x7fffu);
    if (!(e & 0x8000u)) return tile0 + li;
    return tn >= 0 ? tn * 256 + li : nb[(size_t)d * V + s];
  }
}

// a site of an input vector of another precision (its own chunked layout), converted on the way in: the fp64 operator on the
// fp32 iterates the V-cycle hands to the outer solver (FineOp<double>::apply_f32in)
template <typename T, typename TIN, int NR>
__device__ __forceinline__ void load_site_as(const TIN* __restrict__ base, size_t V, size_t s, T (&out)[NR]) {
  if constexpr (sizeof(T) == sizeof(TIN)) load_site<T, NR>(reinterpret_cast<const T*>(base), V, s, out);
  else {
    TIN tmp[NR];
    load_site<TIN, NR>(base, V, s, tmp);
#pragma unroll
    for (int k = 0; k < NR; k++) out[k] = (T)tmp[k];
  }
}

// the dagger form (FineOp::apply_dagger): gamma5 = diag(-1, -1, +1, +1) in spin, so spin components 0 and 1 (reals 0-11 of the 24)
// change sign on everything read from phi and on eta in front of its store; the arithmetic in between is the one of D, and every
// intermediate is the one of gamma5, D, gamma5 in three passes (negation is exact), hence the same bits
template <bool DAG, typename T>
__device__ __forceinline__ void gamma5_sign(T (&v)[24]) {
  if constexpr (DAG) {
#pragma unroll
    for (int k = 0; k < 12; k++) v[k] = -v[k];
  }
}

// CCL is not used here: it gives each kernel its own instantiation (one tile_dir shared by the CCL and the non-CCL kernel is
// optimised once before it is inlined into both, and both then need 143 VGPRs instead of 120)
template <typename T, int MU, bool ARITH, LinkForm LF, bool HB2, typename TIN = T, bool CCL = false, bool DAG = false>
__device__ __forceinline__ void tile_dir(const TIN* __restrict__ phi, const FineOpDev<T>& op, size_t s, bool live, int tile0, const uint4& q,
                                         const int (&tn)[8], const T (&p)[24], T (&e)[24], T* __restrict__ sp, T* __restrict__ hb) {
  const size_t V = op.V;
  const int t = threadIdx.x;
  T U[18];
  if (live) load_link<T, MU, LF>(op, V, s, U);
  // (a) backward product for my +mu neighbour:  U_mu(s)^dagger (1+gamma_mu) phi(s)
  {
    T h[12], g[12];
    spin_project<T, MU, +1>(p, h);
    su3_mul_dag<T>(U, h, g);
#pragma unroll
    for (int c = 0; c < 12; c++) hb[c * 256 + t] = g[c];
  }
  // (b) forward term with my own link
  if (live) {
    const int j = tile_neighbor<ARITH>(op.nb, V, s, MU, tile0, q, tn[MU]);
    if (j >= 0) {
      T pn[24];
      if (j - tile0 >= 0 && j - tile0 < 256) {
#pragma unroll
        for (int c = 0; c < 24; c++) pn[c] = sp[c * 256 + (j - tile0)];
      } else {
        load_site_as<T, TIN, 24>(phi, V, j, pn);
        gamma5_sign<DAG>(pn);
      }
      hop_accumulate<T, MU, true>(U, pn, e);
    } else {
      halo_forward<T, MU>(op, -1 - j, U, e);
    }
  }
  __syncthreads();
  // (c) backward term: product computed by site s-mu (in LDS) or, across the tile face, from global memory
  if (live) {
    const int j = tile_neighbor<ARITH>(op.nb, V, s, 4 + MU, tile0, q, tn[4 + MU]);
    if (j < 0) {
      halo_backward<T, MU>(op, -1 - j, e);
    } else if (j - tile0 >= 0 && j - tile0 < 256) {
      T g[12];
#pragma unroll
      for (int c = 0; c < 12; c++) g[c] = hb[c * 256 + (j - tile0)];
      spin_reconstruct_sub<T, MU, +1>(g, e);
    } else {
      T pn[24], Un[18];
      load_site_as<T, TIN, 24>(phi, V, j, pn);
      gamma5_sign<DAG>(pn);
      load_link<T, MU, LF>(op, V, (size_t)j, Un);
      hop_accumulate<T, MU, false>(Un, pn, e);
    }
  }
  if constexpr (!HB2) __syncthreads();   // HB2: the caller alternates between two hb buffers, one barrier per direction
}

// The order in which dirac_apply_lds_kernel walks the directions (mu: 0 = T, 1 = Z, 2 = Y, 3 = X), shared by every instantiation:
// X, Y, T, Z.  The X and Y neighbour tiles run on the same XCD at about the same time and staged their spinors at their start, so
// these face reads come first, while the lines are still in the L2; a T face belongs to another XCD and misses whenever it is read,
// and a Z neighbour (64 tiles away in the XCD's sequence) ran too long ago.  The order of the sum of the eight hop terms follows
// the list, so results change by rounding with it (docs/design/04_kernels.md has what was measured for the other orders).
constexpr int kDirOrder[4] = {3, 2, 0, 1};

// CCL: the clover term from its 56-real form (FineOpDev::cloverc, fp32 only); DAG: eta = D^dagger phi = gamma5 D gamma5 phi (gamma5_sign)
template <typename T, bool ARITH, LinkForm LF = LinkForm::Full, typename TIN = T, bool CCL = false, bool DAG = false>
__global__ __launch_bounds__(256, (sizeof(T) == 4 ? 3 : 2)) void dirac_apply_lds_kernel(T* __restrict__ eta, const TIN* __restrict__ phi, FineOpDev<T> op, int ntiles,
                                                                  const int* __restrict__ tile_list) {
  // fp32: two buffers for the backward products, used in turn, so that one barrier per direction is enough (48 KB of LDS,
  // three workgroups per CU as before); fp64 keeps one buffer and two barriers (its tile already takes 72 KB)
  constexpr bool HB2 = sizeof(T) == 4;
  __shared__ T sp[24 * 256];
  __shared__ T hb[(HB2 ? 2 : 1) * 12 * 256];
  T* const hb1 = hb + (HB2 ? 12 * 256 : 0);
  // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs, so give XCD k the
  // k-th contiguous eighth of the tiles (neighbouring tiles then share one L2)
  int tile = blockIdx.x;
  if ((ntiles & 7) == 0) tile = (blockIdx.x & 7) * (ntiles >> 3) + (blockIdx.x >> 3);
  if (tile_list) tile = tile_list[tile];   // interior / boundary subsets of a decomposed lattice
  const size_t V = op.V;
  const int tile0 = tile * 256;
  const size_t s = (size_t)tile0 + threadIdx.x;
  const bool live = s < V;
  T p[24], e[24];
  uint4 q = make_uint4(0, 0, 0, 0);
  if constexpr (ARITH) q = reinterpret_cast<const uint4*>(op.tnb)[threadIdx.x];
  // the tile's eight neighbour tiles: the index is wave-uniform, so these are scalar loads, issued once here
  int tn[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if constexpr (ARITH) {
#pragma unroll
    for (int d = 0; d < 8; d++) tn[d] = op.tile_nb[(size_t)d * (V >> 8) + tile];
  }
  if (live) {
    load_site_as<T, TIN, 24>(phi, V, s, p);
    gamma5_sign<DAG>(p);
  } else {
#pragma unroll
    for (int k = 0; k < 24; k++) p[k] = 0;
  }
#pragma unroll
  for (int c = 0; c < 24; c++) sp[c * 256 + threadIdx.x] = p[c];
  if (live) {
    if constexpr (CCL) {
      T cl[28];
      load_site<T, 28, DDAMG_NT_CLOVER>(op.cloverc, V, s, cl);
      herm6c_mul<T>(cl, p, e);
      load_site<T, 28, DDAMG_NT_CLOVER>(op.cloverc + (size_t)28 * V, V, s, cl);
      herm6c_mul<T>(cl, p + 12, e + 12);
    } else {
      T cl[36];
      load_site<T, 36, DDAMG_NT_CLOVER>(op.clover, V, s, cl);
      herm6_mul<T>(cl, p, e);
      load_site<T, 36, DDAMG_NT_CLOVER>(op.clover + (size_t)36 * V, V, s, cl);
      herm6_mul<T>(cl, p + 12, e + 12);
    }
  }
  __syncthreads();
  // the two hb buffers alternate with the position in the list, whichever direction stands there
  tile_dir<T, kDirOrder[0], ARITH, LF, HB2, TIN, CCL, DAG>(phi, op, s, live, tile0, q, tn, p, e, sp, hb);
  tile_dir<T, kDirOrder[1], ARITH, LF, HB2, TIN, CCL, DAG>(phi, op, s, live, tile0, q, tn, p, e, sp, hb1);
  tile_dir<T, kDirOrder[2], ARITH, LF, HB2, TIN, CCL, DAG>(phi, op, s, live, tile0, q, tn, p, e, sp, hb);
  tile_dir<T, kDirOrder[3], ARITH, LF, HB2, TIN, CCL, DAG>(phi, op, s, live, tile0, q, tn, p, e, sp, hb1);
  if (live) {
    gamma5_sign<DAG>(e);
    store_site<T, 24, DDAMG_NT_STORE>(eta, V, s, e);
  }
}

// ---- hopping term onto one parity (global odd-even: GMRES smoother) -----------------------------------------------
// Same tiling as above with the two roles separated: a site of the input parity only produces the backward products of
// its links (for its +mu neighbours), a site of the output parity only consumes -- its own links for the forward terms,
// the products of its -mu neighbours for the backward ones.  Every link is read once; with the parity-split order of the
// sites inside a block whole wavefronts take one role.
template <typename T, int MU, bool ARITH>
__device__ __forceinline__ void tile_dir_parity(const T* __restrict__ phi, const FineOpDev<T>& op, size_t s, bool live, bool is_out, int tile0, const uint4& q,
                                                const T (&p)[24], T (&e)[24], T* __restrict__ sp, T* __restrict__ hb) {
  const size_t V = op.V;
  const int t = threadIdx.x;
  T U[18];
  if (live) load_site<T, 18>(op.D + (size_t)MU * 18 * V, V, s, U);
  if (live && !is_out) {
    T h[12], g[12];
    spin_project<T, MU, +1>(p, h);
    su3_mul_dag<T>(U, h, g);
#pragma unroll
    for (int c = 0; c < 12; c++) hb[c * 256 + t] = g[c];
  }
  if (live && is_out) {
    const int j = tile_neighbor<ARITH>(op.nb, V, s, MU, tile0, q, op.tile_nb, (int)(V >> 8));
    if (j >= 0) {
      T pn[24];
      if (j - tile0 >= 0 && j - tile0 < 256) {
#pragma unroll
        for (int c = 0; c < 24; c++) pn[c] = sp[c * 256 + (j - tile0)];
      } else {
        load_site<T, 24>(phi, V, j, pn);
      }
      hop_accumulate<T, MU, true>(U, pn, e);
    } else {
      halo_forward<T, MU>(op, -1 - j, U, e);
    }
  }
  __syncthreads();
  if (live && is_out) {
    const int j = tile_neighbor<ARITH>(op.nb, V, s, 4 + MU, tile0, q, op.tile_nb, (int)(V >> 8));
    if (j < 0) {
      halo_backward<T, MU>(op, -1 - j, e);
    } else if (j - tile0 >= 0 && j - tile0 < 256) {
      T g[12];
#pragma unroll
      for (int c = 0; c < 12; c++) g[c] = hb[c * 256 + (j - tile0)];
      spin_reconstruct_sub<T, MU, +1>(g, e);
    } else {
      T pn[24], Un[18];
      load_site<T, 24>(phi, V, j, pn);
      load_site<T, 18>(op.D + (size_t)MU * 18 * V, V, j, Un);
      hop_accumulate<T, MU, false>(Un, pn, e);
    }
  }
  __syncthreads();
}

template <typename T, bool ARITH>
__global__ __launch_bounds__(256, (sizeof(T) == 4 ? 3 : 2)) void dirac_hop_parity_kernel(T* __restrict__ eta, const T* __restrict__ phi, FineOpDev<T> op, int ntiles,
                                                                                         const int* __restrict__ tile_list, int par, int post,
                                                                                         const T* __restrict__ a) {
  __shared__ T sp[24 * 256];
  __shared__ T hb[12 * 256];
  int tile = blockIdx.x;
  if ((ntiles & 7) == 0) tile = (blockIdx.x & 7) * (ntiles >> 3) + (blockIdx.x >> 3);
  if (tile_list) tile = tile_list[tile];
  const size_t V = op.V;
  const int tile0 = tile * 256;
  const size_t s = (size_t)tile0 + threadIdx.x;
  const bool live = s < V;
  const bool is_out = live && op.parity[s] == par;
  T p[24], e[24];
  uint4 q = make_uint4(0, 0, 0, 0);
  if constexpr (ARITH) q = reinterpret_cast<const uint4*>(op.tnb)[threadIdx.x];
#pragma unroll
  for (int k = 0; k < 24; k++) { p[k] = 0; e[k] = 0; }
  if (live && !is_out) {
    load_site<T, 24>(phi, V, s, p);
#pragma unroll
    for (int c = 0; c < 24; c++) sp[c * 256 + threadIdx.x] = p[c];
  }
  __syncthreads();
  tile_dir_parity<T, 0, ARITH>(phi, op, s, live, is_out, tile0, q, p, e, sp, hb);
  tile_dir_parity<T, 1, ARITH>(phi, op, s, live, is_out, tile0, q, p, e, sp, hb);
  tile_dir_parity<T, 2, ARITH>(phi, op, s, live, is_out, tile0, q, p, e, sp, hb);
  tile_dir_parity<T, 3, ARITH>(phi, op, s, live, is_out, tile0, q, p, e, sp, hb);
  if (is_out) {   // the sites of the input parity are left alone
    if (post == 1) {          // D_ss^-1 (H in): the odd half of the Schur complement
      T f[24], cl[36];
      load_site<T, 36>(op.clover_inv, V, s, cl);
      herm6_mul<T>(cl, e, f);
      load_site<T, 36>(op.clover_inv + (size_t)36 * V, V, s, cl);
      herm6_mul<T>(cl, e + 12, f + 12);
      store_site<T, 24>(eta, V, s, f);
    } else if (post == 2) {   // D_ss a - H in: its even half
      T pa[24], f[24], cl[36];
      load_site<T, 24>(a, V, s, pa);
      load_site<T, 36>(op.clover, V, s, cl);
      herm6_mul<T>(cl, pa, f);
      load_site<T, 36>(op.clover + (size_t)36 * V, V, s, cl);
      herm6_mul<T>(cl, pa + 12, f + 12);
#pragma unroll
      for (int k = 0; k < 24; k++) f[k] -= e[k];
      store_site<T, 24>(eta, V, s, f);
    } else {
      store_site<T, 24>(eta, V, s, e);
    }
  }
}

template <typename T, bool CCL, bool DAG>
static void launch_dirac_apply(T* eta, const T* phi, const FineOpDev<T>& op, int ntiles, const int* tile_list, hipStream_t st) {
  if constexpr (sizeof(T) == 4) {
    if (op.tnb && op.Dp) {
      hipLaunchKernelGGL((dirac_apply_lds_kernel<T, true, LinkForm::Pivot, T, CCL, DAG>), dim3(ntiles), dim3(256), 0, st, eta, phi, op, ntiles, tile_list);
      return;
    }
  }
  if (op.tnb && op.Dc) hipLaunchKernelGGL((dirac_apply_lds_kernel<T, true, LinkForm::TwoRow, T, CCL, DAG>), dim3(ntiles), dim3(256), 0, st, eta, phi, op, ntiles, tile_list);
  else if (op.tnb) hipLaunchKernelGGL((dirac_apply_lds_kernel<T, true, LinkForm::Full, T, CCL, DAG>), dim3(ntiles), dim3(256), 0, st, eta, phi, op, ntiles, tile_list);
  else hipLaunchKernelGGL((dirac_apply_lds_kernel<T, false, LinkForm::Full, T, CCL, DAG>), dim3(ntiles), dim3(256), 0, st, eta, phi, op, ntiles, tile_list);
}

// apply() and apply_dagger(): the same launches, the kernels with and without the gamma5 signs
template <typename T>
template <bool DAG>
void FineOp<T>::apply_impl(T* eta, const T* phi, hipStream_t st) const {
  DDAMG_REQUIRE(D_ != nullptr, "fine operator not uploaded");
  auto launch = [&](int ntiles, const int* tile_list) {
    if (ntiles == 0) return;
    if (Cc_) launch_dirac_apply<T, sizeof(T) == 4, DAG>(eta, phi, dev(), ntiles, tile_list, st);
    else launch_dirac_apply<T, false, DAG>(eta, phi, dev(), ntiles, tile_list, st);
    DDAMG_HIP_CHECK(hipGetLastError());
  };
  if (!halo_.active()) {
    launch((V_ + 255) / 256, nullptr);
    return;
  }
  // reference order of events: src/dirac_generic.c:178-262 (project+send, interior work, wait, boundary): tiles without an
  // off-process neighbour during the exchange, the others after it
  halo_.pack(phi, D_, V_, st, DAG);
  halo_.exchange_begin(comm_, st);
  launch(halo_.n_interior(), halo_.interior_tiles());
  halo_.exchange_finish(comm_, st);
  launch(halo_.n_boundary(), halo_.boundary_tiles());
}
template <typename T>
void FineOp<T>::apply(T* eta, const T* phi, hipStream_t st) const { apply_impl<false>(eta, phi, st); }
// d_plus_clover_dagger_PRECISION (src/dirac_generic.c:281-285: gamma5, D, gamma5 in three passes) in one
template <typename T>
void FineOp<T>::apply_dagger(T* eta, const T* phi, hipStream_t st) const {
  DDAMG_REQUIRE(eta != phi, "apply_dagger: in place");
  apply_impl<true>(eta, phi, st);
}

// eta = D phi with phi an fp32 vector (its own layout): the fp64 operator of the outer solver on the iterates that come out of the
// fp32 V-cycle (fgmres_double + preconditioner(), src/linsolve_generic.c:219-413, src/preconditioner.c:25-69, where the iterate is
// converted first) -- the conversion happens in the loads, the result is the one of apply() on the converted vector bit for bit.
template <>
void FineOp<double>::apply_f32in(double* eta, const float* phi, hipStream_t st) const {
  DDAMG_REQUIRE(D_ != nullptr, "fine operator not uploaded");
  auto launch = [&](int ntiles, const int* tile_list) {
    if (ntiles == 0) return;
    if (tnb_ && Dc_) hipLaunchKernelGGL((dirac_apply_lds_kernel<double, true, LinkForm::TwoRow, float>), dim3(ntiles), dim3(256), 0, st, eta, phi, dev(), ntiles, tile_list);
    else if (tnb_) hipLaunchKernelGGL((dirac_apply_lds_kernel<double, true, LinkForm::Full, float>), dim3(ntiles), dim3(256), 0, st, eta, phi, dev(), ntiles, tile_list);
    else hipLaunchKernelGGL((dirac_apply_lds_kernel<double, false, LinkForm::Full, float>), dim3(ntiles), dim3(256), 0, st, eta, phi, dev(), ntiles, tile_list);
    DDAMG_HIP_CHECK(hipGetLastError());
  };
  if (!halo_.active()) { launch((V_ + 255) / 256, nullptr); return; }
  // on a process grid: the order of events of apply()
  halo_.pack_f32in(phi, D_, V_, st);
  halo_.exchange_begin(comm_, st);
  launch(halo_.n_interior(), halo_.interior_tiles());
  halo_.exchange_finish(comm_, st);
  launch(halo_.n_boundary(), halo_.boundary_tiles());
}

template <typename T>
void FineOp<T>::hop(T* eta, const T* phi, int par, hipStream_t st, int post, const T* a) const {
  DDAMG_REQUIRE(post == 0 || post == 1 || (post == 2 && a != nullptr && a != eta), "hop: unknown epilogue");
  DDAMG_REQUIRE(D_ != nullptr, "fine operator not uploaded");
  auto launch = [&](int ntiles, const int* tile_list) {
    if (ntiles == 0) return;
    if (tnb_) hipLaunchKernelGGL((dirac_hop_parity_kernel<T, true>), dim3(ntiles), dim3(256), 0, st, eta, phi, dev(), ntiles, tile_list, par, post, a);
    else hipLaunchKernelGGL((dirac_hop_parity_kernel<T, false>), dim3(ntiles), dim3(256), 0, st, eta, phi, dev(), ntiles, tile_list, par, post, a);
    DDAMG_HIP_CHECK(hipGetLastError());
  };
  if (!halo_.active()) { launch((V_ + 255) / 256, nullptr); return; }
  halo_.pack(phi, D_, V_, st);
  halo_.exchange_begin(comm_, st);
  launch(halo_.n_interior(), halo_.interior_tiles());
  halo_.exchange_finish(comm_, st);
  launch(halo_.n_boundary(), halo_.boundary_tiles());
}

template <typename T>
void FineOp<T>::halo_begin(const T* v, hipStream_t st) const {
  if (!halo_.active()) return;
  halo_.pack(v, D_, V_, st);
  halo_.exchange_begin(comm_, st);
}
template <typename T>
void FineOp<T>::halo_finish(hipStream_t st) const {
  if (halo_.active()) halo_.exchange_finish(comm_, st);
}
template <typename T>
void FineOp<T>::halo_exchange(const T* v, hipStream_t st) const {
  halo_begin(v, st);
  halo_finish(st);
}

// ---- operator data: reference storage (lexicographic fp64) -> device layouts, on the device -----------------------
// One thread per site: links into the chunked-SoA rows, both Hermitian 6x6 clover blocks into the packed form (real
// diagonal + strict upper triangle) and their inverses (Gauss-Jordan with partial pivoting in fp64, as the host code
// did before; the reference keeps Cholesky factors, src/oddeven_generic.c:24-150).  set_operator is on the path of every
// mass shift and clover scaling of the library interface (src/dirac.c:624-668), so it must not cost host seconds.
template <typename T>
__device__ __forceinline__ size_t soa_index_dev(int NR, size_t V, size_t s, int r) {
  constexpr int CH = Chunk<T>::CH;
  const int NF = NR / CH;
  if (r < NF * CH) return ((size_t)(r / CH) * V + s) * CH + (r % CH);
  const int TL = NR % CH;
  return (size_t)NF * V * CH + s * TL + (r - NF * CH);
}

// [A | 1] -> [1 | A^-1] for a complex 6x6 matrix, Gauss-Jordan with partial pivoting in fp64
__device__ __forceinline__ void gauss_jordan6(double (&mr)[6][12], double (&mi)[6][12]) {
  for (int col = 0; col < 6; col++) {
    int piv = col;
    double best = mr[col][col] * mr[col][col] + mi[col][col] * mi[col][col];
    for (int r = col + 1; r < 6; r++) {
      const double a2 = mr[r][col] * mr[r][col] + mi[r][col] * mi[r][col];
      if (a2 > best) { best = a2; piv = r; }
    }
    if (piv != col)
      for (int j = 0; j < 12; j++) {
        double t = mr[col][j]; mr[col][j] = mr[piv][j]; mr[piv][j] = t;
        t = mi[col][j]; mi[col][j] = mi[piv][j]; mi[piv][j] = t;
      }
    const double dr = mr[col][col] / best, di = -mi[col][col] / best;   // 1 / pivot
    for (int j = 0; j < 12; j++) {
      const double xr = mr[col][j], xi = mi[col][j];
      mr[col][j] = xr * dr - xi * di; mi[col][j] = xr * di + xi * dr;
    }
    for (int r = 0; r < 6; r++) {
      if (r == col) continue;
      const double fr = mr[r][col], fi = mi[r][col];
      if (fr == 0.0 && fi == 0.0) continue;
      for (int j = 0; j < 12; j++) {
        mr[r][j] -= fr * mr[col][j] - fi * mi[col][j];
        mi[r][j] -= fr * mi[col][j] + fi * mr[col][j];
      }
    }
  }
}

// In-place Gauss-Jordan inversion of a complex 6x6 matrix without pivoting, every index a compile-time constant: the matrix
// stays in registers (the pivoting form above indexes its rows dynamically and lives in scratch memory: 577 us per 65k
// sites against 60 us).  The clover blocks are Hermitian with the diagonal 4 + m0 +- O(csw) -- the reference factorises them
// by Cholesky without pivoting (src/oddeven_generic.c:24-60) --; returns false when a pivot is too small for that, and the
// caller then takes the pivoting form.
__device__ __forceinline__ bool invert6_in_place(double (&ar)[6][6], double (&ai)[6][6]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const double n2 = ar[k][k] * ar[k][k] + ai[k][k] * ai[k][k];
    ok = ok && n2 > 1e-24;
    const double pr = ar[k][k] / n2, pi = -ai[k][k] / n2;     // 1 / pivot
#pragma unroll
    for (int j = 0; j < 6; j++)
      if (j != k) { const double xr = ar[k][j], xi = ai[k][j]; ar[k][j] = xr * pr - xi * pi; ai[k][j] = xr * pi + xi * pr; }
#pragma unroll
    for (int i = 0; i < 6; i++)
      if (i != k) {
        const double fr = ar[i][k], fi = ai[i][k];
#pragma unroll
        for (int j = 0; j < 6; j++)
          if (j != k) { ar[i][j] -= fr * ar[k][j] - fi * ai[k][j]; ai[i][j] -= fr * ai[k][j] + fi * ar[k][j]; }
        ar[i][k] = -(fr * pr - fi * pi); ai[i][k] = -(fr * pi + fi * pr);
      }
    ar[k][k] = pr; ai[k][k] = pi;
  }
  return ok;
}
// inverse of the Hermitian 6x6 block given by its real diagonal d and strict upper triangle (ur, ui), row-major pairs
// (i < j): out_d the diagonal of the inverse, (our, oui) its strict upper triangle
__device__ __forceinline__ void invert_herm6(const double (&d)[6], const double (&ur)[15], const double (&ui)[15], double (&od)[6], double (&our)[15], double (&oui)[15]) {
  double ar[6][6], ai[6][6];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      ar[i][i] = d[i]; ai[i][i] = 0.0;
#pragma unroll
      for (int j = i + 1; j < 6; j++, k++) { ar[i][j] = ur[k]; ai[i][j] = ui[k]; ar[j][i] = ur[k]; ai[j][i] = -ui[k]; }
    }
  }
  if (!invert6_in_place(ar, ai)) {
    // cold path: partial pivoting (dynamic row indices, scratch memory)
    double mr[6][12], mi[6][12];
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 12; j++) { mr[i][j] = (j == 6 + i) ? 1.0 : 0.0; mi[i][j] = 0.0; }
    int k = 0;
    for (int i = 0; i < 6; i++) {
      mr[i][i] = d[i];
      for (int j = i + 1; j < 6; j++, k++) { mr[i][j] = ur[k]; mi[i][j] = ui[k]; mr[j][i] = ur[k]; mi[j][i] = -ui[k]; }
    }
    gauss_jordan6(mr, mi);
    k = 0;
    for (int i = 0; i < 6; i++) {
      od[i] = mr[i][6 + i];
      for (int j = i + 1; j < 6; j++, k++) { our[k] = mr[i][6 + j]; oui[k] = mi[i][6 + j]; }
    }
    return;
  }
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    od[i] = ar[i][i];
#pragma unroll
    for (int j = i + 1; j < 6; j++, k++) { our[k] = ar[i][j]; oui[k] = ai[i][j]; }
  }
}

// the 28-real form of one Hermitian 6x6 block (FineOpDev::cloverc), given as for invert_herm6, into reals r0..r0+27 of site s of
// the 56-real field; returns whether the block has the chiral structure A + Dd = c 1 to 1e-12 of its largest entry
template <typename T>
__device__ __forceinline__ bool compress_herm6(const double (&d)[6], const double (&ur)[15], const double (&ui)[15], T* __restrict__ out,
                                               size_t V, size_t s, int r0) {
  // index of the strict-upper entry (i, j) in ur / ui (row-major)
  auto up = [](int i, int j) { return 5 * i - i * (i - 1) / 2 + j - i - 1; };
  double mx = 0, dev = 0, c = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) mx = fmax(mx, fabs(d[i]));
#pragma unroll
  for (int k = 0; k < 15; k++) mx = fmax(mx, hypot(ur[k], ui[k]));
#pragma unroll
  for (int i = 0; i < 3; i++) {
    c += d[i] + d[3 + i];
    dev = fmax(dev, fabs(d[i] + d[3 + i] - (d[0] + d[3])));
#pragma unroll
    for (int j = i + 1; j < 3; j++) dev = fmax(dev, hypot(ur[up(i, j)] + ur[up(3 + i, 3 + j)], ui[up(i, j)] + ui[up(3 + i, 3 + j)]));
  }
  T v[28];
  v[0] = (T)(c / 6);
#pragma unroll
  for (int i = 0; i < 3; i++) v[1 + i] = (T)((d[i] - d[3 + i]) / 2);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = i + 1; j < 3; j++) { v[4 + 2 * (i + j - 1)] = (T)ur[up(i, j)]; v[5 + 2 * (i + j - 1)] = (T)ui[up(i, j)]; }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) { v[10 + 2 * (3 * i + j)] = (T)ur[up(i, 3 + j)]; v[11 + 2 * (3 * i + j)] = (T)ui[up(i, 3 + j)]; }
#pragma unroll
  for (int r = 0; r < 28; r++) out[soa_index_dev<T>(56, V, s, r0 + r)] = v[r];
  return dev <= 1e-12 * mx;   // false for NaN as well
}

template <typename T>
__global__ __launch_bounds__(128) void operator_layout_kernel(T* __restrict__ D, T* __restrict__ clover, T* __restrict__ clover_inv,
                                                              const double* __restrict__ D_lex, const double* __restrict__ clover_lex,
                                                              const int* __restrict__ lex_of_site, int V) {
  const size_t s = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (s >= (size_t)V) return;
  const size_t lx = lex_of_site[s];
  for (int mu = 0; mu < 4; mu++)
    for (int r = 0; r < 18; r++)
      D[(size_t)mu * 18 * V + soa_index_dev<T>(18, V, s, r)] = (T)D_lex[(lx * 36 + mu * 9) * 2 + r];
  const double* c = clover_lex + lx * 42 * 2;
#pragma unroll
  for (int b = 0; b < 2; b++) {
    double d[6], ur[15], ui[15], od[6], our[15], oui[15];
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = c[2 * (6 * b + i)];
#pragma unroll
    for (int k = 0; k < 15; k++) { ur[k] = c[2 * (12 + 15 * b + k)]; ui[k] = c[2 * (12 + 15 * b + k) + 1]; }
    invert_herm6(d, ur, ui, od, our, oui);
    const int r0 = 36 * b;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      clover[soa_index_dev<T>(72, V, s, r0 + i)] = (T)d[i];
      clover_inv[soa_index_dev<T>(72, V, s, r0 + i)] = (T)od[i];
    }
#pragma unroll
    for (int k = 0; k < 15; k++) {
      clover[soa_index_dev<T>(72, V, s, r0 + 6 + 2 * k)] = (T)ur[k];
      clover[soa_index_dev<T>(72, V, s, r0 + 6 + 2 * k + 1)] = (T)ui[k];
      clover_inv[soa_index_dev<T>(72, V, s, r0 + 6 + 2 * k)] = (T)our[k];
      clover_inv[soa_index_dev<T>(72, V, s, r0 + 6 + 2 * k + 1)] = (T)oui[k];
    }
  }
}

// mass shift: new diagonal = fp64 diagonal + diff, inverses of both 6x6 blocks rebuilt in fp64 (FineOp::shift_diagonal)
template <typename T>
__global__ __launch_bounds__(128) void clover_shift_kernel(T* clover, T* __restrict__ clover_inv, T* __restrict__ cloverc, const double* clover64, double diff,
                                                           int V) {
  const size_t s = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (s >= (size_t)V) return;
#pragma unroll
  for (int b = 0; b < 2; b++) {
    double d[6], ur[15], ui[15], od[6], our[15], oui[15];
    const int r0 = 36 * b;
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = clover64[soa_index_dev<double>(72, V, s, r0 + i)] + diff;
#pragma unroll
    for (int k = 0; k < 15; k++) {
      ur[k] = clover64[soa_index_dev<double>(72, V, s, r0 + 6 + 2 * k)];
      ui[k] = clover64[soa_index_dev<double>(72, V, s, r0 + 6 + 2 * k + 1)];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) clover[soa_index_dev<T>(72, V, s, r0 + i)] = (T)d[i];
    if (cloverc) (void)compress_herm6<T>(d, ur, ui, cloverc, V, s, 28 * b);   // the shift keeps the structure
    invert_herm6(d, ur, ui, od, our, oui);
#pragma unroll
    for (int i = 0; i < 6; i++) clover_inv[soa_index_dev<T>(72, V, s, r0 + i)] = (T)od[i];
#pragma unroll
    for (int k = 0; k < 15; k++) {
      clover_inv[soa_index_dev<T>(72, V, s, r0 + 6 + 2 * k)] = (T)our[k];
      clover_inv[soa_index_dev<T>(72, V, s, r0 + 6 + 2 * k + 1)] = (T)oui[k];
    }
  }
}
template <typename T>
void FineOp<T>::shift_diagonal(const double* clover64, double diff, hipStream_t st) {
  DDAMG_REQUIRE(clover_ != nullptr && clover64 != nullptr, "shift_diagonal: no operator uploaded");
  hipLaunchKernelGGL(clover_shift_kernel<T>, dim3((unsigned)((V_ + 127) / 128)), dim3(128), 0, st, clover_, clover_inv_, Cc_, clover64, diff, (int)V_);
  DDAMG_HIP_CHECK(hipGetLastError());
}

// scale_clover (src/dirac.c:624-644): the clover term of every site times scale_even or scale_odd by the global parity of the
// site, from an unscaled fp64 copy `base64` (so that scaling by (1, 1) restores the field bit for bit); the inverses of both 6x6
// blocks rebuilt in fp64 from the scaled blocks
template <typename T>
__global__ __launch_bounds__(128) void clover_scale_kernel(T* clover, T* __restrict__ clover_inv, T* __restrict__ cloverc, const double* base64,
                                                           const unsigned char* __restrict__ parity, double scale_even, double scale_odd, int V) {
  const size_t s = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (s >= (size_t)V) return;
  const double f = parity[s] ? scale_odd : scale_even;
#pragma unroll
  for (int b = 0; b < 2; b++) {
    double d[6], ur[15], ui[15], od[6], our[15], oui[15];
    const int r0 = 36 * b;
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = f * base64[soa_index_dev<double>(72, V, s, r0 + i)];
#pragma unroll
    for (int k = 0; k < 15; k++) {
      ur[k] = f * base64[soa_index_dev<double>(72, V, s, r0 + 6 + 2 * k)];
      ui[k] = f * base64[soa_index_dev<double>(72, V, s, r0 + 6 + 2 * k + 1)];
    }
    if (cloverc) (void)compress_herm6<T>(d, ur, ui, cloverc, V, s, 28 * b);   // so does the scaling
    invert_herm6(d, ur, ui, od, our, oui);
#pragma unroll
    for (int i = 0; i < 6; i++) {
      clover[soa_index_dev<T>(72, V, s, r0 + i)] = (T)d[i];
      clover_inv[soa_index_dev<T>(72, V, s, r0 + i)] = (T)od[i];
    }
#pragma unroll
    for (int k = 0; k < 15; k++) {
      clover[soa_index_dev<T>(72, V, s, r0 + 6 + 2 * k)] = (T)ur[k];
      clover[soa_index_dev<T>(72, V, s, r0 + 6 + 2 * k + 1)] = (T)ui[k];
      clover_inv[soa_index_dev<T>(72, V, s, r0 + 6 + 2 * k)] = (T)our[k];
      clover_inv[soa_index_dev<T>(72, V, s, r0 + 6 + 2 * k + 1)] = (T)oui[k];
    }
  }
}
template <typename T>
void FineOp<T>::scale_clover(const double* base64, double scale_even, double scale_odd, hipStream_t st) {
  DDAMG_REQUIRE(clover_ != nullptr && base64 != nullptr && parity_ != nullptr, "scale_clover: no operator uploaded");
  DDAMG_REQUIRE((const void*)base64 != (const void*)clover_, "scale_clover: the unscaled copy must be a buffer of its own");
  hipLaunchKernelGGL(clover_scale_kernel<T>, dim3((unsigned)((V_ + 127) / 128)), dim3(128), 0, st, clover_, clover_inv_, Cc_, base64, parity_, scale_even, scale_odd, (int)V_);
  DDAMG_HIP_CHECK(hipGetLastError());
}

// two-row link storage from the reference's links (lexicographic fp64, U/2): rows 0 and 1 in fp32, the sign with which
// 2 conj(row0 x row1) gives row 2, and -- in *bad -- whether any link is not of that form (then the full storage is used).
// With Dp: the pivot form as well (fine_op.h): row 0, the two entries of row 1 outside the pivot column p, and the byte sgn * (1 + p)
template <typename T>
__global__ __launch_bounds__(128) void link_compress_kernel(T* __restrict__ Dc, signed char* __restrict__ sgn, int* __restrict__ bad,
                                                            const double* __restrict__ D_lex, const int* __restrict__ lex_of_site, int V,
                                                            T* __restrict__ Dp, signed char* __restrict__ pb) {
  const size_t s = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (s >= (size_t)V) return;
  const size_t lx = lex_of_site[s];
  for (int mu = 0; mu < 4; mu++) {
    const double* u = D_lex + (lx * 36 + mu * 9) * 2;
    double dev_p = 0, dev_m = 0, nrm = 0;
    for (int k = 0; k < 3; k++) {
      const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
      const double cr = u[2 * k1] * u[6 + 2 * k2] - u[2 * k1 + 1] * u[6 + 2 * k2 + 1] - (u[2 * k2] * u[6 + 2 * k1] - u[2 * k2 + 1] * u[6 + 2 * k1 + 1]);
      const double ci = u[2 * k1] * u[6 + 2 * k2 + 1] + u[2 * k1 + 1] * u[6 + 2 * k2] - (u[2 * k2] * u[6 + 2 * k1 + 1] + u[2 * k2 + 1] * u[6 + 2 * k1]);
      const double er = 2 * cr, ei = -2 * ci;      // 2 conj(row0 x row1)
      dev_p += (u[12 + 2 * k] - er) * (u[12 + 2 * k] - er) + (u[12 + 2 * k + 1] - ei) * (u[12 + 2 * k + 1] - ei);
      dev_m += (u[12 + 2 * k] + er) * (u[12 + 2 * k] + er) + (u[12 + 2 * k + 1] + ei) * (u[12 + 2 * k + 1] + ei);
      nrm += u[12 + 2 * k] * u[12 + 2 * k] + u[12 + 2 * k + 1] * u[12 + 2 * k + 1];
    }
    const bool plus = dev_p <= dev_m;
    // accepted deviation of the stored third row from the rebuilt one, relative and squared: the fp32 operator rounds at 6e-8
    // anyway (1e-12 relative is far below it); the fp64 operator defines the outer solver's residual, so there only fields that
    // are unitary to fp64 rounding (1e-14) are replaced by their reconstruction -- anything else keeps the caller's third row
    const double accept = sizeof(T) == 4 ? 1e-24 : 1e-28;
    if ((plus ? dev_p : dev_m) > accept * (nrm > 0 ? nrm : 1.0) || nrm == 0) atomicOr(bad, 1);
    sgn[(size_t)mu * V + s] = plus ? 1 : -1;
    for (int r = 0; r < 12; r++) Dc[(size_t)mu * 12 * V + soa_index_dev<T>(12, V, s, r)] = (T)u[r];
    if (Dp) {
      // p: the smallest column that maximises |row0[k]|^2 of the rounded row 0 (the squares and their sum in fp64: the products
      // of two rounded entries are exact there, so no contraction of the compiler's can move the choice)
      int p = 0;
      double best = -1.0;
      for (int k = 0; k < 3; k++) {
        const double re = (double)(T)u[2 * k], im = (double)(T)u[2 * k + 1];
        const double n2 = re * re + im * im;
        if (n2 > best) { best = n2; p = k; }
      }
      T* const out = Dp + (size_t)mu * 10 * V;
      for (int r = 0; r < 6; r++) out[soa_index_dev<T>(10, V, s, r)] = (T)u[r];
      const int ka = p == 0 ? 1 : 0, kb = p == 2 ? 1 : 2;
      out[soa_index_dev<T>(10, V, s, 6)] = (T)u[6 + 2 * ka]; out[soa_index_dev<T>(10, V, s, 7)] = (T)u[6 + 2 * ka + 1];
      out[soa_index_dev<T>(10, V, s, 8)] = (T)u[6 + 2 * kb]; out[soa_index_dev<T>(10, V, s, 9)] = (T)u[6 + 2 * kb + 1];
      pb[(size_t)mu * V + s] = (signed char)((plus ? 1 : -1) * (1 + p));
    }
  }
}

// 56-real clover from the reference's clover (lexicographic fp64), and -- in *bad -- whether any block lacks the chiral structure
// (then the fp32 operator keeps reading the 72-real form)
template <typename T>
__global__ __launch_bounds__(128) void clover_compress_kernel(T* __restrict__ cloverc, int* __restrict__ bad, const double* __restrict__ clover_lex,
                                                              const int* __restrict__ lex_of_site, int V) {
  const size_t s = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (s >= (size_t)V) return;
  const double* c = clover_lex + (size_t)lex_of_site[s] * 42 * 2;
  bool ok = true;
#pragma unroll
  for (int b = 0; b < 2; b++) {
    double d[6], ur[15], ui[15];
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = c[2 * (6 * b + i)];
#pragma unroll
    for (int k = 0; k < 15; k++) { ur[k] = c[2 * (12 + 15 * b + k)]; ui[k] = c[2 * (12 + 15 * b + k) + 1]; }
    ok = compress_herm6<T>(d, ur, ui, cloverc, V, s, 28 * b) && ok;
  }
  if (!ok) atomicOr(bad, 1);
}

template <typename T>
void FineOp<T>::ensure_storage(const Geometry& g, hipStream_t st) {
  const size_t V = g.V;
  V_ = g.V;
  if (!D_) {
    D_.alloc(72 * V);
    clover_.alloc(72 * V);
    clover_inv_.alloc(72 * V);
    nb_.alloc(8 * V);
    lex_.alloc(V);
    DDAMG_HIP_CHECK(hipMemcpyAsync(lex_, g.lex_of_site.data(), sizeof(int) * V, hipMemcpyHostToDevice, st));
    std::vector<unsigned char> par(V);
    for (size_t i = 0; i < V; i++) par[i] = (unsigned char)g.parity[i];
    parity_.upload(par);
  }
}

template <typename T>
void FineOp<T>::upload(const Geometry& g, const double* D_ref, const double* clover_ref, const Knobs& knobs, hipStream_t st) {
  const size_t V = g.V;
  ensure_storage(g, st);
  DeviceBuffer<double> dD, dC;   // staging of the lexicographic fp64 arrays
  dD.alloc(72 * V);
  dC.alloc(84 * V);
  DDAMG_HIP_CHECK(hipMemcpyAsync(dD, D_ref, sizeof(double) * 72 * V, hipMemcpyHostToDevice, st));
  DDAMG_HIP_CHECK(hipMemcpyAsync(dC, clover_ref, sizeof(double) * 84 * V, hipMemcpyHostToDevice, st));
  layout_staged(g, dD, dC, knobs, st);
  dD.reset(); dC.reset();   // before the halo buffers are allocated
  init_halo(g);
}

template <typename T>
void FineOp<T>::upload_staged(const Geometry& g, const double* dD, const double* dC, const Knobs& knobs, hipStream_t st) {
  ensure_storage(g, st);
  layout_staged(g, dD, dC, knobs, st);
}

template <typename T>
void FineOp<T>::init_halo(const Geometry& g) {
  if (g.distributed() && !halo_.active()) halo_.init(g);
}

template <typename T>
void FineOp<T>::layout_staged(const Geometry& g, const double* dD, const double* dC, const Knobs& knobs, hipStream_t st) {
  const size_t V = g.V;
  hipLaunchKernelGGL(operator_layout_kernel<T>, dim3((unsigned)((V + 127) / 128)), dim3(128), 0, st, D_, clover_, clover_inv_, dD, dC, lex_, (int)V);
  DDAMG_HIP_CHECK(hipGetLastError());
  // two-row links (a third less link traffic in dirac_apply_lds_kernel and the Schwarz block solver) when every link allows it
  // fp32: the pivot form next to them (a sixth less again, dirac_apply_lds_kernel only) when a tile is one 4^4 block
  Dc_ = nullptr;
  Dp_ = nullptr;
  {
    if (knobs.link_compression && g.block_sites == 256) {
      if (!Dc_store_) {
        Dc_store_.alloc(48 * V);
        Dsgn_.alloc(4 * V, sizeof(int));
      }
      const bool pivot = sizeof(T) == 4 && knobs.link_pivot && g.B[0] == 4 && g.B[1] == 4 && g.B[2] == 4 && g.B[3] == 4;
      if (pivot && !Dp_store_) {
        Dp_store_.alloc(40 * V);
        Dpb_.alloc(4 * V);
      }
      int* d_bad = reinterpret_cast<int*>(Dsgn_ + 4 * V);   // one flag behind the signs
      DDAMG_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), st));
      hipLaunchKernelGGL(link_compress_kernel<T>, dim3((unsigned)((V + 127) / 128)), dim3(128), 0, st, Dc_store_, Dsgn_, d_bad, dD, lex_, (int)V,
                         pivot ? Dp_store_.get() : nullptr, pivot ? Dpb_.get() : nullptr);
      DDAMG_HIP_CHECK(hipGetLastError());
      int bad = 1;
      DDAMG_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
      DDAMG_HIP_CHECK(hipStreamSynchronize(st));
      if (!bad) Dc_ = Dc_store_;
      if (!bad && pivot) Dp_ = Dp_store_;
    }
  }
  // 56-real clover for the fp32 apply (dirac_apply_lds_kernel; a fifth less clover traffic) when every block allows it
  Cc_ = nullptr;
  if constexpr (sizeof(T) == 4) {
    if (knobs.clover_compression) {
      if (!Cc_store_) Cc_store_.alloc(56 * V, sizeof(int));
      int* d_bad = reinterpret_cast<int*>(Cc_store_ + 56 * V);   // one flag behind the field
      DDAMG_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), st));
      hipLaunchKernelGGL(clover_compress_kernel<T>, dim3((unsigned)((V + 127) / 128)), dim3(128), 0, st, Cc_store_, d_bad, dC, lex_, (int)V);
      DDAMG_HIP_CHECK(hipGetLastError());
      int bad = 1;
      DDAMG_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
      DDAMG_HIP_CHECK(hipStreamSynchronize(st));
      if (!bad) Cc_ = Cc_store_;
    }
  }
  DDAMG_HIP_CHECK(hipMemcpyAsync(nb_, g.nb.data(), sizeof(int) * 8 * V, hipMemcpyHostToDevice, st));
  if (g.block_sites == 256 && !tnb_) {   // one tile of the LDS kernel == one Schwarz block: arithmetic neighbours
    tile_nb_.alloc(8 * g.num_blocks);
    tnb_.alloc(8 * 256);
    DDAMG_HIP_CHECK(hipMemcpyAsync(tile_nb_, g.block_nb.data(), sizeof(int) * 8 * g.num_blocks, hipMemcpyHostToDevice, st));
    DDAMG_HIP_CHECK(hipMemcpyAsync(tnb_, g.blk_wrap_nb.data(), sizeof(unsigned short) * 8 * 256, hipMemcpyHostToDevice, st));
  }
  DDAMG_HIP_CHECK(hipStreamSynchronize(st));
}

// the fp64 operator back into the reference's storage: the exact inverse of operator_layout_kernel<double> (a permutation; the
// imaginary parts of the clover diagonal, which the device does not keep, are zero)
__global__ __launch_bounds__(128) void operator_export_kernel(double* __restrict__ D_lex, double* __restrict__ clover_lex, const double* __restrict__ D,
                                                              const double* __restrict__ clover, const int* __restrict__ lex_of_site, int V) {
  const size_t s = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (s >= (size_t)V) return;
  const size_t lx = lex_of_site[s];
  for (int mu = 0; mu < 4; mu++)
    for (int r = 0; r < 18; r++)
      D_lex[(lx * 36 + mu * 9) * 2 + r] = D[(size_t)mu * 18 * V + soa_index_dev<double>(18, V, s, r)];
  double* c = clover_lex + lx * 42 * 2;
  for (int b = 0; b < 2; b++) {
    const int r0 = 36 * b;
    for (int i = 0; i < 6; i++) { c[2 * (6 * b + i)] = clover[soa_index_dev<double>(72, V, s, r0 + i)]; c[2 * (6 * b + i) + 1] = 0.0; }
    for (int k = 0; k < 15; k++) {
      c[2 * (12 + 15 * b + k)] = clover[soa_index_dev<double>(72, V, s, r0 + 6 + 2 * k)];
      c[2 * (12 + 15 * b + k) + 1] = clover[soa_index_dev<double>(72, V, s, r0 + 6 + 2 * k + 1)];
    }
  }
}
template <>
void FineOp<double>::export_lex(double* dD_lex, double* dC_lex, const double* clover64, hipStream_t st) const {
  DDAMG_REQUIRE(D_ != nullptr, "fine operator not uploaded");
  hipLaunchKernelGGL(operator_export_kernel, dim3((unsigned)((V_ + 127) / 128)), dim3(128), 0, st, dD_lex, dC_lex, D_, clover64 ? clover64 : clover_.get(), lex_, (int)V_);
  DDAMG_HIP_CHECK(hipGetLastError());
}

// ---- global odd-even pieces ------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void oo_inv_kernel(T* __restrict__ out, const T* __restrict__ in, const T* __restrict__ clover_inv,
                                                     const unsigned char* __restrict__ parity, int V) {
  const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= (size_t)V) return;
  T e[24];
  if (parity[s]) {
    T p[24], cl[36];
    load_site<T, 24>(in, V, s, p);
    load_site<T, 36>(clover_inv, V, s, cl);
    herm6_mul<T>(cl, p, e);
    load_site<T, 36>(clover_inv + (size_t)36 * V, V, s, cl);
    herm6_mul<T>(cl, p + 12, e + 12);
  } else {
#pragma unroll
    for (int k = 0; k < 24; k++) e[k] = 0;
  }
  store_site<T, 24>(out, V, s, e);
}
template <typename T>
__global__ __launch_bounds__(256) void parity_select_kernel(T* __restrict__ out, const T* __restrict__ a, const T* __restrict__ b,
                                                            const unsigned char* __restrict__ parity, int keep, int V) {
  const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= (size_t)V) return;
  T e[24];
  if (parity[s] == keep) {
    load_site<T, 24>(a, V, s, e);
    if (b) {
      T f[24];
      load_site<T, 24>(b, V, s, f);
#pragma unroll
      for (int k = 0; k < 24; k++) e[k] -= f[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 24; k++) e[k] = 0;
  }
  store_site<T, 24>(out, V, s, e);
}
template <typename T>
void FineOp<T>::oo_inv(T* out, const T* in, hipStream_t st) const {
  hipLaunchKernelGGL(oo_inv_kernel<T>, dim3((unsigned)((V_ + 255) / 256)), dim3(256), 0, st, out, in, clover_inv_, parity_, (int)V_);
  DDAMG_HIP_CHECK(hipGetLastError());
}
template <typename T>
void FineOp<T>::parity_select(T* out, const T* a, const T* b, int keep, hipStream_t st) const {
  hipLaunchKernelGGL(parity_select_kernel<T>, dim3((unsigned)((V_ + 255) / 256)), dim3(256), 0, st, out, a, b, parity_, keep, (int)V_);
  DDAMG_HIP_CHECK(hipGetLastError());
}

// ---- layout converters ---------------------------------------------------------------------
// G5: the vector times gamma5 on the way (the reals of spin components 0 and 1, the first half of a site's, change sign)
template <typename T, bool G5>
__global__ void vec_from_lex_kernel(T* __restrict__ dst, const double* __restrict__ src, const int* __restrict__ lex_of_site, int V, int nreal) {
  // one thread per (site, real): coalesced on the SoA side
  constexpr int CH = Chunk<T>::CH;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)V * nreal;
  if (i >= total) return;
  // SoA linear index i -> (chunk k, site s, lane-in-chunk c)
  size_t k = i / ((size_t)V * CH);
  size_t rem = i - k * (size_t)V * CH;
  size_t s = rem / CH;
  int c = rem % CH;
  int r = (int)k * CH + c;
  const T x = (T)src[(size_t)lex_of_site[s] * nreal + r];
  dst[i] = G5 && 2 * r < nreal ? -x : x;
}
template <typename T, bool G5>
__global__ void vec_to_lex_kernel(double* __restrict__ dst, const T* __restrict__ src, const int* __restrict__ lex_of_site, int V, int nreal) {
  constexpr int CH = Chunk<T>::CH;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)V * nreal;
  if (i >= total) return;
  size_t k = i / ((size_t)V * CH);
  size_t rem = i - k * (size_t)V * CH;
  size_t s = rem / CH;
  int c = rem % CH;
  int r = (int)k * CH + c;
  const double x = (double)src[i];
  dst[(size_t)lex_of_site[s] * nreal + r] = G5 && 2 * r < nreal ? -x : x;
}

template <typename T>
void vec_from_lex(T* dst, const double* src, const int* lex_of_site, int V, int ndof, hipStream_t st, bool gamma5) {
  int nreal = 2 * ndof;
  DDAMG_REQUIRE(nreal % Chunk<T>::CH == 0, "dof per site must fill whole 16-byte chunks");
  size_t total = (size_t)V * nreal;
  DDAMG_REQUIRE(!gamma5 || ndof == 12, "gamma5 acts on fine vectors");
  if (gamma5) hipLaunchKernelGGL((vec_from_lex_kernel<T, true>), dim3((total + 255) / 256), dim3(256), 0, st, dst, src, lex_of_site, V, nreal);
  else hipLaunchKernelGGL((vec_from_lex_kernel<T, false>), dim3((total + 255) / 256), dim3(256), 0, st, dst, src, lex_of_site, V, nreal);
  DDAMG_HIP_CHECK(hipGetLastError());
}
template <typename T>
void vec_to_lex(double* dst, const T* src, const int* lex_of_site, int V, int ndof, hipStream_t st, bool gamma5) {
  int nreal = 2 * ndof;
  DDAMG_REQUIRE(nreal % Chunk<T>::CH == 0, "dof per site must fill whole 16-byte chunks");
  size_t total = (size_t)V * nreal;
  DDAMG_REQUIRE(!gamma5 || ndof == 12, "gamma5 acts on fine vectors");
  if (gamma5) hipLaunchKernelGGL((vec_to_lex_kernel<T, true>), dim3((total + 255) / 256), dim3(256), 0, st, dst, src, lex_of_site, V, nreal);
  else hipLaunchKernelGGL((vec_to_lex_kernel<T, false>), dim3((total + 255) / 256), dim3(256), 0, st, dst, src, lex_of_site, V, nreal);
  DDAMG_HIP_CHECK(hipGetLastError());
}

template <typename T, bool TO_LEX>
__global__ void aos_lex_kernel(T* __restrict__ v, double* __restrict__ lexv, const int* __restrict__ lex_of_site, int V, int nreal) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)V * nreal) return;
  const size_t s = i / nreal; const int r = (int)(i - s * nreal);
  if constexpr (TO_LEX) lexv[(size_t)lex_of_site[s] * nreal + r] = (double)v[i];
  else v[i] = (T)lexv[(size_t)lex_of_site[s] * nreal + r];
}
template <typename T>
void aos_from_lex(T* dst, const double* src, const int* lex_of_site, int V, int ndof, hipStream_t st) {
  size_t total = (size_t)V * 2 * ndof;
  hipLaunchKernelGGL((aos_lex_kernel<T, false>), dim3((total + 255) / 256), dim3(256), 0, st, dst, const_cast<double*>(src), lex_of_site, V, 2 * ndof);
  DDAMG_HIP_CHECK(hipGetLastError());
}
template <typename T>
void aos_to_lex(double* dst, const T* src, const int* lex_of_site, int V, int ndof, hipStream_t st) {
  size_t total = (size_t)V * 2 * ndof;
  hipLaunchKernelGGL((aos_lex_kernel<T, true>), dim3((total + 255) / 256), dim3(256), 0, st, const_cast<T*>(src), dst, lex_of_site, V, 2 * ndof);
  DDAMG_HIP_CHECK(hipGetLastError());
}
template void aos_from_lex<float>(float*, const double*, const int*, int, int, hipStream_t);
template void aos_from_lex<double>(double*, const double*, const int*, int, int, hipStream_t);
template void aos_to_lex<float>(double*, const float*, const int*, int, int, hipStream_t);
template void aos_to_lex<double>(double*, const double*, const int*, int, int, hipStream_t);

template class FineOp<float>;
template class FineOp<double>;
template void vec_from_lex<float>(float*, const double*, const int*, int, int, hipStream_t, bool);
template void vec_from_lex<double>(double*, const double*, const int*, int, int, hipStream_t, bool);
template void vec_to_lex<float>(double*, const float*, const int*, int, int, hipStream_t, bool);
template void vec_to_lex<double>(double*, const double*, const int*, int, int, hipStream_t, bool);

}  // namespace ddamg
