// gauge_device.hip -- clover term and plaquette on the device, for the own lattice of a single process and for the
// lattice extended by the neighbours' links on a process grid (gauge.cpp fetches them for links in host memory, ExtendedLinks,
// extended_links.h, for links in device memory).
// Reference: compute_clover_term src/dirac.c:24-58, Q / Qdiff / set_clover :304-402, calc_plaq :568-622.
// One thread per lexicographic site; links are read straight from the reference layout [V][4][3x3] complex fp64.
#include "gauge.h"
#include "common.h"
#include "extended_links.h"
#include "field_strength.h"
#include "geometry.h"
#include "halo.h"
#include <algorithm>
#include <cstdint>
#include <vector>

namespace ddamg {

namespace {
struct cplx { double r, i; };
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return cplx{a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
struct M3d { cplx a[9]; };

__device__ __forceinline__ M3d load_link(const double* __restrict__ U, size_t lx, int mu) {
  M3d m; const double* p = U + (lx * 4 + mu) * 18;
#pragma unroll
  for (int k = 0; k < 9; k++) m.a[k] = cplx{p[2 * k], p[2 * k + 1]};
  return m;
}
__device__ __forceinline__ M3d mmul(const M3d& x, const M3d& y) {
  M3d r;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      cplx s{0, 0};
#pragma unroll
      for (int k = 0; k < 3; k++) { cplx t = cmul(x.a[3 * i + k], y.a[3 * k + j]); s.r += t.r; s.i += t.i; }
      r.a[3 * i + j] = s;
    }
  return r;
}
__device__ __forceinline__ M3d mdag(const M3d& x) {
  M3d r;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) r.a[3 * i + j] = cplx{x.a[3 * j + i].r, -x.a[3 * j + i].i};
  return r;
}

struct Lat { int L[4]; };
__device__ __forceinline__ size_t lexd(const Lat& g, const int c[4]) { return ((size_t)(c[0] * g.L[1] + c[1]) * g.L[2] + c[2]) * g.L[3] + c[3]; }
__device__ __forceinline__ void shiftd(const Lat& g, const int c[4], int mu, int d, int out[4]) {
  out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
  out[mu] = (c[mu] + d + g.L[mu]) % g.L[mu];
}

// sum of the four plaquette leaves in the (mu,nu) plane at x, divided by 16 (src/dirac.c:304-358)
__device__ M3d leaves(const double* __restrict__ U, const Lat& g, const int x[4], int mu, int nu) {
  int xpm[4], xpn[4], xmm[4], xmn[4], xpnmm[4], xmmmn[4], xmnpm[4];
  shiftd(g, x, mu, +1, xpm); shiftd(g, x, nu, +1, xpn);
  shiftd(g, x, mu, -1, xmm); shiftd(g, x, nu, -1, xmn);
  shiftd(g, xpn, mu, -1, xpnmm); shiftd(g, xmm, nu, -1, xmmmn); shiftd(g, xmn, mu, +1, xmnpm);
  const size_t lx = lexd(g, x), lxpm = lexd(g, xpm), lxpn = lexd(g, xpn), lxmm = lexd(g, xmm), lxmn = lexd(g, xmn);
  M3d q = mmul(mmul(mmul(load_link(U, lx, mu), load_link(U, lxpm, nu)), mdag(load_link(U, lxpn, mu))), mdag(load_link(U, lx, nu)));
  M3d t = mmul(mmul(mmul(load_link(U, lx, nu), mdag(load_link(U, lexd(g, xpnmm), mu))), mdag(load_link(U, lxmm, nu))), load_link(U, lxmm, mu));
#pragma unroll
  for (int k = 0; k < 9; k++) { q.a[k].r += t.a[k].r; q.a[k].i += t.a[k].i; }
  const size_t lxmmmn = lexd(g, xmmmn);
  t = mmul(mmul(mmul(mdag(load_link(U, lxmm, mu)), mdag(load_link(U, lxmmmn, nu))), load_link(U, lxmmmn, mu)), load_link(U, lxmn, nu));
#pragma unroll
  for (int k = 0; k < 9; k++) { q.a[k].r += t.a[k].r; q.a[k].i += t.a[k].i; }
  t = mmul(mmul(mmul(mdag(load_link(U, lxmn, nu)), load_link(U, lxmn, mu)), load_link(U, lexd(g, xmnpm), nu)), mdag(load_link(U, lx, mu)));
#pragma unroll
  for (int k = 0; k < 9; k++) { q.a[k].r = (q.a[k].r + t.a[k].r) / 16.0; q.a[k].i = (q.a[k].i + t.a[k].i) / 16.0; }
  return q;
}

struct GammaProducts { double re[6][16], im[6][16]; };   // gamma_mu gamma_nu for the six planes mu < nu

// U: links of the lattice g (the own one, or the own one extended by a shell `halo` sites deep in the split directions:
// then the wrap-around of `shiftd` is never taken in those directions); one thread per site of the own lattice `loc`
__global__ __launch_bounds__(64) void clover_kernel(double* __restrict__ clover, double* __restrict__ plaq_site, const double* __restrict__ U,
                                                    Lat g, Lat loc, Lat halo, int V, double m0, double csw, GammaProducts gp) {
  const int site = blockIdx.x * 64 + threadIdx.x;
  if (site >= V) return;
  int x[4]; int r = site;
  x[3] = r % loc.L[3]; r /= loc.L[3]; x[2] = r % loc.L[2]; r /= loc.L[2]; x[1] = r % loc.L[1]; r /= loc.L[1]; x[0] = r;
#pragma unroll
  for (int mu = 0; mu < 4; mu++) x[mu] += halo.L[mu];
  const size_t lx = lexd(g, x);
  double clr[42], cli[42];
  for (int k = 0; k < 42; k++) { clr[k] = k < 12 ? 4.0 + m0 : 0.0; cli[k] = 0.0; }
  double pl = 0;
  int plane = 0;
  for (int mu = 0; mu < 4; mu++)
    for (int nu = mu + 1; nu < 4; nu++, plane++) {
      int xpm[4], xpn[4];
      shiftd(g, x, mu, +1, xpm); shiftd(g, x, nu, +1, xpn);
      const M3d p = mmul(mmul(mmul(load_link(U, lx, mu), load_link(U, lexd(g, xpm), nu)), mdag(load_link(U, lexd(g, xpn), mu))), mdag(load_link(U, lx, nu)));
      pl += p.a[0].r + p.a[4].r + p.a[8].r;
      if (csw != 0.0) {
        const M3d q = leaves(U, g, x, mu, nu), qt = leaves(U, g, x, nu, mu);
        cplx qd[9];
        for (int k = 0; k < 9; k++) qd[k] = cplx{q.a[k].r - qt.a[k].r, q.a[k].i - qt.a[k].i};
        // tensor = -csw * (gamma_mu gamma_nu) (x) Qdiff; keep the diagonal and the strict upper parts of both 6x6 blocks
        auto T = [&](int i, int j) -> cplx {
          const int gi = 4 * (i / 3) + (j / 3);
          cplx t = cmul(cplx{gp.re[plane][gi], gp.im[plane][gi]}, qd[3 * (i % 3) + (j % 3)]);
          return cplx{-csw * t.r, -csw * t.i};
        };
        for (int k = 0; k < 12; k++) { cplx t = T(k, k); clr[k] += t.r; cli[k] += t.i; }
        int k = 12;
        for (int i = 0; i < 6; i++) for (int j = i + 1; j < 6; j++, k++) { cplx t = T(i, j); clr[k] += t.r; cli[k] += t.i; }
        for (int i = 6; i < 12; i++) for (int j = i + 1; j < 12; j++, k++) { cplx t = T(i, j); clr[k] += t.r; cli[k] += t.i; }
      }
    }
  for (int k = 0; k < 42; k++) { clover[((size_t)site * 42 + k) * 2] = clr[k]; clover[((size_t)site * 42 + k) * 2 + 1] = cli[k]; }
  plaq_site[site] = pl;
}

__global__ void scale_links_kernel(double* __restrict__ D, double* __restrict__ U, size_t n, int anti_pbc, size_t first_last_slice, int Lx_links) {
  // D = U/2 after the optional sign flip of the T-links of the last time slice (src/io.c:536-541, src/dirac.c:80); U is
  // updated in place so that the clover kernel sees the same links
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // one real
  if (i >= n) return;
  double u = U[i];
  if (anti_pbc && i >= first_last_slice && ((i / 18) % 4) == 0) { u = -u; U[i] = u; }
  D[i] = 0.5 * u;
  (void)Lx_links;
}
static GammaProducts gamma_products() {
  // gamma_mu gamma_nu (BASIS0, src/clifford.h:39-100)
  static const int col[4][4] = {{2, 3, 0, 1}, {3, 2, 1, 0}, {3, 2, 1, 0}, {2, 3, 0, 1}};
  static const double vre[4][4] = {{-1, -1, -1, -1}, {0, 0, 0, 0}, {-1, 1, 1, -1}, {0, 0, 0, 0}};
  static const double vim[4][4] = {{0, 0, 0, 0}, {-1, -1, 1, 1}, {0, 0, 0, 0}, {-1, 1, 1, -1}};
  GammaProducts gp;
  int plane = 0;
  for (int mu = 0; mu < 4; mu++)
    for (int nu = mu + 1; nu < 4; nu++, plane++) {
      for (int k = 0; k < 16; k++) { gp.re[plane][k] = 0; gp.im[plane][k] = 0; }
      for (int i = 0; i < 4; i++) {   // (gamma_mu gamma_nu)[i][j] = gamma_mu[i][c] * gamma_nu[c][j], one non-zero per row each
        const int c = col[mu][i], j = col[nu][c];
        const double ar = vre[mu][i], ai = vim[mu][i], br = vre[nu][c], bi = vim[nu][c];
        gp.re[plane][4 * i + j] = ar * br - ai * bi; gp.im[plane][4 * i + j] = ar * bi + ai * br;
      }
    }
  return gp;
}

// clover term of the V own sites into clover_out (host) and the sum of their plaquette traces; dU: links of the lattice
// `ext` on the device
static double clover_and_plaquette_on_device(const double* dU, const Lat& ext, const Lat& loc, const Lat& halo, double m0, double csw, double* clover_out, hipStream_t st) {
  const size_t V = (size_t)loc.L[0] * loc.L[1] * loc.L[2] * loc.L[3];
  DeviceBuffer<double> dC, dP;
  dC.alloc(84 * V);
  dP.alloc(V);
  hipLaunchKernelGGL(clover_kernel, dim3((unsigned)((V + 63) / 64)), dim3(64), 0, st, dC, dP, dU, ext, loc, halo, (int)V, m0, csw, gamma_products());
  DDAMG_HIP_CHECK(hipGetLastError());
  std::vector<double> hp(V);
  DDAMG_HIP_CHECK(hipMemcpyAsync(clover_out, dC, sizeof(double) * 84 * V, hipMemcpyDeviceToHost, st));
  DDAMG_HIP_CHECK(hipMemcpyAsync(hp.data(), dP, sizeof(double) * V, hipMemcpyDeviceToHost, st));
  DDAMG_HIP_CHECK(hipStreamSynchronize(st));
  double plaq = 0;
  for (size_t i = 0; i < V; i++) plaq += hp[i];
  return plaq;
}
}  // namespace

double gauge_to_operator_device(const int L[4], const double* gauge_in, int anti_pbc, double m0, double csw, double* D_out, double* clover_out,
                                hipStream_t st) {
  const size_t V = (size_t)L[0] * L[1] * L[2] * L[3];
  DeviceBuffer<double> dU, dD;
  dU.alloc(72 * V);
  dD.alloc(72 * V);
  DDAMG_HIP_CHECK(hipMemcpyAsync(dU, gauge_in, sizeof(double) * 72 * V, hipMemcpyHostToDevice, st));
  const size_t vol3 = (size_t)L[1] * L[2] * L[3];
  hipLaunchKernelGGL(scale_links_kernel, dim3((unsigned)((72 * V + 255) / 256)), dim3(256), 0, st, dD, dU, 72 * V, anti_pbc,
                     (size_t)(L[0] - 1) * vol3 * 72, 0);
  DDAMG_HIP_CHECK(hipMemcpyAsync(D_out, dD, sizeof(double) * 72 * V, hipMemcpyDeviceToHost, st));
  Lat g, none; for (int mu = 0; mu < 4; mu++) { g.L[mu] = L[mu]; none.L[mu] = 0; }
  const double plaq = clover_and_plaquette_on_device(dU, g, g, none, m0, csw, clover_out, st);
  return plaq / ((double)V * 6.0);
}

double clover_and_plaquette_extended_device(const int L[4], const int halo[4], const double* U_ext_host, double m0, double csw, double* clover_out, hipStream_t st) {
  Lat ext, loc, h; size_t Ve = 1;
  for (int mu = 0; mu < 4; mu++) { loc.L[mu] = L[mu]; h.L[mu] = halo[mu]; ext.L[mu] = L[mu] + 2 * halo[mu]; Ve *= ext.L[mu]; }
  DeviceBuffer<double> dU;
  dU.alloc(72 * Ve);
  DDAMG_HIP_CHECK(hipMemcpyAsync(dU, U_ext_host, sizeof(double) * 72 * Ve, hipMemcpyHostToDevice, st));
  const double plaq = clover_and_plaquette_on_device(dU, ext, loc, h, m0, csw, clover_out, st);
  return plaq;
}


// ---- links that the caller keeps in device memory (ddamg_hip_set_gauge_device, _set_gauge_device_grid) -----------------------
// The links are read in place and never written: the anti-periodic sign is applied in the loads (on a process grid: in the copy
// into the extended array).  Kernel bodies: field_strength.h.
namespace {
// F of one plane for an 8 x 8 tile of its sites (grid: x = tiles, y = the six planes) and the tile's sum of plaquette traces.
// EXTENDED: U is the lattice extended by the neighbours' links (shell); tiles, F and the sums stay those of the own lattice
template <bool EXTENDED>
__global__ __launch_bounds__(fs::THREADS) void field_strength_kernel(double* __restrict__ F, double* __restrict__ plaq_block, const double* __restrict__ U,
                                                                      fs::Planes g, size_t V, int anti_pbc, fs::Shell shell) {
  __shared__ double lds[fs::LDS_DOUBLES];
  __shared__ size_t off[2 * fs::EXT];
  __shared__ int flip[fs::EXT];
  const int p = blockIdx.y, block = blockIdx.x, tid = threadIdx.x;
  const size_t slot = (size_t)p * g.max_blocks + block;
  if (block >= g.nblocks[p]) {   // planes of a lattice with unequal extents have unequal numbers of tiles
    if (tid == 0) plaq_block[slot] = 0.0;
    return;
  }
  const fs::Tile t = fs::tile_of(g, p, block);
  if constexpr (EXTENDED) {
    const fs::Tile te = fs::extended_tile(g, shell, t, block);
    fs::stage_offsets<true>(g, te, 0, tid, off, flip, &shell);
    __syncthreads();
    fs::stage_links(U, te, tid, off, flip, lds);
  } else {
    fs::stage_offsets(g, t, anti_pbc, tid, off, flip);
    __syncthreads();
    fs::stage_links(U, t, tid, off, flip, lds);
  }
  __syncthreads();
  size_t lex = 0; double f[9]; double pl = 0.0;
  if (fs::site_field_strength(g, t, tid, lds, &lex, f, &pl)) {
#pragma unroll
    for (int r = 0; r < 9; r++) F[((size_t)p * 9 + r) * V + lex] = f[r];
  } else {
    pl = 0.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pl += __shfl_down(pl, o, 64);   // the workgroup is one wave
  if (tid == 0) plaq_block[slot] = pl;
}

// the caller's links into the interior of the extended array, W reals per thread (fs::extend_links)
template <int W>
__global__ __launch_bounds__(256) void links_extend_kernel(double* __restrict__ Ue, const double* __restrict__ U, fs::Shell shell, int negate_last_t) {
  fs::extend_links<W>(shell, U, Ue, (size_t)blockIdx.x * 256 + threadIdx.x, negate_last_t);
}
// one slab of the extended array into a contiguous buffer, and a received buffer into the slab one site further out (fs::slab_copy)
__global__ __launch_bounds__(256) void link_slab_pack_kernel(double* __restrict__ buf, double* __restrict__ Ue, fs::Shell shell, fs::Slab slab) {
  fs::slab_copy(shell, slab, Ue, buf, (size_t)blockIdx.x * 256 + threadIdx.x, true);
}
__global__ __launch_bounds__(256) void link_slab_unpack_kernel(double* __restrict__ Ue, double* __restrict__ buf, fs::Shell shell, fs::Slab slab) {
  fs::slab_copy(shell, slab, Ue, buf, (size_t)blockIdx.x * 256 + threadIdx.x, false);
}

__global__ __launch_bounds__(128) void clover_assemble_kernel(double* __restrict__ clover, const double* __restrict__ F, size_t V, double m0, double csw,
                                                              fs::GammaProducts gp) {
  const size_t lex = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (lex >= V) return;
  fs::site_clover(F, V, lex, m0, csw, gp, clover);
}

// second stage of the plaquette sum: one workgroup, every thread a fixed subsequence, then a tree -- the same sum on every run
__global__ __launch_bounds__(256) void plaquette_sum_kernel(double* __restrict__ out, const double* __restrict__ part, size_t n) {
  __shared__ double sh[256];
  double s = 0.0;
  for (size_t i = threadIdx.x; i < n; i += 256) s += part[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

// D = U/2 with the anti-periodic sign of the T-links of the last time slice (src/io.c:536-541, src/dirac.c:80); one real per thread
__global__ __launch_bounds__(256) void links_to_D_kernel(double* __restrict__ D, const double* __restrict__ U, size_t n, int anti_pbc, size_t first_last_slice) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double u = U[i];
  D[i] = (anti_pbc && i >= first_last_slice && ((i / 18) % 4) == 0) ? -0.5 * u : 0.5 * u;
}

fs::GammaProducts gamma_products_fs() {
  const GammaProducts a = gamma_products();
  fs::GammaProducts b;
  for (int p = 0; p < 6; p++) for (int k = 0; k < 16; k++) { b.re[p][k] = a.re[p][k]; b.im[p][k] = a.im[p][k]; }
  return b;
}

// work space of the three kernels: F (54 reals per site), the tiles' plaquette sums and the total
struct ResidentWork {
  fs::Planes planes;
  size_t V;
  DeviceBuffer<double> F, part;
  ResidentWork(const int L[4]) : planes(fs::make_planes(L)), V((size_t)L[0] * L[1] * L[2] * L[3]) {
    F.alloc(54 * V);
    part.alloc(6 * (size_t)planes.max_blocks + 1);
  }
  double* total() { return part + 6 * (size_t)planes.max_blocks; }
  void field_strength(const double* dU, int anti_pbc, hipStream_t st) {
    hipLaunchKernelGGL(field_strength_kernel<false>, dim3((unsigned)planes.max_blocks, 6), dim3(fs::THREADS), 0, st, F, part, dU, planes, V, anti_pbc,
                       fs::Shell{});
    DDAMG_HIP_CHECK(hipGetLastError());
  }
  void field_strength_extended(const double* dUe, const fs::Shell& shell, hipStream_t st) {   // the sign is in dUe
    hipLaunchKernelGGL(field_strength_kernel<true>, dim3((unsigned)planes.max_blocks, 6), dim3(fs::THREADS), 0, st, F, part, dUe, planes, V, 0, shell);
    DDAMG_HIP_CHECK(hipGetLastError());
  }
  void assemble(double* dC, double m0, double csw, hipStream_t st) {
    hipLaunchKernelGGL(clover_assemble_kernel, dim3((unsigned)((V + 127) / 128)), dim3(128), 0, st, dC, F, V, m0, csw, gamma_products_fs());
    DDAMG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(plaquette_sum_kernel, dim3(1), dim3(256), 0, st, total(), part, 6 * (size_t)planes.max_blocks);
    DDAMG_HIP_CHECK(hipGetLastError());
  }
  double plaquette_sum(hipStream_t st) {   // over the own sites and the planes; waits for the stream
    double sum = 0;
    DDAMG_HIP_CHECK(hipMemcpyAsync(&sum, total(), sizeof(double), hipMemcpyDeviceToHost, st));
    DDAMG_HIP_CHECK(hipStreamSynchronize(st));
    return sum;
  }
  double plaquette(hipStream_t st) { return plaquette_sum(st) / ((double)V * 6.0); }   // the average
};

}  // namespace

// ExtendedLinks (extended_links.h)
void ExtendedLinks::fill(const Geometry& g, Comm* comm, const double* dU, int anti_pbc, hipStream_t st) {
  const int negate_last_t = (anti_pbc && g.pc[0] == g.P[0] - 1) ? 1 : 0;
  if (reinterpret_cast<uintptr_t>(dU) % 16 == 0)
    hipLaunchKernelGGL(links_extend_kernel<2>, dim3((unsigned)((shell.V * 36 + 255) / 256)), dim3(256), 0, st, Ue, dU, shell, negate_last_t);
  else
    hipLaunchKernelGGL(links_extend_kernel<1>, dim3((unsigned)((shell.V * 72 + 255) / 256)), dim3(256), 0, st, Ue, dU, shell, negate_last_t);
  DDAMG_HIP_CHECK(hipGetLastError());
  for (int mu = 0; mu < 4; mu++) {
    if (!shell.h[mu]) continue;
    const fs::Slab slab = fs::make_slab(shell, mu);
    const unsigned blocks = (unsigned)((slab.sites * 36 + 255) / 256);
    for (int side = 0; side < 2; side++) {
      // side 0: my slices x_mu = L-h .. L-1 go to the +mu neighbour (its x_mu = -h .. -1); side 1: x_mu = 0 .. h-1 to the -mu
      // neighbour (its x_mu = L .. L+h-1); h: the depth of the shell
      const int h = shell.h[mu];
      const int src_c = side == 0 ? shell.L[mu] - h : 0, dst_c = side == 0 ? -h : shell.L[mu];
      hipLaunchKernelGGL(link_slab_pack_kernel, dim3(blocks), dim3(256), 0, st, sbuf, Ue, shell, fs::slab_at(shell, slab, src_c));
      DDAMG_HIP_CHECK(hipGetLastError());
      comm_sendrecv_device(comm, sbuf, g.neighbor_rank[side == 0 ? mu : 4 + mu], rbuf, g.neighbor_rank[side == 0 ? 4 + mu : mu],
                           sizeof(double) * 72 * slab.sites, 100 + 2 * mu + side, st);
      hipLaunchKernelGGL(link_slab_unpack_kernel, dim3(blocks), dim3(256), 0, st, Ue, rbuf, shell, fs::slab_at(shell, slab, dst_c));
      DDAMG_HIP_CHECK(hipGetLastError());
    }
  }
}

double gauge_to_operator_resident(const int L[4], const double* dU_hopp, const double* dU_clover, int anti_pbc, double m0, double csw, double* dD,
                                  double* dC, hipStream_t st) {
  ResidentWork w(L);
  const size_t n = 72 * w.V, vol3 = (size_t)L[1] * L[2] * L[3];
  hipLaunchKernelGGL(links_to_D_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dD, dU_hopp, n, anti_pbc, (size_t)(L[0] - 1) * vol3 * 72);
  DDAMG_HIP_CHECK(hipGetLastError());
  w.field_strength(dU_clover, anti_pbc, st);
  w.assemble(dC, m0, csw, st);
  return w.plaquette(st);
}

double gauge_to_operator_resident_grid(const Geometry& g, Comm* comm, const double* dU_hopp, const double* dU_clover, int anti_pbc, double m0, double csw,
                                       double* dD, double* dC, hipStream_t st) {
  DDAMG_REQUIRE(comm != nullptr, "process grid > 1 but no transport: call ddamg_hip_comm_init_rccl or ddamg_hip_comm_init_host first");
  ResidentWork w(g.L);
  // D needs the own links only; the last global time slice lives on the processes at the end of the T direction of the grid
  const int negate_last_t = (anti_pbc && g.pc[0] == g.P[0] - 1) ? 1 : 0;
  const size_t n = 72 * w.V, vol3 = (size_t)g.L[1] * g.L[2] * g.L[3];
  hipLaunchKernelGGL(links_to_D_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dD, dU_hopp, n, negate_last_t, (size_t)(g.L[0] - 1) * vol3 * 72);
  DDAMG_HIP_CHECK(hipGetLastError());
  ExtendedLinks x(g);
  x.fill(g, comm, dU_clover, anti_pbc, st);
  w.field_strength_extended(x.Ue, x.shell, st);
  w.assemble(dC, m0, csw, st);
  double acc[2] = {w.plaquette_sum(st), (double)w.V * 6.0};   // the stream is idle now: x may go
  comm_allreduce_host(comm, acc, 2);
  comm_release_device_staging(comm);
  return acc[0] / acc[1];
}

double extended_field_strength_timed(const Geometry& g, Comm* comm, const double* dU, int reps, hipEvent_t e0, hipEvent_t e1, hipStream_t st, float* ms) {
  DDAMG_REQUIRE(comm != nullptr && reps >= 1, "extended_field_strength_timed: a transport and reps >= 1");
  ResidentWork w(g.L);
  ExtendedLinks x(g);
  x.fill(g, comm, dU, 0, st);
  for (int r = -1; r < reps; r++) {   // r = -1: untimed first launch
    if (r == 0) DDAMG_HIP_CHECK(hipEventRecord(e0, st));
    w.field_strength_extended(x.Ue, x.shell, st);
  }
  DDAMG_HIP_CHECK(hipEventRecord(e1, st));
  DDAMG_HIP_CHECK(hipEventSynchronize(e1));
  DDAMG_HIP_CHECK(hipEventElapsedTime(ms, e0, e1));
  *ms /= (float)reps;
  DeviceBuffer<double> dC;
  dC.alloc(84 * w.V);
  w.assemble(dC, 0.0, 0.0, st);
  const double pl = w.plaquette(st);
  comm_release_device_staging(comm);
  return pl;
}

double clover_kernels_timed(const int L[4], const double* dU, double m0, double csw, int which, int reps, hipEvent_t e0, hipEvent_t e1, hipStream_t st,
                            float* ms) {
  DDAMG_REQUIRE(which >= 0 && which <= 2 && reps >= 1, "clover_kernels_timed: which is 0, 1 or 2 and reps >= 1");
  ResidentWork w(L);
  DeviceBuffer<double> dC, dP;
  dC.alloc(84 * w.V);
  Lat g, none; for (int mu = 0; mu < 4; mu++) { g.L[mu] = L[mu]; none.L[mu] = 0; }
  if (which == 1) dP.alloc(w.V);
  for (int r = -1; r < reps; r++) {   // r = -1: untimed first launch
    if (r == 0) DDAMG_HIP_CHECK(hipEventRecord(e0, st));
    if (which == 1) {
      hipLaunchKernelGGL(clover_kernel, dim3((unsigned)((w.V + 63) / 64)), dim3(64), 0, st, dC, dP, dU, g, g, none, (int)w.V, m0, csw, gamma_products());
      DDAMG_HIP_CHECK(hipGetLastError());
    } else {
      w.field_strength(dU, 0, st);
      if (which == 2) w.assemble(dC, m0, csw, st);
    }
  }
  DDAMG_HIP_CHECK(hipEventRecord(e1, st));
  DDAMG_HIP_CHECK(hipEventSynchronize(e1));
  DDAMG_HIP_CHECK(hipEventElapsedTime(ms, e0, e1));
  *ms /= (float)reps;
  if (which == 1) {
    std::vector<double> hp(w.V);
    DDAMG_HIP_CHECK(hipMemcpy(hp.data(), dP, sizeof(double) * w.V, hipMemcpyDeviceToHost));
    double s = 0; for (size_t i = 0; i < w.V; i++) s += hp[i];
    return s / ((double)w.V * 6.0);
  }
  if (which == 0) w.assemble(dC, m0, csw, st);
  return w.plaquette(st);
}

}  // namespace ddamg
