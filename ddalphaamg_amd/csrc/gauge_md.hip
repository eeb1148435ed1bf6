// gauge_md.hip -- the gauge sector of the molecular dynamics (ddamg_hip_gauge_*, ddamg_hip_links_*, ddamg_hip_momentum_*): kernels
// around the bodies of gauge_md.h.  Launches of one call:
//   gauge_loops          gauge_loops_kernel<H> (x = tiles, y = the six planes), reduce_partials_kernel
//   gauge_force          gauge_force_kernel<H> (the same grid), gauge_force_assemble_kernel       H = 1 where c1 == 0, else 2
//   links_update         links_update_kernel
//   links_reunitarize    links_reunitarize_kernel, and where the deviation is asked for reduce_partials_kernel
//   momentum_update      momentum_update_kernel
//   momentum_kinetic     momentum_kinetic_kernel, reduce_partials_kernel
// On a process grid (gauge_loops_grid, gauge_force_grid) ExtendedLinks::fill at depth H comes first: the extend pass and per split
// direction two packs, two messages and two unpacks; the plane kernels then read the extended array and write the own lattice.
// No atomics: every number is written by one thread.  A sum or maximum is taken in two stages, the workgroups' parts in a fixed
// order by ONE workgroup, so two calls give the same bits.
#include "common.h"
#include "gauge_md.h"

namespace ddamg {

namespace {
// grid: x = tiles, y = the six planes; one workgroup = one wave = an 8 x 8 tile (field_strength.h).  The plane's part of the two
// links every site of the tile owns, into their slots of that plane.  U: the links of the lattice extended by `shell` (a process
// grid), or the caller's own with a shell of depth 0 (undivided): ONE kernel for both, so that the compiler contracts the same
// products and the two give the same bits.  Tiles, slots and sums are those of the own lattice.
template <int H>
__global__ __launch_bounds__(fs::THREADS) void gauge_force_kernel(double* __restrict__ slots, const double* __restrict__ U, fs::Planes g, size_t V, double beta,
                                                                   double c0, double c1, fs::Shell shell) {
  __shared__ double lds[gmd::Nb<H>::LDS_DOUBLES];
  __shared__ size_t off[2 * gmd::Nb<H>::EXT];
  const int p = blockIdx.y, block = blockIdx.x, tid = threadIdx.x;
  if (block >= g.nblocks[p]) return;
  const fs::Tile t = fs::tile_of(g, p, block);
  const fs::Tile te = fs::extended_tile(g, shell, t, block);     // where the loads go; t: where the results go
  gmd::stage_offsets<H>(g, te, shell, tid, off);
  __syncthreads();
  gmd::stage_links<H>(U, te, tid, off, lds);
  __syncthreads();
  size_t lex = 0; double out[2][9];
  if (gmd::site_gauge_force<H>(g, t, tid, lds, beta, c0, c1, &lex, out)) {
    const int smu = t.mu * force::SLOTS + force::plane_slot(t.mu, t.nu), snu = t.nu * force::SLOTS + force::plane_slot(t.nu, t.mu);
#pragma unroll
    for (int r = 0; r < 9; r++) {
      slots[((size_t)smu * 9 + r) * V + lex] = out[0][r];
      slots[((size_t)snu * 9 + r) * V + lex] = out[1][r];
    }
  }
}

__global__ __launch_bounds__(128) void gauge_force_assemble_kernel(double* __restrict__ out, const double* __restrict__ slots, size_t V, double coeff,
                                                                   int accumulate) {
  force::site_assemble(slots, V, (size_t)blockIdx.x * 128 + threadIdx.x, 1, 0, coeff, accumulate, out);
}

// the tile's sums of Re tr P and (H = 2) Re tr R: part[p * max_blocks + block], and behind the 6 max_blocks of the plaquette those
// of the rectangle.  A plane with fewer tiles than the largest writes zeros there
template <int H>
__global__ __launch_bounds__(fs::THREADS) void gauge_loops_kernel(double* __restrict__ part, const double* __restrict__ U, fs::Planes g, fs::Shell shell) {
  __shared__ double lds[gmd::Nb<H>::LDS_DOUBLES];
  __shared__ size_t off[2 * gmd::Nb<H>::EXT];
  const int p = blockIdx.y, block = blockIdx.x, tid = threadIdx.x;
  const size_t slot = (size_t)p * g.max_blocks + block, rect_slot = 6 * (size_t)g.max_blocks + slot;
  if (block >= g.nblocks[p]) {
    if (tid == 0) { part[slot] = 0.0; if (H == 2) part[rect_slot] = 0.0; }
    return;
  }
  const fs::Tile t = fs::tile_of(g, p, block);
  const fs::Tile te = fs::extended_tile(g, shell, t, block);     // where the loads go; t: where the results go
  gmd::stage_offsets<H>(g, te, shell, tid, off);
  __syncthreads();
  gmd::stage_links<H>(U, te, tid, off, lds);
  __syncthreads();
  double pl, re;
  gmd::site_gauge_loops<H>(g, t, tid, lds, &pl, &re);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { pl += __shfl_down(pl, o, 64); re += __shfl_down(re, o, 64); }   // the workgroup is one wave
  if (tid == 0) { part[slot] = pl; if (H == 2) part[rect_slot] = re; }
}

__global__ __launch_bounds__(256) void links_update_kernel(double* __restrict__ U, const double* __restrict__ P, double eps, size_t nlinks) {
  gmd::link_update(U, P, eps, nlinks, (size_t)blockIdx.x * 256 + threadIdx.x);
}

// the sum (MAX: the maximum) over the workgroup, in thread 0: a tree in LDS, the same on every run
template <bool MAX>
__device__ __forceinline__ double block_reduce(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = gmd::REDUCE_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double a = sh[threadIdx.x], b = sh[threadIdx.x + o];
      sh[threadIdx.x] = MAX ? (b > a || b != b ? b : a) : a + b;     // a NaN wins: a field that is not finite is reported as such
    }
    __syncthreads();
  }
  return sh[0];
}

// part == nullptr: nobody asked for the deviation
__global__ __launch_bounds__(gmd::REDUCE_THREADS) void links_reunitarize_kernel(double* __restrict__ U, size_t nlinks, double* __restrict__ part) {
  __shared__ double sh[gmd::REDUCE_THREADS];
  const double dev = gmd::link_reunitarize(U, nlinks, (size_t)blockIdx.x * gmd::REDUCE_THREADS + threadIdx.x);
  if (part == nullptr) return;
  const double m = block_reduce<true>(dev, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}

__global__ __launch_bounds__(256) void momentum_update_kernel(double* __restrict__ P, const double* __restrict__ F, double eps, size_t n) {
  gmd::momentum_update(P, F, eps, n, (size_t)blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(gmd::REDUCE_THREADS) void momentum_kinetic_kernel(double* __restrict__ part, const double* __restrict__ P, size_t n) {
  __shared__ double sh[gmd::REDUCE_THREADS];
  const double s = block_reduce<false>(gmd::kinetic_part(P, n, blockIdx.x, threadIdx.x), sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// second stage, one workgroup per result (x): out[x] = the sum (MAX: the maximum) of part[x * n .. x * n + n), every thread a fixed
// subsequence, then the tree
template <bool MAX>
__global__ __launch_bounds__(gmd::REDUCE_THREADS) void reduce_partials_kernel(double* __restrict__ out, const double* __restrict__ part, size_t n) {
  __shared__ double sh[gmd::REDUCE_THREADS];
  const double* p = part + (size_t)blockIdx.x * n;
  double s = 0.0;
  for (size_t i = threadIdx.x; i < n; i += gmd::REDUCE_THREADS) {
    const double v = p[i];
    s = MAX ? (v > s || v != v ? v : s) : s + v;
  }
  s = block_reduce<MAX>(s, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// room for n parts and, behind them, two results
double* parts(GaugeMdWork& w, size_t n) {
  if (w.part.size() < n + 2) w.part.alloc(n + 2);
  return w.part.get();
}

// results [0, count) behind the n parts, to the host; waits for the stream
template <bool MAX>
void reduce_to_host(double* part, size_t n, int count, double* host, hipStream_t st) {
  double* out = part + (size_t)count * n;
  hipLaunchKernelGGL(reduce_partials_kernel<MAX>, dim3((unsigned)count), dim3(gmd::REDUCE_THREADS), 0, st, out, part, n);
  DDAMG_HIP_CHECK(hipGetLastError());
  DDAMG_HIP_CHECK(hipMemcpyAsync(host, out, sizeof(double) * count, hipMemcpyDeviceToHost, st));
  DDAMG_HIP_CHECK(hipStreamSynchronize(st));
}

// the shell of an undivided lattice: no direction split, the extended array is the caller's
fs::Shell no_shell(const int L[4]) {
  const bool split[4] = {false, false, false, false};
  return fs::make_shell(L, split, 0);
}

// the extended links of a depth, made at the first call; then the caller's links and the neighbours' shell into them.  That there
// is a transport is the entry point's to check (capi.cpp, require_gauge_collective), before anything is enqueued
ExtendedLinks& extended(GaugeMdWork& w, const Geometry& g, Comm* comm, int depth, const double* dU, hipStream_t st) {
  std::unique_ptr<ExtendedLinks>& x = w.extended[depth - 1];
  if (!x) x.reset(new ExtendedLinks(g, depth));
  x->fill(g, comm, dU, 0, st);     // the caller's links: no anti-periodic sign
  return *x;
}

// the links dU of the lattice extended by `shell`, whose own lattice is shell.L
void loops_of(const fs::Shell& shell, const double* dU, double* plaq, double* rect, GaugeMdWork& w, hipStream_t st) {
  const fs::Planes planes = fs::make_planes(shell.L);
  const size_t n = 6 * (size_t)planes.max_blocks;
  const int count = rect ? 2 : 1;
  double* part = parts(w, (size_t)count * n);
  const dim3 grid((unsigned)planes.max_blocks, 6);
  if (rect) hipLaunchKernelGGL(gauge_loops_kernel<2>, grid, dim3(fs::THREADS), 0, st, part, dU, planes, shell);
  else hipLaunchKernelGGL(gauge_loops_kernel<1>, grid, dim3(fs::THREADS), 0, st, part, dU, planes, shell);
  DDAMG_HIP_CHECK(hipGetLastError());
  double sums[2] = {0.0, 0.0};
  reduce_to_host<false>(part, n, count, sums, st);
  *plaq = sums[0];
  if (rect) *rect = sums[1];
}

void force_of(const fs::Shell& shell, const double* dU, double beta, double c1, double coeff, int accumulate, double* force_dev, double* slots, hipStream_t st) {
  const fs::Planes planes = fs::make_planes(shell.L);
  const size_t V = shell.V;
  const double c0 = 1.0 - 8.0 * c1;
  const dim3 grid((unsigned)planes.max_blocks, 6);
  if (c1 == 0.0) hipLaunchKernelGGL(gauge_force_kernel<1>, grid, dim3(fs::THREADS), 0, st, slots, dU, planes, V, beta, c0, c1, shell);
  else hipLaunchKernelGGL(gauge_force_kernel<2>, grid, dim3(fs::THREADS), 0, st, slots, dU, planes, V, beta, c0, c1, shell);
  DDAMG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(gauge_force_assemble_kernel, dim3((unsigned)((V + 127) / 128)), dim3(128), 0, st, force_dev, slots, V, coeff, accumulate);
  DDAMG_HIP_CHECK(hipGetLastError());
}

}  // namespace

void gauge_loops(const int L[4], const double* dU, double* plaq, double* rect, GaugeMdWork& w, hipStream_t st) {
  loops_of(no_shell(L), dU, plaq, rect, w, st);
}
void gauge_loops_grid(const Geometry& g, Comm* comm, const double* dU, double* plaq, double* rect, GaugeMdWork& w, hipStream_t st) {
  const ExtendedLinks& x = extended(w, g, comm, gauge_depth(rect != nullptr), dU, st);
  loops_of(x.shell, x.Ue.get(), plaq, rect, w, st);
}

void gauge_force(const int L[4], const double* dU, double beta, double c1, double coeff, int accumulate, double* force_dev, double* slots, hipStream_t st) {
  force_of(no_shell(L), dU, beta, c1, coeff, accumulate, force_dev, slots, st);
}
void gauge_force_grid(const Geometry& g, Comm* comm, const double* dU, double beta, double c1, double coeff, int accumulate, double* force_dev, double* slots,
                      GaugeMdWork& w, hipStream_t st) {
  const ExtendedLinks& x = extended(w, g, comm, gauge_depth(c1 != 0.0), dU, st);
  force_of(x.shell, x.Ue.get(), beta, c1, coeff, accumulate, force_dev, slots, st);
}

void links_update(size_t V, double* dU, const double* dP, double eps, hipStream_t st) {
  hipLaunchKernelGGL(links_update_kernel, dim3((unsigned)((4 * V + 255) / 256)), dim3(256), 0, st, dU, dP, eps, 4 * V);
  DDAMG_HIP_CHECK(hipGetLastError());
}

void links_reunitarize(size_t V, double* dU, double* max_deviation, GaugeMdWork& w, hipStream_t st) {
  const size_t blocks = (4 * V + gmd::REDUCE_THREADS - 1) / gmd::REDUCE_THREADS;
  double* part = max_deviation ? parts(w, blocks) : nullptr;
  hipLaunchKernelGGL(links_reunitarize_kernel, dim3((unsigned)blocks), dim3(gmd::REDUCE_THREADS), 0, st, dU, 4 * V, part);
  DDAMG_HIP_CHECK(hipGetLastError());
  if (max_deviation) reduce_to_host<true>(part, blocks, 1, max_deviation, st);
}

void momentum_update(size_t V, double* dP, const double* dF, double eps, hipStream_t st) {
  hipLaunchKernelGGL(momentum_update_kernel, dim3((unsigned)((72 * V + 255) / 256)), dim3(256), 0, st, dP, dF, eps, 72 * V);
  DDAMG_HIP_CHECK(hipGetLastError());
}

double momentum_kinetic(size_t V, const double* dP, GaugeMdWork& w, hipStream_t st) {
  const size_t per_block = (size_t)gmd::REDUCE_THREADS * gmd::KINETIC_BATCH, blocks = (72 * V + per_block - 1) / per_block;
  double* part = parts(w, blocks);
  hipLaunchKernelGGL(momentum_kinetic_kernel, dim3((unsigned)blocks), dim3(gmd::REDUCE_THREADS), 0, st, part, dP, 72 * V);
  DDAMG_HIP_CHECK(hipGetLastError());
  double sum = 0.0;
  reduce_to_host<false>(part, blocks, 1, &sum, st);
  return 0.5 * sum;
}

}  // namespace ddamg
