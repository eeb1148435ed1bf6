// force.hip -- the derivative of the operator that is set with respect to its links (ddamg_hip_force_*): kernels around the
// bodies of force.h.  Launch order of one call:
//   force_links_kernel                       W = 2 D of the fp64 operator, lexicographic (nothing is read from the caller's links)
//   force_tensor_kernel / force_inverse_tensor_kernel    A_p per site and plane (+ the hopping part of the four own links)
//   clover_derivative_kernel                 per plane tile: the plane's part of the two links every site owns (csw != 0 only)
//   force_assemble_kernel                    sum of the slots, traceless part, times coeff into the caller's array
// Many pairs (force_multi_*): force_planes_multi_kernel + force_hop_multi_kernel per group of force::GROUP pairs in place of
// force_tensor_kernel; everything else once.
// No atomics and no reduction: every number is written by one thread.
// On a process grid (force_bilinear_grid / force_logdet_grid) the same kernels in their GRID / EXTENDED forms, and between them:
//   face_spinor_pack_kernel + one message per split direction     X and Y of the face x_mu = 0 to the - mu neighbour (bilinear)
//   ExtendedLinks::fill                                            W into the extended array, its shell from the neighbours
//   tensor_slab_pack_kernel / _unpack_kernel + two messages per split direction     the shell of A, behind the tensor kernel
#include "common.h"
#include "force.h"
#include <algorithm>
#include <vector>

namespace ddamg {

namespace {
// one thread per (site, direction): the 18 reals of D_mu(s), chunked SoA, times 2 into W[lex][mu][18]
__global__ __launch_bounds__(256) void force_links_kernel(double* __restrict__ W, const double* __restrict__ D, const int* __restrict__ lex, size_t V) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 4 * V) return;
  const size_t mu = i / V, s = i - mu * V;
  double* o = W + ((size_t)lex[s] * 4 + mu) * 18;
#pragma unroll
  for (int r = 0; r < 18; r++) o[r] = 2.0 * D[mu * 18 * V + force::soa2(V, s, r)];
}

__global__ __launch_bounds__(128) void force_tensor_kernel(force::Sites g, force::Gammas gm, const double* __restrict__ X, const double* __restrict__ Y,
                                                           const double* __restrict__ W, int clover, double* __restrict__ A, double* __restrict__ slots) {
  force::site_force_tensor(g, gm, X, Y, W, clover, A, slots, (size_t)blockIdx.x * 128 + threadIdx.x);
}
// on a process grid: A is the extended array, X and Y at x + mu come from the neighbour's face where the site has none of its own
__global__ __launch_bounds__(128) void force_tensor_grid_kernel(force::Sites g, force::Gammas gm, const double* __restrict__ X, const double* __restrict__ Y,
                                                                const double* __restrict__ W, int clover, double* __restrict__ A, double* __restrict__ slots,
                                                                force::Grid gr) {
  force::site_force_tensor<true>(g, gm, X, Y, W, clover, A, slots, (size_t)blockIdx.x * 128 + threadIdx.x, &gr);
}

// the tensor stage for a group of pairs (force.h): the six planes of a site, and the hopping part of one link per thread, y = mu
// grid != 0: on a process grid (gr).  One kernel for both, so that both give the same bits
__global__ __launch_bounds__(128) void force_planes_multi_kernel(force::Sites g, force::Gammas gm, force::Pairs pr, double* __restrict__ A, int grid,
                                                                 force::Grid gr) {
  force::site_planes_multi(g, gm, pr, A, (size_t)blockIdx.x * 128 + threadIdx.x, grid != 0, &gr);
}
__global__ __launch_bounds__(128) void force_hop_multi_kernel(force::Sites g, force::Gammas gm, force::Pairs pr, const double* __restrict__ W,
                                                              double* __restrict__ slots, int grid, force::Grid gr) {
  force::site_hop_multi(g, gm, pr, W, slots, (size_t)blockIdx.x * 128 + threadIdx.x, (int)blockIdx.y, grid != 0, &gr);
}
// y = the pair of the group: its X and Y of the face, 48 F doubles, behind those of the pairs before it
__global__ __launch_bounds__(256) void face_spinor_pack_multi_kernel(double* __restrict__ buf, force::Pairs pr, size_t V, const int* __restrict__ sites, size_t F) {
  const int k = blockIdx.y;
  force::face_spinor_pack(pr.x[k], pr.y[k], V, sites, F, buf + (size_t)k * 48 * F, (size_t)blockIdx.x * 256 + threadIdx.x);
}

// EXTENDED: A is the extended array of `shell`
template <bool EXTENDED>
__global__ __launch_bounds__(128) void force_inverse_tensor_kernel(force::Sites g, force::Gammas gm, const double* __restrict__ clover_inv, int par,
                                                                   double* __restrict__ A, fs::Shell shell) {
  force::site_inverse_tensor(g, gm, clover_inv, par, A, (size_t)blockIdx.x * 128 + threadIdx.x, EXTENDED ? &shell : nullptr);
}

// one real of a slab of the extended A into a contiguous buffer, and a received buffer into the slab one site further out
__global__ __launch_bounds__(256) void tensor_slab_pack_kernel(double* __restrict__ buf, double* __restrict__ A, fs::Shell shell, fs::Slab slab) {
  force::tensor_slab_copy(shell, slab, A, buf, (size_t)blockIdx.x * 256 + threadIdx.x, true);
}
__global__ __launch_bounds__(256) void tensor_slab_unpack_kernel(double* __restrict__ A, double* __restrict__ buf, fs::Shell shell, fs::Slab slab) {
  force::tensor_slab_copy(shell, slab, A, buf, (size_t)blockIdx.x * 256 + threadIdx.x, false);
}
__global__ __launch_bounds__(256) void face_spinor_pack_kernel(double* __restrict__ buf, const double* __restrict__ X, const double* __restrict__ Y, size_t V,
                                                               const int* __restrict__ sites, size_t F) {
  force::face_spinor_pack(X, Y, V, sites, F, buf, (size_t)blockIdx.x * 256 + threadIdx.x);
}

// grid: x = tiles, y = the six planes; one workgroup = one wave = an 8 x 8 tile (field_strength.h).
// EXTENDED: W and A are the lattice extended by the neighbours' shell; the tile, the output index and the slots stay those of the
// own lattice, as in field_strength_kernel<true>
template <bool EXTENDED>
__global__ __launch_bounds__(fs::THREADS) void clover_derivative_kernel(double* __restrict__ slots, const double* __restrict__ W, const double* __restrict__ A,
                                                                         fs::Planes g, size_t V, fs::Shell shell) {
  __shared__ double lds[fs::LDS_DOUBLES];
  __shared__ double lds_a[force::LDS_A_DOUBLES];
  __shared__ size_t off[2 * fs::EXT];
  __shared__ int flip[fs::EXT];
  const int p = blockIdx.y, block = blockIdx.x, tid = threadIdx.x;
  if (block >= g.nblocks[p]) return;
  const fs::Tile t = fs::tile_of(g, p, block);
  if constexpr (EXTENDED) {
    const fs::Tile te = fs::extended_tile(g, shell, t, block);
    fs::stage_offsets<true>(g, te, 0, tid, off, flip, &shell);
    __syncthreads();
    fs::stage_links(W, te, tid, off, flip, lds);
    force::stage_tensor(A, shell.Ve, p, te, tid, off, lds_a);
  } else {
    fs::stage_offsets(g, t, 0, tid, off, flip);     // the sign is in W
    __syncthreads();
    fs::stage_links(W, t, tid, off, flip, lds);
    force::stage_tensor(A, V, p, t, tid, off, lds_a);
  }
  __syncthreads();
  size_t lex = 0; double out[2][9];
  if (force::site_clover_derivative(g, t, tid, lds, lds_a, &lex, out)) {
    const int smu = t.mu * force::SLOTS + force::plane_slot(t.mu, t.nu), snu = t.nu * force::SLOTS + force::plane_slot(t.nu, t.mu);
#pragma unroll
    for (int r = 0; r < 9; r++) {
      slots[((size_t)smu * 9 + r) * V + lex] = out[0][r];
      slots[((size_t)snu * 9 + r) * V + lex] = out[1][r];
    }
  }
}

__global__ __launch_bounds__(128) void force_assemble_kernel(double* __restrict__ out, const double* __restrict__ slots, size_t V, int clover, int hop,
                                                             double coeff, int accumulate) {
  force::site_assemble(slots, V, (size_t)blockIdx.x * 128 + threadIdx.x, clover, hop, coeff, accumulate, out);
}

double* work(DeviceBuffer<double>& b, size_t n) {
  if (!b.get()) b.alloc(n);
  DDAMG_REQUIRE(b.bytes() == sizeof(double) * n, "force workspace of another lattice");
  return b.get();
}

force::Sites sites_of(const FineOp<double>& op, const int* lex, double csw, double scale_even, double scale_odd) {
  const FineOpDev<double> d = op.dev();
  DDAMG_REQUIRE(d.D != nullptr && d.nb != nullptr && d.parity != nullptr && lex != nullptr, "force: no operator uploaded");
  return force::Sites{(size_t)d.V, d.nb, lex, d.parity, csw, scale_even, scale_odd};
}

const double* export_links(const FineOp<double>& op, const force::Sites& g, ForceWork& w, hipStream_t st) {
  double* W = work(w.W, 72 * g.V);
  hipLaunchKernelGGL(force_links_kernel, dim3((unsigned)((4 * g.V + 255) / 256)), dim3(256), 0, st, W, op.dev().D, g.lex, g.V);
  DDAMG_HIP_CHECK(hipGetLastError());
  return W;
}

void clover_derivative(const int L[4], const double* W, const double* A, double* slots, size_t V, hipStream_t st) {
  const fs::Planes planes = fs::make_planes(L);
  hipLaunchKernelGGL(clover_derivative_kernel<false>, dim3((unsigned)planes.max_blocks, 6), dim3(fs::THREADS), 0, st, slots, W, A, planes, V, fs::Shell{});
  DDAMG_HIP_CHECK(hipGetLastError());
}
void clover_derivative_extended(const int L[4], const double* We, const double* Ae, const fs::Shell& shell, double* slots, size_t V, hipStream_t st) {
  const fs::Planes planes = fs::make_planes(L);
  hipLaunchKernelGGL(clover_derivative_kernel<true>, dim3((unsigned)planes.max_blocks, 6), dim3(fs::THREADS), 0, st, slots, We, Ae, planes, V, shell);
  DDAMG_HIP_CHECK(hipGetLastError());
}

// the extended arrays and the buffers of a process grid, at the first call
void grid_work(ForceWork& w, const Geometry& g, hipStream_t st) {
  if (w.links) return;
  w.links.reset(new ExtendedLinks(g));
  w.Ae.alloc(54 * w.links->shell.Ve);
  std::vector<int> sites;
  size_t most = 0;
  for (int mu = 0; mu < 4; mu++)
    if (g.split[mu]) { sites.insert(sites.end(), g.face_sites[4 + mu].begin(), g.face_sites[4 + mu].end()); most = std::max(most, (size_t)g.face_size(mu)); }
  w.face_sites.alloc(sites.size());
  DDAMG_HIP_CHECK(hipMemcpyAsync(w.face_sites, sites.data(), sizeof(int) * sites.size(), hipMemcpyHostToDevice, st));
  DDAMG_HIP_CHECK(hipStreamSynchronize(st));     // `sites` goes
  w.face_send.alloc(48 * most * force::GROUP);     // of a whole group of pairs (force_multi_group)
  w.face_recv.alloc(48 * sites.size() * force::GROUP);
}

// X and Y of the face x_mu = 0 to the - mu neighbour, those of the + mu neighbour's into w.face_recv: one message per split direction
force::Grid exchange_face_spinors(const Geometry& g, Comm* comm, const double* x, const double* y, ForceWork& w, hipStream_t st) {
  force::Grid gr;
  gr.shell = w.links->shell;
  size_t first = 0;     // face site of the direction in w.face_sites / w.face_recv
  for (int mu = 0; mu < 4; mu++) {
    gr.face[mu] = nullptr; gr.F[mu] = 0;
    if (!g.split[mu]) continue;
    const size_t F = (size_t)g.face_size(mu);
    double* recv = w.face_recv + 48 * first;
    gr.face[mu] = recv; gr.F[mu] = (int)F;
    hipLaunchKernelGGL(face_spinor_pack_kernel, dim3((unsigned)((24 * F + 255) / 256)), dim3(256), 0, st, w.face_send, x, y, (size_t)g.V,
                       w.face_sites + first, F);
    DDAMG_HIP_CHECK(hipGetLastError());
    comm_sendrecv_device(comm, w.face_send, g.neighbor_rank[4 + mu], recv, g.neighbor_rank[mu], sizeof(double) * 48 * F, 140 + mu, st);
    first += F;
  }
  return gr;
}

// the same for the pairs of a group: X then Y of every pair, one after the other, in ONE message per split direction
force::Grid exchange_face_spinors_multi(const Geometry& g, Comm* comm, const force::Pairs& pr, ForceWork& w, hipStream_t st) {
  force::Grid gr;
  gr.shell = w.links->shell;
  size_t first = 0;
  for (int mu = 0; mu < 4; mu++) {
    gr.face[mu] = nullptr; gr.F[mu] = 0;
    if (!g.split[mu]) continue;
    const size_t F = (size_t)g.face_size(mu);
    double* recv = w.face_recv + 48 * first * force::GROUP;
    gr.face[mu] = recv; gr.F[mu] = (int)F;
    hipLaunchKernelGGL(face_spinor_pack_multi_kernel, dim3((unsigned)((24 * F + 255) / 256), (unsigned)pr.n), dim3(256), 0, st, w.face_send.get(), pr,
                       (size_t)g.V, w.face_sites + first, F);
    DDAMG_HIP_CHECK(hipGetLastError());
    comm_sendrecv_device(comm, w.face_send, g.neighbor_rank[4 + mu], recv, g.neighbor_rank[mu], sizeof(double) * 48 * F * (size_t)pr.n, 140 + mu, st);
    first += F;
  }
  return gr;
}

// the shell of A behind the tensor kernel, by the slab scheme of ExtendedLinks::fill: two messages per split direction
void exchange_tensor_shell(const Geometry& g, Comm* comm, ForceWork& w, hipStream_t st) {
  const fs::Shell& shell = w.links->shell;
  double* sbuf = w.links->sbuf; double* rbuf = w.links->rbuf;
  for (int mu = 0; mu < 4; mu++) {
    if (!shell.h[mu]) continue;
    const fs::Slab slab = fs::make_slab(shell, mu);
    const unsigned blocks = (unsigned)((slab.sites * 54 + 255) / 256);
    for (int side = 0; side < 2; side++) {
      const int src_c = side == 0 ? shell.L[mu] - 1 : 0, dst_c = side == 0 ? -1 : shell.L[mu];
      hipLaunchKernelGGL(tensor_slab_pack_kernel, dim3(blocks), dim3(256), 0, st, sbuf, w.Ae.get(), shell, fs::slab_at(shell, slab, src_c));
      DDAMG_HIP_CHECK(hipGetLastError());
      comm_sendrecv_device(comm, sbuf, g.neighbor_rank[side == 0 ? mu : 4 + mu], rbuf, g.neighbor_rank[side == 0 ? 4 + mu : mu],
                           sizeof(double) * 54 * slab.sites, 120 + 2 * mu + side, st);
      hipLaunchKernelGGL(tensor_slab_unpack_kernel, dim3(blocks), dim3(256), 0, st, w.Ae.get(), rbuf, shell, fs::slab_at(shell, slab, dst_c));
      DDAMG_HIP_CHECK(hipGetLastError());
    }
  }
}

void assemble(double* force_dev, const double* slots, size_t V, bool clover, bool hop, double coeff, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(force_assemble_kernel, dim3((unsigned)((V + 127) / 128)), dim3(128), 0, st, force_dev, slots, V, (int)clover, (int)hop, coeff,
                     accumulate);
  DDAMG_HIP_CHECK(hipGetLastError());
}
}  // namespace

void force_bilinear(const FineOp<double>& op, const int L[4], const int* lex, double csw, double scale_even, double scale_odd, const double* y,
                    const double* x, double coeff, int accumulate, double* force_dev, ForceWork& w, hipStream_t st) {
  const force::Sites g = sites_of(op, lex, csw, scale_even, scale_odd);
  const bool clover = csw != 0.0;
  const double* W = export_links(op, g, w, st);
  double* A = clover ? work(w.A, 54 * g.V) : nullptr;
  double* slots = work(w.slots, (size_t)4 * force::SLOTS * 9 * g.V);
  hipLaunchKernelGGL(force_tensor_kernel, dim3((unsigned)((g.V + 127) / 128)), dim3(128), 0, st, g, force::make_gammas(), x, y, W, (int)clover, A, slots);
  DDAMG_HIP_CHECK(hipGetLastError());
  if (clover) clover_derivative(L, W, A, slots, g.V, st);
  assemble(force_dev, slots, g.V, clover, true, coeff, accumulate, st);
}

void force_logdet(const FineOp<double>& op, const int L[4], const int* lex, double csw, double scale_even, double scale_odd, int par, double coeff,
                  int accumulate, double* force_dev, ForceWork& w, hipStream_t st) {
  DDAMG_REQUIRE(par == 0 || par == 1, "parity must be 0 (even) or 1 (odd)");
  const force::Sites g = sites_of(op, lex, csw, scale_even, scale_odd);
  const bool clover = csw != 0.0;     // without a clover term C is a constant
  double* slots = work(w.slots, (size_t)4 * force::SLOTS * 9 * g.V);
  if (clover) {
    DDAMG_REQUIRE(op.dev().clover_inv != nullptr, "force: no operator uploaded");
    const double* W = export_links(op, g, w, st);
    double* A = work(w.A, 54 * g.V);
    hipLaunchKernelGGL(force_inverse_tensor_kernel<false>, dim3((unsigned)((g.V + 127) / 128)), dim3(128), 0, st, g, force::make_gammas(), op.dev().clover_inv,
                       par, A, fs::Shell{});
    DDAMG_HIP_CHECK(hipGetLastError());
    clover_derivative(L, W, A, slots, g.V, st);
  }
  assemble(force_dev, slots, g.V, clover, false, coeff, accumulate, st);
}

void force_bilinear_grid(const FineOp<double>& op, const Geometry& geom, Comm* comm, const int* lex, double csw, double scale_even, double scale_odd,
                         const double* y, const double* x, double coeff, int accumulate, double* force_dev, ForceWork& w, hipStream_t st) {
  DDAMG_REQUIRE(comm != nullptr, "the force on a process grid needs a transport");
  const force::Sites g = sites_of(op, lex, csw, scale_even, scale_odd);
  const bool clover = csw != 0.0;
  grid_work(w, geom, st);
  const double* W = export_links(op, g, w, st);      // the hopping part reads the own links only
  double* slots = work(w.slots, (size_t)4 * force::SLOTS * 9 * g.V);
  const force::Grid gr = exchange_face_spinors(geom, comm, x, y, w, st);
  if (clover) w.links->fill(geom, comm, W, 0, st);   // no sign: it is in W
  hipLaunchKernelGGL(force_tensor_grid_kernel, dim3((unsigned)((g.V + 127) / 128)), dim3(128), 0, st, g, force::make_gammas(), x, y, W, (int)clover,
                     clover ? w.Ae.get() : nullptr, slots, gr);
  DDAMG_HIP_CHECK(hipGetLastError());
  if (clover) {
    exchange_tensor_shell(geom, comm, w, st);
    clover_derivative_extended(geom.L, w.links->Ue, w.Ae, gr.shell, slots, g.V, st);
  }
  assemble(force_dev, slots, g.V, clover, true, coeff, accumulate, st);
}

ForceMulti force_multi_begin(const FineOp<double>& op, const Geometry& geom, Comm* comm, const int* lex, double csw, double scale_even, double scale_odd,
                             ForceWork& w, hipStream_t st) {
  ForceMulti m;
  m.sites = sites_of(op, lex, csw, scale_even, scale_odd);
  m.clover = csw != 0.0;
  m.distributed = geom.distributed();
  for (int mu = 0; mu < 4; mu++) { m.grid.face[mu] = nullptr; m.grid.F[mu] = 0; }
  m.grid.shell = fs::Shell{};
  if (m.distributed) {
    DDAMG_REQUIRE(comm != nullptr, "the force on a process grid needs a transport");
    grid_work(w, geom, st);
  }
  m.W = export_links(op, m.sites, w, st);
  m.slots = work(w.slots, (size_t)4 * force::SLOTS * 9 * m.sites.V);
  if (m.distributed) {
    if (m.clover) w.links->fill(geom, comm, m.W, 0, st);   // no sign: it is in W
    m.A = m.clover ? w.Ae.get() : nullptr;
  } else {
    m.A = m.clover ? work(w.A, 54 * m.sites.V) : nullptr;
  }
  return m;
}

void force_multi_group(ForceMulti& m, const Geometry& geom, Comm* comm, int n, const double* const* y, const double* const* x, const double* weights,
                       ForceWork& w, hipStream_t st) {
  DDAMG_REQUIRE(n >= 1 && n <= force::GROUP, "force_multi_group: 1 .. force::GROUP pairs");
  force::Pairs pr;
  for (int k = 0; k < force::GROUP; k++) { pr.x[k] = k < n ? x[k] : nullptr; pr.y[k] = k < n ? y[k] : nullptr; pr.w[k] = k < n ? weights[k] : 0.0; }
  pr.n = n; pr.add = m.groups > 0;
  const force::Sites& g = m.sites;
  const dim3 sites((unsigned)((g.V + 127) / 128)), links((unsigned)((g.V + 127) / 128), 4);
  const force::Gammas gm = force::make_gammas();
  if (m.distributed) m.grid = exchange_face_spinors_multi(geom, comm, pr, w, st);
  if (m.clover) hipLaunchKernelGGL(force_planes_multi_kernel, sites, dim3(128), 0, st, g, gm, pr, m.A, (int)m.distributed, m.grid);
  hipLaunchKernelGGL(force_hop_multi_kernel, links, dim3(128), 0, st, g, gm, pr, m.W, m.slots, (int)m.distributed, m.grid);
  DDAMG_HIP_CHECK(hipGetLastError());
  m.groups++;
}

void force_multi_end(ForceMulti& m, const Geometry& geom, Comm* comm, double coeff, int accumulate, double* force_dev, ForceWork& w, hipStream_t st) {
  DDAMG_REQUIRE(m.groups > 0, "force_multi_end: no group of pairs");
  if (m.clover) {
    if (m.distributed) {
      exchange_tensor_shell(geom, comm, w, st);
      clover_derivative_extended(geom.L, w.links->Ue, w.Ae, w.links->shell, m.slots, m.sites.V, st);
    } else {
      clover_derivative(geom.L, m.W, m.A, m.slots, m.sites.V, st);
    }
  }
  assemble(force_dev, m.slots, m.sites.V, m.clover, true, coeff, accumulate, st);
}

void force_logdet_grid(const FineOp<double>& op, const Geometry& geom, Comm* comm, const int* lex, double csw, double scale_even, double scale_odd, int par,
                       double coeff, int accumulate, double* force_dev, ForceWork& w, hipStream_t st) {
  DDAMG_REQUIRE(par == 0 || par == 1, "parity must be 0 (even) or 1 (odd)");
  DDAMG_REQUIRE(comm != nullptr, "the force on a process grid needs a transport");
  const force::Sites g = sites_of(op, lex, csw, scale_even, scale_odd);
  const bool clover = csw != 0.0;     // without a clover term C is a constant: nothing is sent
  double* slots = work(w.slots, (size_t)4 * force::SLOTS * 9 * g.V);
  if (clover) {
    DDAMG_REQUIRE(op.dev().clover_inv != nullptr, "force: no operator uploaded");
    grid_work(w, geom, st);
    const fs::Shell& shell = w.links->shell;
    w.links->fill(geom, comm, export_links(op, g, w, st), 0, st);
    hipLaunchKernelGGL(force_inverse_tensor_kernel<true>, dim3((unsigned)((g.V + 127) / 128)), dim3(128), 0, st, g, force::make_gammas(), op.dev().clover_inv,
                       par, w.Ae.get(), shell);
    DDAMG_HIP_CHECK(hipGetLastError());
    exchange_tensor_shell(geom, comm, w, st);
    clover_derivative_extended(geom.L, w.links->Ue, w.Ae, shell, slots, g.V, st);
  }
  assemble(force_dev, slots, g.V, clover, false, coeff, accumulate, st);
}

}  // namespace ddamg
