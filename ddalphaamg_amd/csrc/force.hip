// force.hip -- the derivative of the operator that is set with respect to its links (ddamg_hip_force_*): kernels around the
// bodies of force.h.  Launch order of one call:
//   force_links_kernel                       W = 2 D of the fp64 operator, lexicographic (nothing is read from the caller's links)
//   force_tensor_kernel / force_inverse_tensor_kernel    A_p per site and plane (+ the hopping part of the four own links)
//   clover_derivative_kernel                 per plane tile: the plane's part of the two links every site owns (csw != 0 only)
//   force_assemble_kernel                    sum of the slots, traceless part, times coeff into the caller's array
// No atomics and no reduction: every number is written by one thread.
#include "common.h"
#include "force.h"

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

__global__ __launch_bounds__(128) void force_inverse_tensor_kernel(force::Sites g, force::Gammas gm, const double* __restrict__ clover_inv, int par,
                                                                   double* __restrict__ A) {
  force::site_inverse_tensor(g, gm, clover_inv, par, A, (size_t)blockIdx.x * 128 + threadIdx.x);
}

// grid: x = tiles, y = the six planes; one workgroup = one wave = an 8 x 8 tile (field_strength.h)
__global__ __launch_bounds__(fs::THREADS) void clover_derivative_kernel(double* __restrict__ slots, const double* __restrict__ W, const double* __restrict__ A,
                                                                         fs::Planes g, size_t V) {
  __shared__ double lds[fs::LDS_DOUBLES];
  __shared__ double lds_a[force::LDS_A_DOUBLES];
  __shared__ size_t off[2 * fs::EXT];
  __shared__ int flip[fs::EXT];
  const int p = blockIdx.y, block = blockIdx.x, tid = threadIdx.x;
  if (block >= g.nblocks[p]) return;
  const fs::Tile t = fs::tile_of(g, p, block);
  fs::stage_offsets(g, t, 0, tid, off, flip);     // the sign is in W
  __syncthreads();
  fs::stage_links(W, t, tid, off, flip, lds);
  force::stage_tensor(A, V, p, t, tid, off, lds_a);
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
  hipLaunchKernelGGL(clover_derivative_kernel, dim3((unsigned)planes.max_blocks, 6), dim3(fs::THREADS), 0, st, slots, W, A, planes, V);
  DDAMG_HIP_CHECK(hipGetLastError());
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
    hipLaunchKernelGGL(force_inverse_tensor_kernel, dim3((unsigned)((g.V + 127) / 128)), dim3(128), 0, st, g, force::make_gammas(), op.dev().clover_inv, par, A);
    DDAMG_HIP_CHECK(hipGetLastError());
    clover_derivative(L, W, A, slots, g.V, st);
  }
  assemble(force_dev, slots, g.V, clover, false, coeff, accumulate, st);
}

}  // namespace ddamg
