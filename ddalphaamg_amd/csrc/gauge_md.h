// gauge_md.h -- the bodies of the kernels of the gauge sector of the molecular dynamics (gauge_md.hip: gauge_loops_kernel,
// gauge_force_kernel, gauge_force_assemble_kernel, links_update_kernel, links_reunitarize_kernel, momentum_update_kernel,
// momentum_kinetic_kernel, reduce_partials_kernel), and the host interface of gauge_md.hip.  Definitions: include/ddamg_hip.h
// ("Gauge sector").  Everything is fp64; every output is written by exactly one thread and every sum is taken in a fixed order,
// so two calls give the same bits.
//
// Links U are the caller's, lexicographic [V][4][18], without the anti-periodic sign: a closed loop crosses the time boundary an
// even number of times.  Varying U_mu(x) -> exp(eps Omega) U_mu(x), the action changes by  sum Re tr(Omega M_mu(x)),
//   M_mu(x) = -(beta/3) U_mu(x) [c0 sum(plaquette staples) + c1 sum(rectangle staples)],      c0 = 1 - 8 c1,
// and the force is TA(M).  A staple is the rest of a closed loop that starts with the link: a path from x + mu back to x.
//
// The force is taken plane by plane, as clover_derivative_kernel (force.h) takes the clover part: one workgroup = one wave = an
// 8 x 8 tile of sites of ONE plane (mu, nu), both directions of the plane staged in LDS once, every thread the plane's part of the
// two links its site owns: per link 2 plaquette staples and 6 rectangle staples (the nu-long rectangle, the mu-long one with the
// link first, the mu-long one with the link second, each above and below), 6 + 18 over a link's three planes.  The anti-Hermitian
// part goes, in the 9-real packing of force.h, into the link's slot of that plane (force::plane_slot; the layout of ForceWork::slots,
// whose hopping slot stays unused); force::site_assemble sums the three slots, removes the trace and writes coeff * G.
//
// The staged neighbourhood is H sites deep (Nb<H>): H = 1 for the plaquette, (8+2)^2 sites as field_strength.h, 30 KB; H = 2 with
// rectangles, whose staples reach from -2 to +2 across and from -1 to +2 along the link: (8+4)^2 sites x 2 directions x 19 doubles
// = 43 KB.  With c1 == 0 the H = 1 kernel runs and no rectangle is touched.
//
// The bodies are plain functions of (workgroup, thread) or of an index, so that a host program can run them thread by thread
// (tests/native/gauge_md_check.cpp does).
#pragma once
#include "force.h"
#include <cmath>

namespace ddamg {
namespace gmd {

using fs::cplx;
using fs::M3;

// the plane tile with its neighbourhood H sites deep
template <int H> struct Nb {
  static constexpr int EXT = fs::TILE + 2 * H;
  static constexpr int NEXT = EXT * EXT;
  static constexpr int LDS_DOUBLES = 2 * NEXT * fs::PITCH;
};

// step 1, threads 0 .. 2 EXT - 1: lexicographic site offset of every mu row (entries 0 .. EXT - 1) and nu column (EXT .. 2 EXT - 1)
// of the staged neighbourhood, periodic -- on a lattice smaller than the neighbourhood it wraps onto itself, more than once if need be
//
// On a process grid the links are those of the lattice extended by the neighbours' links H sites deep (fs::Shell of depth H; t:
// fs::extended_tile, whose strides and outside offset are the extended array's).  A split direction (s.h[d] = H) is addressed without
// wrap, coordinate c in [-H, L + H) at c + H; rows of a tile tail beyond L + H - 1, which no site of the lattice reads, are clamped
// to the last one.  An unsplit direction (s.h[d] = 0) wraps as above.  An undivided lattice is the shell with h = 0 everywhere and the
// lattice's own tile: the kernels of gauge_md.hip run this one form for both, so that a grid and the undivided lattice give the
// same bits.
template <int H>
DDAMG_FS_HD void stage_offsets(const fs::Planes& g, const fs::Tile& t, const fs::Shell& s, int tid, size_t* off) {
  constexpr int EXT = Nb<H>::EXT;
  if (tid >= 2 * EXT) return;
  const bool row = tid < EXT;
  const int i = row ? tid : tid - EXT;
  const int d = row ? t.mu : t.nu;
  const int Ld = g.L[d], h = s.h[d];
  int c = (row ? t.a0 : t.b0) + i - H;
  if (h) { c = c < -h ? -h : (c > Ld + h - 1 ? Ld + h - 1 : c); c += h; }
  else c = (c % Ld + Ld) % Ld;
  off[tid] = (size_t)c * (row ? t.smu : t.snu);
}
// the undivided lattice, t its own tile
template <int H>
DDAMG_FS_HD void stage_offsets(const fs::Planes& g, const fs::Tile& t, int tid, size_t* off) {
  const fs::Shell none{};
  stage_offsets<H>(g, t, none, tid, off);
}

// step 2, all threads: the links of both directions into LDS, lds[(w * NEXT + i * EXT + j) * PITCH + k], w = 0: U_mu, 1: U_nu;
// consecutive threads read consecutive reals of the caller's array (fs::stage_links at depth H)
template <int H>
DDAMG_FS_HD void stage_links(const double* __restrict__ U, const fs::Tile& t, int tid, const size_t* off, double* lds) {
  constexpr int EXT = Nb<H>::EXT, NEXT = Nb<H>::NEXT;
  constexpr int TOTAL = 2 * NEXT * 18, BATCH = 8;   // BATCH loads in flight per thread before the first store
  for (int k0 = 0; k0 < TOTAL; k0 += fs::THREADS * BATCH) {
    double v[BATCH]; int dst[BATCH];
#pragma unroll
    for (int u = 0; u < BATCH; u++) {
      const int k = k0 + u * fs::THREADS + tid;
      dst[u] = -1; v[u] = 0.0;
      if (k < TOTAL) {
        const int w = k / (NEXT * 18), rem = k - w * (NEXT * 18);
        const int e = rem / 18, comp = rem - e * 18;
        const int i = e / EXT, j = e - i * EXT;
        const size_t lx = t.outside + off[i] + off[EXT + j];
        v[u] = U[(lx * 4 + (w ? t.nu : t.mu)) * 18 + comp];
        dst[u] = (w * NEXT + e) * fs::PITCH + comp;
      }
    }
#pragma unroll
    for (int u = 0; u < BATCH; u++) if (dst[u] >= 0) lds[dst[u]] = v[u];
  }
}

template <int H>
DDAMG_FS_HD M3 staged(const double* lds, int w, int e) {
  M3 m; const double* p = lds + (w * Nb<H>::NEXT + e) * fs::PITCH;
#pragma unroll
  for (int k = 0; k < 9; k++) m.a[k] = cplx{p[2 * k], p[2 * k + 1]};
  return m;
}

// Paths in the plane, relative to a link direction a (0: mu, 1: nu) and the plane's other direction b = 1 - a: two bits per step,
// 0: +a, 1: -a, 2: +b, 3: -b, the first step in the lowest bits.  `below` mirrors the path in b.
constexpr unsigned pack_path(int s0, int s1, int s2, int s3 = 0, int s4 = 0, int s5 = 0) {
  return (unsigned)(s0 | (s1 << 2) | (s2 << 4) | (s3 << 6) | (s4 << 8) | (s5 << 10));
}
// the ordered product of the links along `len` steps of `path` from the staged site pos: a step forward gives the link it walks
// over, a step backward that link's dagger
template <int H>
DDAMG_FS_HD M3 path_product(const double* lds, int a, unsigned path, int len, bool below, int pos) {
  M3 out;
  for (int k = 0; k < len; k++) {
    int s = (int)((path >> (2 * k)) & 3u);
    if (below && (s & 2)) s ^= 1;
    const int w = (s & 2) ? 1 - a : a;
    const int d = w ? 1 : Nb<H>::EXT;
    M3 m;
    if (s & 1) { pos -= d; m = fs::dag(staged<H>(lds, w, pos)); }
    else { m = staged<H>(lds, w, pos); pos += d; }
    out = k == 0 ? m : fs::mul(out, m);
  }
  return out;
}

// the staples of the link U_a(x), paths from x + a back to x, above; the plaquette staple has three steps, the others five
constexpr unsigned STAPLE_PLAQUETTE = pack_path(2, 1, 3);
constexpr unsigned STAPLE_B_LONG = pack_path(2, 2, 1, 3, 3);          // the b-long rectangle
constexpr unsigned STAPLE_A_LONG_FIRST = pack_path(0, 2, 1, 1, 3);    // the a-long one, the link first
constexpr unsigned STAPLE_A_LONG_SECOND = pack_path(2, 1, 1, 3, 0);   // the a-long one, the link second
DDAMG_FS_HD unsigned staple_path(int k) { return k == 0 ? STAPLE_PLAQUETTE : k == 1 ? STAPLE_B_LONG : k == 2 ? STAPLE_A_LONG_FIRST : STAPLE_A_LONG_SECOND; }
// the closed loops from x: the plaquette and the rectangle two steps along a and one along b
constexpr unsigned LOOP_PLAQUETTE = pack_path(0, 2, 1, 3);
constexpr unsigned LOOP_RECTANGLE = pack_path(0, 0, 2, 1, 1, 3);

DDAMG_FS_HD double re_trace(const M3& m) { return m.a[0].r + m.a[4].r + m.a[8].r; }

// gauge_force_kernel, step 3, one thread per site of the tile: the plane's part of M for the two links the site owns
// (out[0]: U_mu(x), out[1]: U_nu(x)), anti-Hermitian part in 9 reals each.  H = 1: plaquette staples only, times c0; H = 2: and the
// rectangle staples times c1.  Returns false for a thread outside the lattice (tile tail).
template <int H>
DDAMG_FS_HD bool site_gauge_force(const fs::Planes& g, const fs::Tile& t, int tid, const double* lds, double beta, double c0, double c1, size_t* lex,
                                  double (&out)[2][9]) {
  const int ta = tid / fs::TILE, tb = tid - ta * fs::TILE;
  if (t.a0 + ta >= g.L[t.mu] || t.b0 + tb >= g.L[t.nu]) return false;
  *lex = t.outside + (size_t)(t.a0 + ta) * t.smu + (size_t)(t.b0 + tb) * t.snu;
  const int x = (ta + H) * Nb<H>::EXT + (tb + H);
#pragma unroll 1
  for (int a = 0; a < 2; a++) {   // one link at a time: the registers of one
    const int start = x + (a ? 1 : Nb<H>::EXT);
    M3 sum;
#pragma unroll
    for (int q = 0; q < 9; q++) sum.a[q] = cplx{0.0, 0.0};
#pragma unroll 1
    for (int k = 0; k < (H == 2 ? 4 : 1); k++) {
      const double weight = k == 0 ? c0 : c1;
      const unsigned path = staple_path(k);
#pragma unroll 1
      for (int below = 0; below < 2; below++) {
        const M3 s = path_product<H>(lds, a, path, k == 0 ? 3 : 5, below != 0, start);
#pragma unroll
        for (int q = 0; q < 9; q++) { sum.a[q].r += weight * s.a[q].r; sum.a[q].i += weight * s.a[q].i; }
      }
    }
    const M3 m = fs::mul(staged<H>(lds, a, x), sum);
    double o9[9];
    force::pack_antihermitian(m, -beta / 3.0, o9);
#pragma unroll
    for (int r = 0; r < 9; r++) { if (a == 0) out[0][r] = o9[r]; else out[1][r] = o9[r]; }   // constant indices: registers
  }
  return true;
}

// gauge_loops_kernel, step 3, one thread per site of the tile: Re tr P_mu_nu(x), and with H = 2 Re tr R_mu_nu(x) + Re tr R_nu_mu(x).
// A thread outside the lattice (tile tail) contributes zeros.
template <int H>
DDAMG_FS_HD void site_gauge_loops(const fs::Planes& g, const fs::Tile& t, int tid, const double* lds, double* plaq, double* rect) {
  *plaq = 0.0; *rect = 0.0;
  const int ta = tid / fs::TILE, tb = tid - ta * fs::TILE;
  if (t.a0 + ta >= g.L[t.mu] || t.b0 + tb >= g.L[t.nu]) return;
  const int x = (ta + H) * Nb<H>::EXT + (tb + H);
  *plaq = re_trace(path_product<H>(lds, 0, LOOP_PLAQUETTE, 4, false, x));
  if (H == 2) *rect = re_trace(path_product<H>(lds, 0, LOOP_RECTANGLE, 6, false, x)) + re_trace(path_product<H>(lds, 1, LOOP_RECTANGLE, 6, false, x));
}

DDAMG_FS_HD M3 load_matrix(const double* __restrict__ p) {
  M3 m;
#pragma unroll
  for (int k = 0; k < 9; k++) m.a[k] = cplx{p[2 * k], p[2 * k + 1]};
  return m;
}
DDAMG_FS_HD void store_matrix(double* __restrict__ p, const M3& m) {
#pragma unroll
  for (int k = 0; k < 9; k++) { p[2 * k] = m.a[k].r; p[2 * k + 1] = m.a[k].i; }
}

// exp(a) by scaling and squaring: a / 2^s of Frobenius norm at most one (a power of two: exact), its Taylor series to degree 18 by
// Horner's rule (the remainder of a matrix of spectral radius sqrt(2/3) is 3e-19), squared s times.  Every squaring doubles the
// error behind it and adds its own rounding, so exp of norm 10 (s = 4) carries some 16 roundings: fp64 rounding, far below 1e-13.
// A vanishing or tiny argument and degenerate eigenvalues are no special cases of a series.  A norm that is not finite gives a
// matrix that is not finite: s is capped.
constexpr int EXP_DEGREE = 18;
DDAMG_FS_HD M3 exp_matrix(M3 a) {
  double n2 = 0.0;
#pragma unroll
  for (int k = 0; k < 9; k++) n2 += a.a[k].r * a.a[k].r + a.a[k].i * a.a[k].i;
  int s = 0; double scale = 1.0;
  while (n2 * scale * scale > 1.0 && s < 64) { scale *= 0.5; s++; }
#pragma unroll
  for (int k = 0; k < 9; k++) { a.a[k].r *= scale; a.a[k].i *= scale; }
  M3 out;
#pragma unroll
  for (int k = 0; k < 9; k++) out.a[k] = cplx{(k % 4 == 0) ? 1.0 : 0.0, 0.0};
#pragma unroll 1
  for (int d = EXP_DEGREE; d >= 1; d--) {     // 1 + a/1 (1 + a/2 (1 + ... (1 + a/DEGREE)))
    const M3 t = fs::mul(a, out);
    const double f = 1.0 / (double)d;
#pragma unroll
    for (int k = 0; k < 9; k++) out.a[k] = cplx{((k % 4 == 0) ? 1.0 : 0.0) + f * t.a[k].r, f * t.a[k].i};
  }
#pragma unroll 1
  for (int k = 0; k < s; k++) out = fs::mul(out, out);
  return out;
}

// links_update_kernel, thread i of 4 V: U <- exp(eps P) U for link i
DDAMG_FS_HD void link_update(double* __restrict__ U, const double* __restrict__ P, double eps, size_t nlinks, size_t i) {
  if (i >= nlinks) return;
  M3 p = load_matrix(P + i * 18);
#pragma unroll
  for (int k = 0; k < 9; k++) { p.a[k].r *= eps; p.a[k].i *= eps; }
  store_matrix(U + i * 18, fs::mul(exp_matrix(p), load_matrix(U + i * 18)));
}

// links_reunitarize_kernel, thread i of 4 V: row 0 normalised, row 1 orthogonalised against row 0 and normalised, row 2 =
// conj(row 0 x row 1).  Returns max |U U^dagger - 1| of the link before the projection (0 for a thread beyond the last link)
DDAMG_FS_HD double link_reunitarize(double* __restrict__ U, size_t nlinks, size_t i) {
  if (i >= nlinks) return 0.0;
  M3 u = load_matrix(U + i * 18);
  const M3 uu = fs::mul(u, fs::dag(u));
  double dev = 0.0;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const double re = uu.a[k].r - ((k % 4 == 0) ? 1.0 : 0.0), im = uu.a[k].i;
    const double d = sqrt(re * re + im * im);
    dev = d > dev ? d : dev;
  }
  double n0 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) n0 += u.a[k].r * u.a[k].r + u.a[k].i * u.a[k].i;
  n0 = sqrt(n0);
#pragma unroll
  for (int k = 0; k < 3; k++) { u.a[k].r /= n0; u.a[k].i /= n0; }     // divisions: one rounding per entry, the rows' norms within 2 eps of one
  cplx dot{0.0, 0.0};     // <row 0, row 1>
#pragma unroll
  for (int k = 0; k < 3; k++) {
    dot.r += u.a[k].r * u.a[3 + k].r + u.a[k].i * u.a[3 + k].i;
    dot.i += u.a[k].r * u.a[3 + k].i - u.a[k].i * u.a[3 + k].r;
  }
  double n1 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    u.a[3 + k].r -= dot.r * u.a[k].r - dot.i * u.a[k].i;
    u.a[3 + k].i -= dot.r * u.a[k].i + dot.i * u.a[k].r;
    n1 += u.a[3 + k].r * u.a[3 + k].r + u.a[3 + k].i * u.a[3 + k].i;
  }
  n1 = sqrt(n1);
#pragma unroll
  for (int k = 0; k < 3; k++) { u.a[3 + k].r /= n1; u.a[3 + k].i /= n1; }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const cplx p = u.a[(k + 1) % 3], q = u.a[3 + (k + 2) % 3], r = u.a[(k + 2) % 3], s = u.a[3 + (k + 1) % 3];
    // conj(p q - r s)
    u.a[6 + k] = cplx{(p.r * q.r - p.i * q.i) - (r.r * s.r - r.i * s.i), -((p.r * q.i + p.i * q.r) - (r.r * s.i + r.i * s.r))};
  }
  store_matrix(U + i * 18, u);
  return dev;
}

// momentum_update_kernel, thread i of 72 V: one real, P <- P + eps F
DDAMG_FS_HD void momentum_update(double* __restrict__ P, const double* __restrict__ F, double eps, size_t n, size_t i) {
  if (i >= n) return;
  P[i] += eps * F[i];
}

// momentum_kinetic_kernel: workgroup `block` of REDUCE_THREADS threads takes REDUCE_THREADS * KINETIC_BATCH consecutive reals,
// thread tid every REDUCE_THREADS-th of them: its part of sum P[i]^2
constexpr int REDUCE_THREADS = 256;
constexpr int KINETIC_BATCH = 8;
DDAMG_FS_HD double kinetic_part(const double* __restrict__ P, size_t n, size_t block, int tid) {
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < KINETIC_BATCH; u++) {
    const size_t i = (block * KINETIC_BATCH + u) * REDUCE_THREADS + tid;
    if (i < n) s += P[i] * P[i];
  }
  return s;
}

}  // namespace gmd
}  // namespace ddamg

#if defined(__HIPCC__)
#include "common.h"
#include "extended_links.h"
#include <memory>
namespace ddamg {
// work space of the gauge sector, in the context from the first call on: the workgroups' partial sums and two results.  The plane
// slots of the force are ForceWork::slots.  From the first _grid call of a depth on a process grid on: the lattice extended by the
// neighbours' links at that depth and its two slab buffers (extended[depth - 1]), reused by every later call.
struct GaugeMdWork {
  DeviceBuffer<double> part;
  std::unique_ptr<ExtendedLinks> extended[2];
};
// how deep the staged neighbourhood, and on a process grid the shell, of an action is: 1 without rectangles, else 2
inline int gauge_depth(bool rectangles) { return rectangles ? 2 : 1; }
// sum_x sum_{mu<nu} Re tr P and (rect != nullptr) sum_x sum_{mu!=nu} Re tr R of the links dU; waits for the stream
void gauge_loops(const int L[4], const double* dU, double* plaq, double* rect, GaugeMdWork& w, hipStream_t st);
// force_dev (+)= coeff * G of the gauge action (beta, c1); slots: 4 * force::SLOTS * 9 * V reals
void gauge_force(const int L[4], const double* dU, double beta, double c1, double coeff, int accumulate, double* force_dev, double* slots, hipStream_t st);
// the same two on a process grid, collective: the caller's links of the own lattice go into the extended array of the action's
// depth, the shell arrives (two messages per split direction), and the same kernels run on it.  The sums are this process's; the
// caller adds them over the grid (comm_allreduce_host).
void gauge_loops_grid(const Geometry& g, Comm* comm, const double* dU, double* plaq, double* rect, GaugeMdWork& w, hipStream_t st);
void gauge_force_grid(const Geometry& g, Comm* comm, const double* dU, double beta, double c1, double coeff, int accumulate, double* force_dev, double* slots,
                      GaugeMdWork& w, hipStream_t st);
void links_update(size_t V, double* dU, const double* dP, double eps, hipStream_t st);
// max_deviation != nullptr: the largest |U U^dagger - 1| before the projection; waits for the stream then
void links_reunitarize(size_t V, double* dU, double* max_deviation, GaugeMdWork& w, hipStream_t st);
void momentum_update(size_t V, double* dP, const double* dF, double eps, hipStream_t st);
double momentum_kinetic(size_t V, const double* dP, GaugeMdWork& w, hipStream_t st);     // waits for the stream
}  // namespace ddamg
#endif
