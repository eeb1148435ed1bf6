// force.h -- the bodies of the kernels that differentiate the operator with respect to its links (force.hip:
// force_tensor_kernel, force_inverse_tensor_kernel, clover_derivative_kernel, force_assemble_kernel), and the host interface of
// force.hip.  Definitions: include/ddamg_hip.h ("Forces").  Everything is fp64; every output is written by exactly one thread, so
// two calls give the same bits.
//
// Links are W_mu(x) = 2 D_mu(x): what the operator stores, times 2, the anti-periodic sign included, lexicographic [V][4][18].
// Varying W_mu(x) -> exp(eps Omega) W_mu(x), a real function S changes by  sum Re tr(Omega M_mu(x)); its force is TA(M).  Only the
// anti-Hermitian part of M matters, so every stage keeps 9 reals per matrix in the packing field_strength.h uses for F (the
// imaginary parts of the diagonal, then (0,1), (0,2), (1,2)); force_assemble_kernel removes the trace.
//
// The clover part.  C(x) = s(x) [(4 + m0) - csw sum_p (gamma_mu gamma_nu) (x) F_p(x)], F = (Q - Q^dagger) / 16, Q the sum of the
// four leaves.  Both functions S (Re <Y, D X> and sum log|det C|) depend on F through  -csw s(x) Re tr_c[F_p(x) Lambda_p(x)]  with a
// site tensor Lambda, and  Re tr[(Q - Q^dagger) L] = Re tr[Q (L - L^dagger)], so what the derivative kernel reads is
//   A_p(x) = -csw s(x) / 8 * (Lambda_p(x) - Lambda_p(x)^dagger) / 2        (anti-Hermitian, 9 reals per site and plane)
// and the clover part of S is  sum_x sum_p Re tr[Q_p(x) A_p(x)].  A leaf is a closed path of four factors f0 f1 f2 f3 from its
// corner y; where the link W sits at position k,
//   as W:         tr[f0 .. (Omega W) .. f3 A] = tr[Omega R_k],       R_k = f_k .. f3 A(y) f0 .. f_{k-1}
//   as W^dagger:  tr[f0 .. (W^dagger (-Omega)) .. f3 A] = -tr[Omega R_{k+1}]
// Every link lies in two plaquettes of a plane and in four leaves of each: eight rotations R per link and plane, all of whose
// factors lie within one site of the link's own site.  clover_derivative_kernel is field_strength_kernel turned round: the same
// 8 x 8 tile of one plane per wave, the same staged (8+2)^2 neighbourhood of W_mu and W_nu, and next to it that of A_p.
//
// On a process grid (the ddamg_hip_force_*_grid calls) who writes what stays as it is; only where a boundary thread reads from
// changes: W and A live in arrays extended by a one-site shell of the neighbours' values in every split direction (fs::Shell), the
// derivative kernel stages its neighbourhood through fs::extended_tile / fs::stage_offsets<true> as field_strength_kernel<true> does,
// and the hopping part reads X and Y at x + mu from the face the + mu neighbour sent (Grid).
//
// The bodies are plain functions of (workgroup, thread) or of a site, so that a host program can run them thread by thread
// (tests/native/clover_force_check.cpp, force_shell_check.cpp and force_multi_check.cpp do).
#pragma once
#include "field_strength.h"

namespace ddamg {
namespace force {

using fs::cplx;
using fs::M3;

constexpr int APITCH = 9;                              // doubles per staged A: odd, as fs::PITCH
constexpr int LDS_A_DOUBLES = fs::NEXT * APITCH;
constexpr int SLOTS = 4;                               // per link: its three planes, then the hopping term
constexpr int HOP_SLOT = 3;

// gamma_mu (BASIS0 of the reference, src/clifford.h:39-100): row i has one entry, (re, im)[mu][i] in column col[mu][i]; and the
// products gamma_mu gamma_nu of the six planes as the clover term takes them (fs::GammaProducts)
struct Gammas {
  double re[4][4], im[4][4];
  fs::GammaProducts prod;
};
// col[mu][i]: {2, 3, 0, 1} for T and X, {3, 2, 1, 0} for Z and Y -- a function, so that it is a constant in unrolled device code
DDAMG_FS_HD int gamma_col(int mu, int i) { return i ^ ((mu == 0 || mu == 3) ? 2 : 3); }
inline Gammas make_gammas() {
  int col[4][4];
  for (int mu = 0; mu < 4; mu++) for (int i = 0; i < 4; i++) col[mu][i] = gamma_col(mu, i);
  static const double vre[4][4] = {{-1, -1, -1, -1}, {0, 0, 0, 0}, {-1, 1, 1, -1}, {0, 0, 0, 0}};
  static const double vim[4][4] = {{0, 0, 0, 0}, {-1, -1, 1, 1}, {0, 0, 0, 0}, {-1, 1, 1, -1}};
  Gammas g;
  for (int mu = 0; mu < 4; mu++)
    for (int i = 0; i < 4; i++) { g.re[mu][i] = vre[mu][i]; g.im[mu][i] = vim[mu][i]; }
  for (int p = 0; p < 6; p++) {
    const int mu = fs::plane_mu(p), nu = fs::plane_nu(p);
    for (int k = 0; k < 16; k++) { g.prod.re[p][k] = 0; g.prod.im[p][k] = 0; }
    for (int i = 0; i < 4; i++) {
      const int c = col[mu][i], j = col[nu][c];
      g.prod.re[p][4 * i + j] = vre[mu][i] * vre[nu][c] - vim[mu][i] * vim[nu][c];
      g.prod.im[p][4 * i + j] = vre[mu][i] * vim[nu][c] + vim[mu][i] * vre[nu][c];
    }
  }
  return g;
}

// what the site kernels read: fields of the fp64 operator in the device's site order (chunked SoA, common.h) and its tables
struct Sites {
  size_t V;
  const int* nb;                 // [8][V] neighbour sites (fine_op.h); only + mu is read
  const int* lex;                // [V] lexicographic index of every site
  const unsigned char* parity;   // [V]
  double csw, scale_even, scale_odd;
};

// what the site kernels of the ddamg_hip_force_*_grid calls need besides: the extended array A goes into (fs::Shell), and for every
// split direction mu the spinors the + mu neighbour sent from its face x_mu = 0: X then Y, each a chunked-SoA fp64 field of F[mu]
// face sites in slot order (geometry.h); a site with x_mu = L - 1 finds its slot as -1 - nb there
struct Grid {
  fs::Shell shell;
  const double* face[4];
  int F[4];
};

// real r of site s of a chunked-SoA fp64 field
DDAMG_FS_HD size_t soa2(size_t V, size_t s, int r) { return ((size_t)(r >> 1) * V + s) * 2 + (r & 1); }

DDAMG_FS_HD void load_spinor(const double* __restrict__ v, size_t V, size_t s, cplx (&out)[12]) {
#pragma unroll
  for (int k = 0; k < 12; k++) out[k] = cplx{v[soa2(V, s, 2 * k)], v[soa2(V, s, 2 * k + 1)]};
}

// the anti-Hermitian part (M - M^dagger) / 2 of a matrix, times f, in 9 reals
DDAMG_FS_HD void pack_antihermitian(const M3& m, double f, double (&out)[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++) out[i] = f * m.a[4 * i].i;
  int k = 3;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = i + 1; j < 3; j++, k += 2) {
      out[k] = f * 0.5 * (m.a[3 * i + j].r - m.a[3 * j + i].r);
      out[k + 1] = f * 0.5 * (m.a[3 * i + j].i + m.a[3 * j + i].i);
    }
}
DDAMG_FS_HD M3 unpack_antihermitian(const double* f) {
  M3 m;
  m.a[0] = cplx{0.0, f[0]}; m.a[4] = cplx{0.0, f[1]}; m.a[8] = cplx{0.0, f[2]};
  m.a[1] = cplx{f[3], f[4]}; m.a[3] = cplx{-f[3], f[4]};
  m.a[2] = cplx{f[5], f[6]}; m.a[6] = cplx{-f[5], f[6]};
  m.a[5] = cplx{f[7], f[8]}; m.a[7] = cplx{-f[7], f[8]};
  return m;
}

DDAMG_FS_HD M3 load_link(const double* __restrict__ W, size_t lx, int mu) {
  M3 m; const double* p = W + (lx * 4 + mu) * 18;
#pragma unroll
  for (int k = 0; k < 9; k++) m.a[k] = cplx{p[2 * k], p[2 * k + 1]};
  return m;
}

// out[c][a] += g * x[sx][c] conj(y[sy][a]) for spin components sx of x and sy of y
DDAMG_FS_HD void add_outer(M3& out, cplx g, const cplx (&x)[12], int sx, const cplx (&y)[12], int sy) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const cplx gx{g.r * x[3 * sx + c].r - g.i * x[3 * sx + c].i, g.r * x[3 * sx + c].i + g.i * x[3 * sx + c].r};
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const cplx w = y[3 * sy + a];
      out.a[3 * c + a].r += gx.r * w.r + gx.i * w.i;
      out.a[3 * c + a].i += gx.i * w.r - gx.r * w.i;
    }
  }
}

// force_tensor_kernel, one thread per site s (device order): A_p of the bilinear function for the six planes,
//   Lambda_p(x)[b][a] = sum_{s,s'} (gamma_mu gamma_nu)[s][s'] X[s'][b](x) conj(Y[s][a](x)),
// A[(p * 9 + r) * V + lex] (clover == 0: not written), and the hopping part of the four links the site owns,
//   M_mu(x) = -1/2 W_mu(x) tr_spin[X(x+mu) Y(x)^dagger (1 - gamma_mu)] + 1/2 tr_spin[X(x) Y(x+mu)^dagger (1 + gamma_mu)] W_mu(x)^dagger,
// anti-Hermitian part into slots[((mu * SLOTS + HOP_SLOT) * 9 + r) * V + lex].
// GRID (gr: the process's Grid): A is the extended array [54][Ve] and the site writes its place in the interior; X and Y at x + mu
// come from gr->face[mu] where the neighbour table holds a slot.  The sums and their order are those of the undivided lattice.
template <bool GRID = false>
DDAMG_FS_HD void site_force_tensor(const Sites& g, const Gammas& gm, const double* __restrict__ X, const double* __restrict__ Y,
                                   const double* __restrict__ W, int clover, double* __restrict__ A, double* __restrict__ slots, size_t s,
                                   const Grid* gr = nullptr) {
  if (s >= g.V) return;
  const size_t V = g.V, lx = (size_t)g.lex[s];
  size_t AV = V, ax = lx;     // sites of A and this site's place in it
  if constexpr (GRID) { AV = gr->shell.Ve; ax = fs::extended_site(gr->shell, lx); }
  cplx x[12], y[12];
  load_spinor(X, V, s, x);
  load_spinor(Y, V, s, y);
  if (clover) {
    const double f = -g.csw * (g.parity[s] ? g.scale_odd : g.scale_even) / 8.0;
#pragma unroll 1
    for (int p = 0; p < 6; p++) {   // one plane at a time: the registers of one
      M3 lam;
#pragma unroll
      for (int k = 0; k < 9; k++) lam.a[k] = cplx{0.0, 0.0};
#pragma unroll
      for (int sp = 0; sp < 4; sp++)
#pragma unroll
        for (int sq = 0; sq < 4; sq++) {
          const cplx c{gm.prod.re[p][4 * sp + sq], gm.prod.im[p][4 * sp + sq]};
          if (c.r != 0.0 || c.i != 0.0) add_outer(lam, c, x, sq, y, sp);
        }
      double a9[9];
      pack_antihermitian(lam, f, a9);
#pragma unroll
      for (int r = 0; r < 9; r++) A[((size_t)p * 9 + r) * AV + ax] = a9[r];
    }
  }
#pragma unroll
  for (int mu = 0; mu < 4; mu++) {   // unrolled: every spin index below is a constant, so the spinors stay in registers
    const int nb = g.nb[(size_t)mu * V + s];
    cplx xn[12], yn[12];
    if (GRID && nb < 0) {
      const size_t F = (size_t)gr->F[mu], slot = (size_t)(-1 - nb);
      load_spinor(gr->face[mu], F, slot, xn);
      load_spinor(gr->face[mu] + 24 * F, F, slot, yn);
    } else {
      load_spinor(X, V, (size_t)nb, xn);
      load_spinor(Y, V, (size_t)nb, yn);
    }
    M3 pf, pb;     // tr_spin[X(x+mu) Y(x)^dagger (1 - gamma_mu)], tr_spin[X(x) Y(x+mu)^dagger (1 + gamma_mu)]
#pragma unroll
    for (int k = 0; k < 9; k++) { pf.a[k] = cplx{0.0, 0.0}; pb.a[k] = cplx{0.0, 0.0}; }
#pragma unroll
    for (int sp = 0; sp < 4; sp++) {
      const int sq = gamma_col(mu, sp);
      const cplx v{gm.re[mu][sp], gm.im[mu][sp]};
      add_outer(pf, cplx{1.0, 0.0}, xn, sp, y, sp);
      add_outer(pf, cplx{-v.r, -v.i}, xn, sq, y, sp);
      add_outer(pb, cplx{1.0, 0.0}, x, sp, yn, sp);
      add_outer(pb, v, x, sq, yn, sp);
    }
    const M3 w = load_link(W, lx, mu);
    const M3 m1 = fs::mul(w, pf), m2 = fs::mul(pb, fs::dag(w));
    M3 m;
#pragma unroll
    for (int k = 0; k < 9; k++) m.a[k] = cplx{0.5 * (m2.a[k].r - m1.a[k].r), 0.5 * (m2.a[k].i - m1.a[k].i)};
    double h9[9];
    pack_antihermitian(m, 1.0, h9);
#pragma unroll
    for (int r = 0; r < 9; r++) slots[((size_t)(mu * SLOTS + HOP_SLOT) * 9 + r) * V + lx] = h9[r];
  }
}

// ---- the tensor stage for many pairs (ddamg_hip_force_bilinear_multi_*, ddamg_hip_force_rational_*) ----
// Everything behind the tensor stage is linear in A_p(x) and in the hopping matrices, and both are sums of outer products X Y^dagger:
// sum_s w_s G(Y_s, X_s) needs one accumulation over the pairs and then the derivative and the assembly once.  A launch takes a group
// of up to GROUP pairs by value; `add` says whether it writes A and the hopping slots or adds to what they hold, so more pairs are a
// sequence of launches.  The sum runs over s in ascending order, every number has one writer, and two calls give the same bits.
// Two bodies, because four spinors and all accumulators do not fit the registers of one thread:
//   site_planes_multi   one thread per site: x_s, y_s of one pair at a time and the 54 packed reals of A as accumulators
//   site_hop_multi      one thread per (site, mu): two spinors at a time and the two 3x3 spin traces as accumulators; W_mu(x) does
//                       not depend on s and multiplies the sums once
#ifndef DDAMG_FORCE_GROUP
#define DDAMG_FORCE_GROUP 8
#endif
constexpr int GROUP = DDAMG_FORCE_GROUP;                // DDAMG_HIP_FORCE_GROUP of include/ddamg_hip.h
struct Pairs {
  const double* x[GROUP];
  const double* y[GROUP];       // fine fp64 vectors in the operator's layout
  double w[GROUP];
  int n, add;                   // pairs in this group; add != 0: onto what A and the hopping slots hold
};

// force_planes_multi_kernel: A_p(x) (+)= sum_s w_s A_p(x) of site_force_tensor for the pair s, in the packed 9 reals per plane.
// add: the sum starts from what A holds, so the result is the left fold over all pairs of all groups.  grid: the process
// grid's form with its Grid gr, as site_force_tensor<true> -- a run-time choice in ONE kernel, so that the undivided lattice and a process grid run
// the same instructions and give the same bits (the compiler contracts products and sums kernel by kernel)
DDAMG_FS_HD void site_planes_multi(const Sites& g, const Gammas& gm, const Pairs& pr, double* __restrict__ A, size_t s, bool grid = false,
                                   const Grid* gr = nullptr) {
  if (s >= g.V) return;
  const size_t V = g.V, lx = (size_t)g.lex[s];
  size_t AV = V, ax = lx;
  if (grid) { AV = gr->shell.Ve; ax = fs::extended_site(gr->shell, lx); }
  double acc[6][9];
#pragma unroll
  for (int p = 0; p < 6; p++)
#pragma unroll
    for (int r = 0; r < 9; r++) acc[p][r] = pr.add ? A[((size_t)p * 9 + r) * AV + ax] : 0.0;
  const double f = -g.csw * (g.parity[s] ? g.scale_odd : g.scale_even) / 8.0;
#pragma unroll 1
  for (int k = 0; k < pr.n; k++) {
    cplx x[12], y[12];
    load_spinor(pr.x[k], V, s, x);
    load_spinor(pr.y[k], V, s, y);
    const double fw = f * pr.w[k];
#pragma unroll
    for (int p = 0; p < 6; p++) {   // unrolled: the accumulators are registers.  Row sp of gamma_mu gamma_nu has its one entry in column sq
      M3 lam;
#pragma unroll
      for (int q = 0; q < 9; q++) lam.a[q] = cplx{0.0, 0.0};
#pragma unroll
      for (int sp = 0; sp < 4; sp++) {
        const int sq = gamma_col(fs::plane_nu(p), gamma_col(fs::plane_mu(p), sp));
        add_outer(lam, cplx{gm.prod.re[p][4 * sp + sq], gm.prod.im[p][4 * sp + sq]}, x, sq, y, sp);
      }
      double a9[9];
      pack_antihermitian(lam, fw, a9);
#pragma unroll
      for (int r = 0; r < 9; r++) acc[p][r] += a9[r];
    }
  }
#pragma unroll
  for (int p = 0; p < 6; p++)
#pragma unroll
    for (int r = 0; r < 9; r++) A[((size_t)p * 9 + r) * AV + ax] = acc[p][r];
}

// force_hop_multi_kernel, one thread per (site, MU): the hopping part of W_MU(x) of site_force_tensor for sum_s w_s (pair s),
//   pf = sum_s w_s tr_spin[X_s(x+mu) Y_s(x)^dagger (1 - gamma_mu)],  pb = sum_s w_s tr_spin[X_s(x) Y_s(x+mu)^dagger (1 + gamma_mu)],
// then  M = (pb W^dagger - W pf) / 2  once; anti-Hermitian part into (add: onto) the link's hopping slot.
// grid: where the neighbour table holds -1 - slot, X_s and Y_s at x + mu come from gr->face[MU], which holds X then Y of every
// pair of the group one after the other, 48 F doubles per pair
template <int MU>
DDAMG_FS_HD void site_hop_multi_dir(const Sites& g, const Gammas& gm, const Pairs& pr, const double* __restrict__ W, double* __restrict__ slots, size_t s,
                                    bool grid, const Grid* gr) {
  const size_t V = g.V, lx = (size_t)g.lex[s];
  const int nb = g.nb[(size_t)MU * V + s];
  M3 pf, pb;
#pragma unroll
  for (int q = 0; q < 9; q++) { pf.a[q] = cplx{0.0, 0.0}; pb.a[q] = cplx{0.0, 0.0}; }
#pragma unroll 1
  for (int k = 0; k < pr.n; k++) {
    const double w = pr.w[k];
    const double* fx = nullptr; size_t F = 0, slot = 0;
    if (grid && nb < 0) { F = (size_t)gr->F[MU]; slot = (size_t)(-1 - nb); fx = gr->face[MU] + (size_t)k * 48 * F; }
    {   // two spinors at a time: X(x+mu) and Y(x) ...
      cplx xn[12], y[12];
      if (grid && nb < 0) load_spinor(fx, F, slot, xn); else load_spinor(pr.x[k], V, (size_t)nb, xn);
      load_spinor(pr.y[k], V, s, y);
#pragma unroll
      for (int sp = 0; sp < 4; sp++) {
        add_outer(pf, cplx{w, 0.0}, xn, sp, y, sp);
        add_outer(pf, cplx{-w * gm.re[MU][sp], -w * gm.im[MU][sp]}, xn, gamma_col(MU, sp), y, sp);
      }
    }
    {   // ... then X(x) and Y(x+mu)
      cplx x[12], yn[12];
      load_spinor(pr.x[k], V, s, x);
      if (grid && nb < 0) load_spinor(fx + 24 * F, F, slot, yn); else load_spinor(pr.y[k], V, (size_t)nb, yn);
#pragma unroll
      for (int sp = 0; sp < 4; sp++) {
        add_outer(pb, cplx{w, 0.0}, x, sp, yn, sp);
        add_outer(pb, cplx{w * gm.re[MU][sp], w * gm.im[MU][sp]}, x, gamma_col(MU, sp), yn, sp);
      }
    }
  }
  const M3 link = load_link(W, lx, MU);
  const M3 m1 = fs::mul(link, pf), m2 = fs::mul(pb, fs::dag(link));
  M3 m;
#pragma unroll
  for (int q = 0; q < 9; q++) m.a[q] = cplx{0.5 * (m2.a[q].r - m1.a[q].r), 0.5 * (m2.a[q].i - m1.a[q].i)};
  double h9[9];
  pack_antihermitian(m, 1.0, h9);
#pragma unroll
  for (int r = 0; r < 9; r++) {
    double* o = slots + ((size_t)(MU * SLOTS + HOP_SLOT) * 9 + r) * V + lx;
    *o = pr.add ? *o + h9[r] : h9[r];
  }
}
DDAMG_FS_HD void site_hop_multi(const Sites& g, const Gammas& gm, const Pairs& pr, const double* __restrict__ W, double* __restrict__ slots, size_t s, int mu,
                                bool grid = false, const Grid* gr = nullptr) {
  if (s >= g.V) return;
  switch (mu) {     // a constant direction in each body: every spin index is one too
    case 0: site_hop_multi_dir<0>(g, gm, pr, W, slots, s, grid, gr); break;
    case 1: site_hop_multi_dir<1>(g, gm, pr, W, slots, s, grid, gr); break;
    case 2: site_hop_multi_dir<2>(g, gm, pr, W, slots, s, grid, gr); break;
    default: site_hop_multi_dir<3>(g, gm, pr, W, slots, s, grid, gr); break;
  }
}

// entry (i, j) of a Hermitian 6x6 block in the packing of fine_op.h: 6 real diagonal entries, then the 15 strict-upper ones
DDAMG_FS_HD cplx herm6_entry(const double* b, int i, int j) {
  if (i == j) return cplx{b[i], 0.0};
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  const int k = 5 * lo - lo * (lo - 1) / 2 + hi - lo - 1;
  return cplx{b[6 + 2 * k], i < j ? b[6 + 2 * k + 1] : -b[6 + 2 * k + 1]};
}

// force_inverse_tensor_kernel, one thread per site: A_p of  sum over the sites of parity `par` of log|det C(x)|,
//   Lambda_p(x)[b][a] = sum_{s,s'} (gamma_mu gamma_nu)[s][s'] [C(x)^-1][s' b][s a]
// from the inverse blocks the odd-even kernels read (clover_inv: 72 reals per site, chunked SoA), zero on the other parity.
// shell != nullptr: A is the extended array [54][Ve] of that shell and the site writes its place in the interior
DDAMG_FS_HD void site_inverse_tensor(const Sites& g, const Gammas& gm, const double* __restrict__ clover_inv, int par,
                                     double* __restrict__ A, size_t s, const fs::Shell* shell = nullptr) {
  if (s >= g.V) return;
  const size_t V = g.V, lx = (size_t)g.lex[s];
  const size_t AV = shell ? shell->Ve : V, ax = shell ? fs::extended_site(*shell, lx) : lx;
  if (g.parity[s] != par) {
    for (int k = 0; k < 54; k++) A[(size_t)k * AV + ax] = 0.0;
    return;
  }
  double inv[72];
#pragma unroll
  for (int r = 0; r < 72; r++) inv[r] = clover_inv[soa2(V, s, r)];
  const double f = -g.csw * (g.parity[s] ? g.scale_odd : g.scale_even) / 8.0;
#pragma unroll
  for (int p = 0; p < 6; p++) {
    M3 lam;
#pragma unroll
    for (int k = 0; k < 9; k++) lam.a[k] = cplx{0.0, 0.0};
#pragma unroll
    for (int sp = 0; sp < 4; sp++)
#pragma unroll
      for (int sq = 0; sq < 4; sq++) {
        const cplx c{gm.prod.re[p][4 * sp + sq], gm.prod.im[p][4 * sp + sq]};
        if ((c.r == 0.0 && c.i == 0.0) || sp / 2 != sq / 2) continue;     // C^-1 couples the spins of one block only
        const double* blk = inv + 36 * (sp / 2);
#pragma unroll
        for (int b = 0; b < 3; b++)
#pragma unroll
          for (int a = 0; a < 3; a++) {
            const cplx e = herm6_entry(blk, 3 * (sq % 2) + b, 3 * (sp % 2) + a);
            lam.a[3 * b + a].r += c.r * e.r - c.i * e.i;
            lam.a[3 * b + a].i += c.r * e.i + c.i * e.r;
          }
      }
    double a9[9];
    pack_antihermitian(lam, f, a9);
#pragma unroll
    for (int r = 0; r < 9; r++) A[((size_t)p * 9 + r) * AV + ax] = a9[r];
  }
}

// tensor_slab_pack_kernel (to_buffer) / tensor_slab_unpack_kernel, thread i of 54 * sites: one real of the slab `b` of the extended
// array A [54][Ve]; buf [54][sites], component-major as A, the sites in the slab's own lexicographic order (fs::slab_site), the same
// on the sender and the receiver.  Consecutive threads: consecutive sites of one component, which are consecutive reals of buf and,
// along the slab's fastest direction, of A.  8-byte accesses: a row of the slab starts at any site of A, so a pair of sites is not
// 16-byte aligned in general.
DDAMG_FS_HD void tensor_slab_copy(const fs::Shell& s, const fs::Slab& b, double* __restrict__ A, double* __restrict__ buf, size_t i, bool to_buffer) {
  if (i >= b.sites * 54) return;
  const size_t comp = i / b.sites, site = i - comp * b.sites;
  double* in_array = A + comp * s.Ve + fs::slab_site(s, b, site);
  if (to_buffer) buf[i] = *in_array; else *in_array = buf[i];
}

// face_spinor_pack_kernel, thread i of 24 * F: complex k = i / F of (X, Y) (k < 12: X) at the face site of slot i % F, 16 bytes,
// into buf: X then Y as chunked-SoA fields of F sites -- what Grid::face[mu] is on the receiver.  sites[slot]: the device site
// with x_mu = 0 of that slot (Geometry::face_sites[4 + mu]).  Consecutive threads write consecutive 16 bytes.
DDAMG_FS_HD void face_spinor_pack(const double* __restrict__ X, const double* __restrict__ Y, size_t V, const int* __restrict__ sites, size_t F,
                                  double* __restrict__ buf, size_t i) {
  if (i >= 24 * F) return;
  const size_t k = i / F, slot = i - k * F;
  const double* v = (k < 12 ? X : Y) + soa2(V, (size_t)sites[slot], 2 * (int)(k % 12));
  *reinterpret_cast<fs::Reals<2>*>(buf + 2 * i) = *reinterpret_cast<const fs::Reals<2>*>(v);
}

// clover_derivative_kernel, step 2b, all threads: A of plane p on the staged neighbourhood, lds_a[e * APITCH + r]
// (off: fs::stage_offsets of the tile).  On a process grid: V the sites of the extended array, t and off those of
// fs::extended_tile and fs::stage_offsets<true>
DDAMG_FS_HD void stage_tensor(const double* __restrict__ A, size_t V, int p, const fs::Tile& t, int tid, const size_t* off, double* lds_a) {
  for (int k = tid; k < fs::NEXT * 9; k += fs::THREADS) {
    const int r = k / fs::NEXT, e = k - r * fs::NEXT;      // consecutive threads: consecutive sites of one component
    const int i = e / fs::EXT, j = e - i * fs::EXT;
    lds_a[e * APITCH + r] = A[((size_t)p * 9 + r) * V + t.outside + off[i] + off[fs::EXT + j]];
  }
}

DDAMG_FS_HD M3 add(const M3& x, const M3& y) {
  M3 r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.a[k] = cplx{x.a[k].r + y.a[k].r, x.a[k].i + y.a[k].i};
  return r;
}

// One step of the counter-clockwise walk round a plaquette of the plane, the orientation of all four leaves: c = 0: +mu, 1: +nu,
// 2: -mu, 3: -nu from the staged site pos.  Returns the factor of the step (the link on the way forward, the dagger of the link it
// walks back over) and moves pos.
DDAMG_FS_HD M3 walk(const double* lds, int c, int& pos) {
  const int d = (c & 1) ? 1 : fs::EXT;
  if (c < 2) { const M3 m = fs::staged(lds, c & 1, pos); pos += d; return m; }
  pos -= d;
  return fs::dag(fs::staged(lds, c & 1, pos));
}

// step 3, one thread per site of the tile: the plane's contribution to the two links the site owns (w = 0: W_mu(x), 1: W_nu(x)),
// anti-Hermitian part in 9 reals each.  Returns false for a thread outside the lattice (tile tail).
// The eight rotations of a link are those of its two plaquettes with A at each of the four corners: the four leaves that hold a
// plaquette walk round it in the same sense and differ in the corner they start from.  Behind the link come the three steps
// G1 G2 G3 of the staple, with corners c0 .. c3 along them, and
//   T = A(c0) G1 G2 G3 + G1 A(c1) G2 G3 + G1 G2 A(c2) G3 + G1 G2 G3 A(c3) = A(c0) (G1 (G2 G3)) + G1 [A(c1) (G2 G3) + G2 (A(c2) G3 + G3 A(c3))]
// in eight products; the plaquette that walks the link forward gives W T, the one that walks it backward -T W^dagger.
DDAMG_FS_HD bool site_clover_derivative(const fs::Planes& g, const fs::Tile& t, int tid, const double* lds, const double* lds_a, size_t* lex,
                                        double (&out)[2][9]) {
  const int a = tid / fs::TILE, b = tid - a * fs::TILE;
  if (t.a0 + a >= g.L[t.mu] || t.b0 + b >= g.L[t.nu]) return false;
  *lex = t.outside + (size_t)(t.a0 + a) * t.smu + (size_t)(t.b0 + b) * t.snu;
  const int x = (a + 1) * fs::EXT + (b + 1);
#pragma unroll 1
  for (int w = 0; w < 2; w++) {   // one link at a time: the registers of one
    const M3 link = fs::staged(lds, w, x);
    M3 m;
#pragma unroll
    for (int back = 0; back < 2; back++) {
      const int c = w + 2 * back;                          // the step of the walk that is this link
      int pos = back ? x : x + (w ? 1 : fs::EXT);          // where that step ends
      const M3 a0 = unpack_antihermitian(lds_a + pos * APITCH);
      const M3 g1 = walk(lds, (c + 1) & 3, pos), a1 = unpack_antihermitian(lds_a + pos * APITCH);
      const M3 g2 = walk(lds, (c + 2) & 3, pos), a2 = unpack_antihermitian(lds_a + pos * APITCH);
      const M3 g3 = walk(lds, (c + 3) & 3, pos), a3 = unpack_antihermitian(lds_a + pos * APITCH);
      const M3 p23 = fs::mul(g2, g3);
      const M3 inner = add(fs::mul(a2, g3), fs::mul(g3, a3));
      const M3 mid = add(fs::mul(a1, p23), fs::mul(g2, inner));
      const M3 T = add(fs::mul(a0, fs::mul(g1, p23)), fs::mul(g1, mid));
      if (!back) {
        m = fs::mul(link, T);
      } else {
        const M3 r = fs::mul(T, fs::dag(link));
#pragma unroll
        for (int q = 0; q < 9; q++) { m.a[q].r -= r.a[q].r; m.a[q].i -= r.a[q].i; }
      }
    }
    double o9[9];
    pack_antihermitian(m, 1.0, o9);
#pragma unroll
    for (int r = 0; r < 9; r++) { if (w == 0) out[0][r] = o9[r]; else out[1][r] = o9[r]; }   // constant indices: registers
  }
  return true;
}
// the slot of plane (mu, nu) among the three planes of a link direction: the other direction's rank among the three others
DDAMG_FS_HD int plane_slot(int link_dir, int other_dir) { return other_dir < link_dir ? other_dir : other_dir - 1; }

// force_assemble_kernel, one thread per lexicographic site: G = TA(sum of the slots), out (+)= coeff * G as [V][4][9] complex.
// clover / hop: whether the three plane slots / the hopping slot hold anything
DDAMG_FS_HD void site_assemble(const double* __restrict__ slots, size_t V, size_t lx, int clover, int hop, double coeff, int accumulate,
                               double* __restrict__ out) {
  if (lx >= V) return;
#pragma unroll
  for (int mu = 0; mu < 4; mu++) {
    double g[9];
#pragma unroll
    for (int r = 0; r < 9; r++) {
      double sum = 0.0;
      if (clover)
        for (int k = 0; k < HOP_SLOT; k++) sum += slots[((size_t)(mu * SLOTS + k) * 9 + r) * V + lx];
      if (hop) sum += slots[((size_t)(mu * SLOTS + HOP_SLOT) * 9 + r) * V + lx];
      g[r] = sum;
    }
    const double tr = (g[0] + g[1] + g[2]) / 3.0;
#pragma unroll
    for (int i = 0; i < 3; i++) g[i] -= tr;
    const M3 m = unpack_antihermitian(g);
    double* o = out + (lx * 4 + mu) * 18;
#pragma unroll
    for (int k = 0; k < 9; k++) {
      const double re = coeff * m.a[k].r, im = coeff * m.a[k].i;
      o[2 * k] = accumulate ? o[2 * k] + re : re;
      o[2 * k + 1] = accumulate ? o[2 * k + 1] + im : im;
    }
  }
}

}  // namespace force
}  // namespace ddamg

#if defined(__HIPCC__)
#include "extended_links.h"
#include "fine_op.h"
#include <memory>
namespace ddamg {
// work space of the force entry points, in the context from the first call on: the links, A (54 reals per site), the slots
// (4 x 4 x 9) and, for the _device entry point, X and Y in the operator's layout
struct ForceWork {
  DeviceBuffer<double> W, A, slots, x, y;
  DeviceBuffer<double> group;     // the many-pair _device and rational entry points: X then Y of the force::GROUP pairs of a group
  // the _grid entry points on a process grid, from the first such call on: W = 2 D and A extended by the neighbours' shell (the slab
  // buffers of the links serve the tensor too: 54 reals per site against 72), and the face spinors of the hopping part, of a
  // whole group of pairs
  std::unique_ptr<ExtendedLinks> links;
  DeviceBuffer<double> Ae, face_send, face_recv;
  DeviceBuffer<int> face_sites;     // Geometry::face_sites[4 + mu] of the split directions, one after the other
};
// force_dev (+)= coeff * the force of Re <Y, D X> (x, y: fine fp64 vectors in the operator's layout; lex: the site table of level 0)
void force_bilinear(const FineOp<double>& op, const int L[4], const int* lex, double csw, double scale_even, double scale_odd, const double* y,
                    const double* x, double coeff, int accumulate, double* force_dev, ForceWork& w, hipStream_t st);
// ... of the sum over the sites of parity `par` of log|det C(x)|
void force_logdet(const FineOp<double>& op, const int L[4], const int* lex, double csw, double scale_even, double scale_odd, int par, double coeff,
                  int accumulate, double* force_dev, ForceWork& w, hipStream_t st);
// the same on a process grid (g.distributed()), collective: this process's part of the force; the neighbours' shell of W and of A
// and their face spinors travel over comm (comm_sendrecv_device).  Messages per split direction: bilinear 1 (spinors), and with a
// clover term 2 (links) + 2 (tensor) more; determinant 2 + 2, none without a clover term.
void force_bilinear_grid(const FineOp<double>& op, const Geometry& g, Comm* comm, const int* lex, double csw, double scale_even, double scale_odd,
                         const double* y, const double* x, double coeff, int accumulate, double* force_dev, ForceWork& w, hipStream_t st);
void force_logdet_grid(const FineOp<double>& op, const Geometry& g, Comm* comm, const int* lex, double csw, double scale_even, double scale_odd, int par,
                       double coeff, int accumulate, double* force_dev, ForceWork& w, hipStream_t st);
// force_dev (+)= coeff * sum_s weights[s] * the force of Re <Y_s, D X_s>, in three steps so that a caller can build the pairs of a
// group in one workspace while the call runs: begin (the links once; on a process grid their shell), any number of groups of
// 1 .. force::GROUP pairs (the tensor stage; on a process grid one message per split direction with the face spinors of the whole
// group), end (with a clover term the shell of A and the derivative, then the assembly, all once).  g.distributed() chooses the form.
struct ForceMulti {
  force::Sites sites;
  force::Grid grid;
  const double* W = nullptr;
  double* A = nullptr;
  double* slots = nullptr;
  bool clover = false, distributed = false;
  int groups = 0;
};
ForceMulti force_multi_begin(const FineOp<double>& op, const Geometry& g, Comm* comm, const int* lex, double csw, double scale_even, double scale_odd,
                             ForceWork& w, hipStream_t st);
void force_multi_group(ForceMulti& m, const Geometry& g, Comm* comm, int n, const double* const* y, const double* const* x, const double* weights,
                       ForceWork& w, hipStream_t st);
void force_multi_end(ForceMulti& m, const Geometry& g, Comm* comm, double coeff, int accumulate, double* force_dev, ForceWork& w, hipStream_t st);
}  // namespace ddamg
#endif
