// multishift.h -- multi-shift conjugate gradients on A_s = Dhat^dagger Dhat + sigma_s, sigma_s >= 0, of the even-odd preconditioned
// system (eo_system.h): one Krylov space for all shifts (B. Jegerlehner, hep-lat/9612014).  What rational HMC needs for
// phi^dagger [alpha_0 + sum_s rho_s (Dhat^dagger Dhat + sigma_s)^-1] phi.  Everything is fp64; every A_s is Hermitian positive
// definite, so all recurrence scalars are real.
//
// The base system is the smallest shift (it converges last) and runs ordinary CG: its r and p are full-length vectors in the
// solver's layout with zeros on the odd sites, which schur_apply takes as they are.  Every shift keeps x_s and p_s as PACKED even
// fields: 12 chunk rows of V/2 complex numbers, entry (k, j) at (k * V/2 + j) * 2 reals, where j counts the even sites in device
// site order (even_site[j] = the site, ascending).  Sites are ordered block by block with the two parities of a block apart
// (geometry.h), so consecutive j are consecutive sites in runs of half a Schwarz block: the reads of r at (k * V + even_site[j]) * 2
// are made of whole 128-byte (2^4 blocks) to 1 KiB segments, the packed side is fully coalesced.
//
// Scalars of step k (zeta_s^0 = zeta_s^-1 = 1, alpha_-1 = 1, beta_-1 = 0, d_s = sigma_s - sigma_base), all on the host:
//   alpha_k      = <r_k, r_k> / <p_k, A p_k>,    beta_k = <r_k+1, r_k+1> / <r_k, r_k>
//   zeta_s^k+1   = zeta_s^k zeta_s^k-1 alpha_k-1 / ( alpha_k beta_k-1 (zeta_s^k-1 - zeta_s^k) + zeta_s^k-1 alpha_k-1 (1 + d_s alpha_k) )
//   alpha_s      = alpha_k zeta_s^k+1 / zeta_s^k,    beta_s = beta_k (zeta_s^k+1 / zeta_s^k)^2
//   x_s += alpha_s p_s,   p_s = zeta_s^k+1 r_k+1 + beta_s p_s,   residual of shift s: zeta_s^k+1 r_k+1
// For d_s = 0 the recurrence gives zeta = 1, alpha_s = alpha, beta_s = beta exactly, so the base system is the shift with d = 0 and
// a duplicate of it gets its bits.
#pragma once
#include "blas.h"
#include <vector>

namespace ddamg {

constexpr int MS_MAX_SHIFTS = 32;   // DDAMG_HIP_MAX_SHIFTS
// coefficients of one update launch in device memory (ReduceWork::d_coef): a head of MS_COEF_HEAD reals
//   [0] number of entries that follow, [1] beta, [2] alpha, [3] the slot of the base system's x (-1: frozen, x is left alone)
// then MS_COEF_PER reals per active shift: [0] its slot, [1] alpha_s, [2] beta_s, [3] zeta_s^k+1
constexpr int MS_COEF_HEAD = 4, MS_COEF_PER = 4;
constexpr int MS_COEF_MAX = MS_COEF_HEAD + MS_COEF_PER * MS_MAX_SHIFTS;

// what the context keeps between solves: the reduction workspace of the loop and the list of even sites
struct MultishiftWork {
  ReduceWork rw;
  DeviceBuffer<int> even_site;   // [V/2] the sites of parity 0 in ascending device order
  int V = 0;
  bool ready = false;
};
// parity: the global parity of every site in device order (Geometry::parity)
void multishift_prepare(MultishiftWork& w, const std::vector<int>& parity, hipStream_t st);

// packed (k, j) <-> the even sites of a full-length vector; scatter leaves the odd sites of `full` alone
void multishift_gather(double* packed, const double* full, const int* even_site, int V, hipStream_t st);
void multishift_scatter(double* full, const double* packed, const int* even_site, int V, hipStream_t st);

// the base system's residual on the even sites, r -= alpha (u + sigma p) with u = Dhat^dagger Dhat p, and d_out[0] = <r, r> of the new r
// in the same pass (two-stage deterministic sum through rw, global on a process grid).  The odd sites hold zeros and keep them.
void multishift_residual(double* r, const double* u, const double* p, double alpha, double sigma, const int* even_site, int V, ReduceWork& rw,
                         double* d_out, hipStream_t st);

// One pass over the even sites (multishift_update_kernel): with r = the new residual, read once,
//   base:   x_base += alpha p (unless frozen),  p = r + beta p           (p full-length, x_base = xs + slot * half)
//   every active shift:  x_s += alpha_s p_s,  p_s = zeta_s r + beta_s p_s   (xs + slot * half, ps + slot * half)
// with the list of active shifts and their reals in d_coef (layout above); half = 12 * V reals, the length of a packed field.
void multishift_update(double* p, const double* r, double* xs, double* ps, const double* d_coef, const int* even_site, int V, hipStream_t st);

// smallest and largest eigenvalue of the Lanczos tridiagonal matrix that the CG scalars alpha_k, beta_k of k = 0..n-1 define,
//   T_jj = 1 / alpha_j + beta_j-1 / alpha_j-1,   T_j,j+1 = sqrt(beta_j) / alpha_j,
// by bisection on the Sturm sequence (host; no LAPACK in this build).  n = 0: both zero.
void lanczos_extremes(const std::vector<double>& alpha, const std::vector<double>& beta, double out[2]);

}  // namespace ddamg
