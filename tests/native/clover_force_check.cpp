// clover_force_check.cpp -- a stand-alone host program (no GPU, no HIP) over the kernel bodies of csrc/force.h: site_force_tensor,
// site_inverse_tensor, stage_tensor, site_clover_derivative and site_assemble, with fs::stage_offsets / stage_links, run thread by
// thread as the kernels of force.hip run them.  tests/test_clover_force_native.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it; it prints CLOVER_FORCE_OK and exits 0 when every comparison held.
//
// The reference is brute force on the periodic global lattice, in its own arithmetic (std::complex, dense 4x4 gamma matrices and a
// dense 12x12 inverse): for every site, plane, leaf and factor of the leaf, the rotation of the leaf that starts at that factor goes
// to the link the factor is; the hopping part follows its formula entry by entry.  Links are random complex matrices, not unitary
// ones, so that no cancellation hides a misplaced factor; sites are stored even sites first, so that the site tables are used.
#include "force.h"
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace ddamg;
typedef std::complex<double> cd;
struct Mat { cd a[3][3]; };

static int failures = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (failures < 20) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
      failures++;                                                              \
    }                                                                          \
  } while (0)

static uint64_t rng_state = 1;
static double urand() {   // splitmix64, uniform in (-0.5, 0.5)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
  return (double)(z >> 11) / 9007199254740992.0 - 0.5;
}
static double* exact_alloc(size_t doubles) {   // not a byte longer than asked for: the sanitizer guards both ends
  double* p = static_cast<double*>(malloc(doubles * sizeof(double)));
  if (!p) { printf("out of memory\n"); exit(2); }
  return p;
}

static Mat mul(const Mat& x, const Mat& y) {
  Mat r;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { r.a[i][j] = 0; for (int k = 0; k < 3; k++) r.a[i][j] += x.a[i][k] * y.a[k][j]; }
  return r;
}
static Mat dag(const Mat& x) { Mat r; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r.a[i][j] = std::conj(x.a[j][i]); return r; }

struct Lattice {
  int L[4]; size_t V;
  size_t lex(const int c[4]) const {
    int w[4];
    for (int d = 0; d < 4; d++) w[d] = ((c[d] % L[d]) + L[d]) % L[d];
    return (((size_t)w[0] * L[1] + w[1]) * L[2] + w[2]) * L[3] + w[3];
  }
  void coords(size_t lx, int c[4]) const { for (int d = 3; d >= 0; d--) { c[d] = (int)(lx % L[d]); lx /= L[d]; } }
};

static Mat link_at(const Lattice& g, const double* W, const int c[4], int mu) {
  const double* p = W + (g.lex(c) * 4 + mu) * 18;
  Mat m;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m.a[i][j] = cd(p[2 * (3 * i + j)], p[2 * (3 * i + j) + 1]);
  return m;
}

// the leaves written out once more, by hand, from Q_mu_nu(y): (direction: 0 = mu, 1 = nu; steps in mu and nu from y; daggered)
static const int LEAF[4][4][4] = {
    {{0, 0, 0, 0}, {1, 1, 0, 0}, {0, 0, 1, 1}, {1, 0, 0, 1}},        // U_mu(y) U_nu(y+mu) U_mu(y+nu)^+ U_nu(y)^+
    {{1, 0, 0, 0}, {0, -1, 1, 1}, {1, -1, 0, 1}, {0, -1, 0, 0}},     // U_nu(y) U_mu(y-mu+nu)^+ U_nu(y-mu)^+ U_mu(y-mu)
    {{0, -1, 0, 1}, {1, -1, -1, 1}, {0, -1, -1, 0}, {1, 0, -1, 0}},  // U_mu(y-mu)^+ U_nu(y-mu-nu)^+ U_mu(y-mu-nu) U_nu(y-nu)
    {{1, 0, -1, 1}, {0, 0, -1, 0}, {1, 1, -1, 0}, {0, 0, 0, 1}}};    // U_nu(y-nu)^+ U_mu(y-nu) U_nu(y-nu+mu) U_mu(y)^+

// M_mu(x) of sum_y sum_p Re tr[Q_p(y) A_p(y)], A given as full matrices [p][lex]
static void brute_force_clover(const Lattice& g, const double* W, const std::vector<Mat>& A, std::vector<Mat>& M) {
  for (size_t ly = 0; ly < g.V; ly++) {
    int y[4]; g.coords(ly, y);
    for (int p = 0; p < 6; p++) {
      const int mu = fs::plane_mu(p), nu = fs::plane_nu(p);
      for (int leaf = 0; leaf < 4; leaf++) {
        Mat f[4]; int where[4][4];
        for (int k = 0; k < 4; k++) {
          for (int d = 0; d < 4; d++) where[k][d] = y[d];
          where[k][mu] += LEAF[leaf][k][1]; where[k][nu] += LEAF[leaf][k][2];
          const Mat u = link_at(g, W, where[k], LEAF[leaf][k][0] ? nu : mu);
          f[k] = LEAF[leaf][k][3] ? dag(u) : u;
        }
        for (int k = 0; k < 4; k++) {
          const bool dg = LEAF[leaf][k][3] != 0;
          const int first = dg ? k + 1 : k;
          Mat r = A[p * g.V + ly];
          for (int j = 3; j >= first; j--) r = mul(f[j], r);
          for (int j = 0; j < first; j++) r = mul(r, f[j]);
          Mat& m = M[g.lex(where[k]) * 4 + (LEAF[leaf][k][0] ? nu : mu)];
          for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m.a[i][j] += dg ? -r.a[i][j] : r.a[i][j];
        }
      }
    }
  }
}

static void run_case(const char* name, const int L[4], bool determinant, int par, double csw, double coeff) {
  Lattice g; g.V = 1;
  for (int d = 0; d < 4; d++) { g.L[d] = L[d]; g.V *= (size_t)L[d]; }
  const size_t V = g.V;
  // the device's site order: even sites first, each parity in lexicographic order
  std::vector<int> lex_of_site(V), site_of_lex(V), nb(8 * V);
  std::vector<unsigned char> parity(V);
  {
    size_t n = 0;
    for (int pass = 0; pass < 2; pass++)
      for (size_t lx = 0; lx < V; lx++) {
        int c[4]; g.coords(lx, c);
        if (((c[0] + c[1] + c[2] + c[3]) & 1) == pass) { lex_of_site[n] = (int)lx; site_of_lex[lx] = (int)n; parity[n] = (unsigned char)pass; n++; }
      }
    for (size_t s = 0; s < V; s++) {
      int c[4]; g.coords((size_t)lex_of_site[s], c);
      for (int mu = 0; mu < 4; mu++) {
        c[mu]++; nb[mu * V + s] = site_of_lex[g.lex(c)];
        c[mu] -= 2; nb[(4 + mu) * V + s] = site_of_lex[g.lex(c)];
        c[mu]++;
      }
    }
  }
  const double scale_even = 1.1, scale_odd = 0.9;
  const force::Gammas gm = force::make_gammas();
  const force::Sites sites{V, nb.data(), lex_of_site.data(), parity.data(), csw, scale_even, scale_odd};
  double* W = exact_alloc(72 * V); double* X = exact_alloc(24 * V); double* Y = exact_alloc(24 * V); double* Cinv = exact_alloc(72 * V);
  double* A = exact_alloc(54 * V); double* slots = exact_alloc(144 * V); double* out = exact_alloc(72 * V);
  for (size_t i = 0; i < 72 * V; i++) { W[i] = urand(); Cinv[i] = urand(); out[i] = urand(); }
  for (size_t i = 0; i < 24 * V; i++) { X[i] = urand(); Y[i] = urand(); }
  for (size_t i = 0; i < 54 * V; i++) A[i] = -7.0e300;
  for (size_t i = 0; i < 144 * V; i++) slots[i] = -7.0e300;
  std::vector<double> out0(out, out + 72 * V);

  // ---- the kernels, thread by thread ----
  const bool clover = csw != 0.0;
  for (size_t s = 0; s < V + 3; s++) {     // a few threads beyond the last site, as a grid has
    if (determinant) force::site_inverse_tensor(sites, gm, Cinv, par, A, s);
    else force::site_force_tensor(sites, gm, X, Y, W, (int)clover, A, slots, s);
  }
  if (clover) {
    const fs::Planes planes = fs::make_planes(L);
    double* lds = exact_alloc(fs::LDS_DOUBLES); double* lds_a = exact_alloc(force::LDS_A_DOUBLES);
    for (int p = 0; p < 6; p++)
      for (int block = 0; block < planes.nblocks[p]; block++) {
        size_t off[2 * fs::EXT]; int flip[fs::EXT];
        const fs::Tile t = fs::tile_of(planes, p, block);
        for (int i = 0; i < fs::LDS_DOUBLES; i++) lds[i] = -7.0e300;
        for (int i = 0; i < force::LDS_A_DOUBLES; i++) lds_a[i] = -7.0e300;
        for (int tid = 0; tid < fs::THREADS; tid++) fs::stage_offsets(planes, t, 0, tid, off, flip);
        for (int tid = 0; tid < fs::THREADS; tid++) { fs::stage_links(W, t, tid, off, flip, lds); force::stage_tensor(A, V, p, t, tid, off, lds_a); }
        for (int tid = 0; tid < fs::THREADS; tid++) {
          size_t lx = 0; double o[2][9];
          if (!force::site_clover_derivative(planes, t, tid, lds, lds_a, &lx, o)) continue;
          const int smu = t.mu * force::SLOTS + force::plane_slot(t.mu, t.nu), snu = t.nu * force::SLOTS + force::plane_slot(t.nu, t.mu);
          for (int r = 0; r < 9; r++) {
            CHECK(slots[((size_t)smu * 9 + r) * V + lx] == -7.0e300 && slots[((size_t)snu * 9 + r) * V + lx] == -7.0e300, "%s: a slot written twice", name);
            slots[((size_t)smu * 9 + r) * V + lx] = o[0][r];
            slots[((size_t)snu * 9 + r) * V + lx] = o[1][r];
          }
        }
      }
    free(lds); free(lds_a);
  }
  for (size_t lx = 0; lx < V + 3; lx++) force::site_assemble(slots, V, lx, (int)clover, determinant ? 0 : 1, coeff, 1, out);

  // ---- brute force ----
  cd gam[4][4][4], gprod[6][4][4];
  for (int mu = 0; mu < 4; mu++) for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) gam[mu][i][j] = j == force::gamma_col(mu, i) ? cd(gm.re[mu][i], gm.im[mu][i]) : cd(0);
  for (int p = 0; p < 6; p++)
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { gprod[p][i][j] = 0; for (int k = 0; k < 4; k++) gprod[p][i][j] += gam[fs::plane_mu(p)][i][k] * gam[fs::plane_nu(p)][k][j]; }
  auto spin = [&](const double* v, size_t lx, int sp, int c) { const size_t s = (size_t)site_of_lex[lx]; const int k = 3 * sp + c;
                                                               return cd(v[((size_t)k * V + s) * 2], v[((size_t)k * V + s) * 2 + 1]); };
  std::vector<Mat> M(4 * V), Afull(6 * V);
  for (auto& m : M) for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m.a[i][j] = 0;
  for (size_t lx = 0; lx < V; lx++) {
    const size_t s = (size_t)site_of_lex[lx];
    const double sc = parity[s] ? scale_odd : scale_even;
    cd inv[12][12];
    for (int i = 0; i < 12; i++) for (int j = 0; j < 12; j++) inv[i][j] = 0;
    for (int b = 0; b < 2; b++) {      // the Hermitian blocks of fine_op.h: 6 real diagonal entries, 15 strict-upper ones, row by row
      int k = 0;
      for (int i = 0; i < 6; i++) {
        inv[6 * b + i][6 * b + i] = Cinv[(((size_t)(36 * b + i) / 2) * V + s) * 2 + (36 * b + i) % 2];
        for (int j = i + 1; j < 6; j++, k++) {
          const int r = 36 * b + 6 + 2 * k;
          const cd e(Cinv[((size_t)(r / 2) * V + s) * 2], Cinv[((size_t)(r / 2) * V + s) * 2 + 1]);
          inv[6 * b + i][6 * b + j] = e; inv[6 * b + j][6 * b + i] = std::conj(e);
        }
      }
    }
    for (int p = 0; p < 6; p++) {
      Mat lam;
      for (int b = 0; b < 3; b++) for (int a = 0; a < 3; a++) {
        lam.a[b][a] = 0;
        for (int sp = 0; sp < 4; sp++) for (int sq = 0; sq < 4; sq++)
          lam.a[b][a] += gprod[p][sp][sq] * (determinant ? (parity[s] == par ? inv[3 * sq + b][3 * sp + a] : cd(0)) : spin(X, lx, sq, b) * std::conj(spin(Y, lx, sp, a)));
      }
      const Mat ld = dag(lam);
      for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Afull[p * V + lx].a[i][j] = -csw * sc * (lam.a[i][j] - ld.a[i][j]) / 16.0;
    }
  }
  if (clover) brute_force_clover(g, W, Afull, M);
  if (!determinant)
    for (size_t lx = 0; lx < V; lx++) {
      int c[4]; g.coords(lx, c);
      for (int mu = 0; mu < 4; mu++) {
        int n[4] = {c[0], c[1], c[2], c[3]}; n[mu]++;
        const size_t ln = g.lex(n);
        Mat P, Pb;
        for (int cc = 0; cc < 3; cc++) for (int a = 0; a < 3; a++) {
          P.a[cc][a] = 0; Pb.a[cc][a] = 0;
          for (int sp = 0; sp < 4; sp++) for (int sq = 0; sq < 4; sq++) {
            const cd one = sp == sq ? 1.0 : 0.0;
            P.a[cc][a] += (one - gam[mu][sp][sq]) * spin(X, ln, sq, cc) * std::conj(spin(Y, lx, sp, a));
            Pb.a[cc][a] += (one + gam[mu][sp][sq]) * spin(X, lx, sq, cc) * std::conj(spin(Y, ln, sp, a));
          }
        }
        const Mat w = link_at(g, W, c, mu), m1 = mul(w, P), m2 = mul(Pb, dag(w));
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M[lx * 4 + mu].a[i][j] += 0.5 * (m2.a[i][j] - m1.a[i][j]);
      }
    }
  double worst = 0, norm = 0, trace = 0, anti = 0;
  for (size_t l = 0; l < 4 * V; l++) {
    const Mat md = dag(M[l]);
    cd tr = 0;
    for (int i = 0; i < 3; i++) tr += (M[l].a[i][i] - md.a[i][i]) / 2.0;
    cd tg = 0;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
      const cd ref = coeff * ((M[l].a[i][j] - md.a[i][j]) / 2.0 - (i == j ? tr / 3.0 : cd(0)));
      const cd got = cd(out[l * 18 + 2 * (3 * i + j)], out[l * 18 + 2 * (3 * i + j) + 1]) - cd(out0[l * 18 + 2 * (3 * i + j)], out0[l * 18 + 2 * (3 * i + j) + 1]);
      const cd gt = cd(out[l * 18 + 2 * (3 * j + i)], out[l * 18 + 2 * (3 * j + i) + 1]) - cd(out0[l * 18 + 2 * (3 * j + i)], out0[l * 18 + 2 * (3 * j + i) + 1]);
      worst = std::fmax(worst, std::abs(got - ref)); norm = std::fmax(norm, std::abs(ref));
      anti = std::fmax(anti, std::abs(got + std::conj(gt)));
      if (i == j) tg += got;
    }
    trace = std::fmax(trace, std::abs(tg));
  }
  // accumulate = 1 onto random numbers of order one costs their rounding; the sums have at most 8 x 6 + 2 terms of 5 factors
  const double bar = 1e-12 * std::fmax(norm, 1.0);
  CHECK(norm > (clover || !determinant ? 1e-3 : -1.0), "%s: the reference force vanishes", name);
  CHECK(worst <= bar, "%s: largest difference %.3e against %.3e (largest entry %.3e)", name, worst, bar, norm);
  CHECK(trace <= bar && anti <= bar, "%s: trace %.3e, Hermitian part %.3e", name, trace, anti);
  printf("%s: largest entry %.3e difference %.3e%s\n", name, norm, worst, (worst <= bar && trace <= bar && anti <= bar) ? ": ok" : ": FAILED");
  free(W); free(X); free(Y); free(Cinv); free(A); free(slots); free(out);
}

int main() {
  const int lattices[3][4] = {{4, 4, 4, 4}, {4, 6, 8, 10}, {4, 4, 12, 12}};
  const char* names[3] = {"4^4", "4x6x8x10", "4x4x12x12"};
  char name[96];
  for (int l = 0; l < 3; l++) {
    snprintf(name, sizeof name, "%s bilinear csw 1.3", names[l]); run_case(name, lattices[l], false, 0, 1.3, -2.0);
    snprintf(name, sizeof name, "%s bilinear csw 0", names[l]); run_case(name, lattices[l], false, 0, 0.0, 0.7);
    snprintf(name, sizeof name, "%s determinant even", names[l]); run_case(name, lattices[l], true, 0, 1.3, 1.0);
    snprintf(name, sizeof name, "%s determinant odd", names[l]); run_case(name, lattices[l], true, 1, 1.3, -2.0);
  }
  if (failures) { printf("%d comparisons FAILED\n", failures); return 1; }
  printf("CLOVER_FORCE_OK\n");
  return 0;
}
