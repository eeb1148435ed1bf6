// gauge_md_check.cpp -- a stand-alone host program (no GPU, no HIP) over the kernel bodies of csrc/gauge_md.h: stage_offsets,
// stage_links, site_gauge_force and site_gauge_loops at both depths of the staged neighbourhood, force::site_assemble behind them,
// link_update (exp_matrix), link_reunitarize, momentum_update and kinetic_part, run thread by thread as the kernels of gauge_md.hip
// run them.  tests/test_gauge_md_native.py builds it with the host compiler under -fsanitize=address,undefined and runs it; it
// prints GAUGE_MD_OK and exits 0 when every comparison held.
//
// The reference is brute force on the periodic global lattice, in its own arithmetic (std::complex): every plaquette and every
// rectangle of every site is walked as a closed path in four dimensions, and for each of its factors the rotation of the loop that
// starts at that factor goes to the link the factor is (with a minus sign and one factor further on where the link is walked
// backwards).  Links are random complex matrices, not unitary ones, so that no cancellation hides a misplaced factor.
#include "gauge_md.h"
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
static Mat matrix_at(const double* p) {
  Mat m;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m.a[i][j] = cd(p[2 * (3 * i + j)], p[2 * (3 * i + j) + 1]);
  return m;
}

struct Lattice {
  int L[4]; size_t V;
  size_t lex(const int c[4]) const {
    int w[4];
    for (int d = 0; d < 4; d++) w[d] = ((c[d] % L[d]) + L[d]) % L[d];
    return (((size_t)w[0] * L[1] + w[1]) * L[2] + w[2]) * L[3] + w[3];
  }
  void coords(size_t lx, int c[4]) const { for (int d = 3; d >= 0; d--) { c[d] = (int)(lx % L[d]); lx /= L[d]; } }
};

// One closed loop from y: steps +1 + d (forward along d) or -1 - d (backward).  Adds Re tr of the loop to *sum and, for every factor,
// weight * (the rotation of the loop that belongs to the factor's link) to M.
static void brute_force_loop(const Lattice& g, const double* U, const int y[4], const int* steps, int n, double weight, double* sum, std::vector<Mat>& M) {
  Mat f[6]; size_t link[6]; bool back[6];
  int pos[4] = {y[0], y[1], y[2], y[3]};
  for (int k = 0; k < n; k++) {
    const int d = steps[k] > 0 ? steps[k] - 1 : -steps[k] - 1;
    back[k] = steps[k] < 0;
    if (back[k]) pos[d]--;
    link[k] = g.lex(pos) * 4 + d;
    const Mat u = matrix_at(U + link[k] * 18);
    f[k] = back[k] ? dag(u) : u;
    if (!back[k]) pos[d]++;
  }
  Mat all = f[0];
  for (int k = 1; k < n; k++) all = mul(all, f[k]);
  *sum += (all.a[0][0] + all.a[1][1] + all.a[2][2]).real();
  for (int k = 0; k < n; k++) {
    const int first = back[k] ? k + 1 : k;      // the rotation f_first ... f_{first - 1}
    Mat r = f[first % n];
    for (int j = 1; j < n; j++) r = mul(r, f[(first + j) % n]);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M[link[k]].a[i][j] += (back[k] ? -weight : weight) * r.a[i][j];
  }
}

static double max_abs(const std::vector<double>& v) { double m = 0; for (double x : v) m = std::fabs(x) > m ? std::fabs(x) : m; return m; }

// the force kernel and its assembly as gauge_md.hip launches them, thread by thread
template <int H>
static void run_force(const Lattice& g, const double* U, double beta, double c1, double coeff, int accumulate, double* out) {
  const fs::Planes planes = fs::make_planes(g.L);
  const size_t V = g.V, nslots = (size_t)4 * force::SLOTS * 9 * V;
  double* slots = exact_alloc(nslots);
  for (size_t i = 0; i < nslots; i++) slots[i] = NAN;     // a slot nobody writes poisons the force
  double* lds = exact_alloc(gmd::Nb<H>::LDS_DOUBLES);
  size_t off[2 * gmd::Nb<H>::EXT];
  std::vector<int> writers(4 * 3 * V, 0);
  for (int p = 0; p < 6; p++)
    for (int block = 0; block < planes.nblocks[p]; block++) {
      const fs::Tile t = fs::tile_of(planes, p, block);
      for (int tid = 0; tid < fs::THREADS; tid++) gmd::stage_offsets<H>(planes, t, tid, off);
      for (int i = 0; i < gmd::Nb<H>::LDS_DOUBLES; i++) lds[i] = NAN;
      for (int tid = 0; tid < fs::THREADS; tid++) gmd::stage_links<H>(U, t, tid, off, lds);
      for (int tid = 0; tid < fs::THREADS; tid++) {
        size_t lex = 0; double o[2][9];
        if (!gmd::site_gauge_force<H>(planes, t, tid, lds, beta, 1.0 - 8.0 * c1, c1, &lex, o)) continue;
        CHECK(lex < V, "site %zu outside the lattice", lex);
        const int smu = t.mu * force::SLOTS + force::plane_slot(t.mu, t.nu), snu = t.nu * force::SLOTS + force::plane_slot(t.nu, t.mu);
        for (int r = 0; r < 9; r++) { slots[((size_t)smu * 9 + r) * V + lex] = o[0][r]; slots[((size_t)snu * 9 + r) * V + lex] = o[1][r]; }
        writers[((size_t)t.mu * 3 + force::plane_slot(t.mu, t.nu)) * V + lex]++;
        writers[((size_t)t.nu * 3 + force::plane_slot(t.nu, t.mu)) * V + lex]++;
      }
    }
  for (int w : writers) CHECK(w == 1, "a slot has %d writers", w);
  for (size_t lx = 0; lx < ((V + 127) / 128) * 128; lx++) force::site_assemble(slots, V, lx, 1, 0, coeff, accumulate, out);
  free(lds); free(slots);
}

template <int H>
static void run_loops(const Lattice& g, const double* U, double* plaq, double* rect) {
  const fs::Planes planes = fs::make_planes(g.L);
  double* lds = exact_alloc(gmd::Nb<H>::LDS_DOUBLES);
  size_t off[2 * gmd::Nb<H>::EXT];
  *plaq = 0; *rect = 0;
  for (int p = 0; p < 6; p++)
    for (int block = 0; block < planes.nblocks[p]; block++) {
      const fs::Tile t = fs::tile_of(planes, p, block);
      for (int tid = 0; tid < fs::THREADS; tid++) gmd::stage_offsets<H>(planes, t, tid, off);
      for (int i = 0; i < gmd::Nb<H>::LDS_DOUBLES; i++) lds[i] = NAN;
      for (int tid = 0; tid < fs::THREADS; tid++) gmd::stage_links<H>(U, t, tid, off, lds);
      for (int tid = 0; tid < fs::THREADS; tid++) {
        double pl, re;
        gmd::site_gauge_loops<H>(planes, t, tid, lds, &pl, &re);
        *plaq += pl; *rect += re;
      }
    }
  free(lds);
}

static void run_lattice(const char* name, const int L[4]) {
  Lattice g; g.V = 1;
  for (int d = 0; d < 4; d++) { g.L[d] = L[d]; g.V *= (size_t)L[d]; }
  const size_t V = g.V;
  const double beta = 5.6;
  double* U = exact_alloc(72 * V);
  for (size_t i = 0; i < 72 * V; i++) U[i] = urand();
  // brute force: the sums, and M of the plaquette part and of the rectangle part with weight -beta/3
  std::vector<Mat> MP(4 * V), MR(4 * V);
  for (auto& m : MP) for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m.a[i][j] = 0;
  MR = MP;
  double plaq = 0, rect = 0;
  for (size_t ly = 0; ly < V; ly++) {
    int y[4]; g.coords(ly, y);
    for (int mu = 0; mu < 4; mu++)
      for (int nu = 0; nu < 4; nu++) {
        if (nu == mu) continue;
        if (mu < nu) { const int s[4] = {1 + mu, 1 + nu, -1 - mu, -1 - nu}; brute_force_loop(g, U, y, s, 4, -beta / 3.0, &plaq, MP); }
        const int s[6] = {1 + mu, 1 + mu, 1 + nu, -1 - mu, -1 - mu, -1 - nu};
        brute_force_loop(g, U, y, s, 6, -beta / 3.0, &rect, MR);
      }
  }
  // the loops at both depths
  double p1, r1, p2, r2;
  run_loops<1>(g, U, &p1, &r1);
  run_loops<2>(g, U, &p2, &r2);
  CHECK(std::fabs(p1 - plaq) <= 1e-13 * (double)V && std::fabs(p2 - plaq) <= 1e-13 * (double)V && r1 == 0.0, "plaquette sum %.15e %.15e, brute force %.15e", p1,
        p2, plaq);
  CHECK(std::fabs(r2 - rect) <= 1e-13 * (double)V, "rectangle sum %.15e, brute force %.15e", r2, rect);
  printf("%s loops: plaquette %.12e (difference %.1e), rectangle %.12e (difference %.1e): %s\n", name, p2, std::fabs(p2 - plaq), r2, std::fabs(r2 - rect),
         failures ? "FAILED" : "ok");
  // the force for the three actions; c1 == 0 through the one-site neighbourhood, as the library runs it, and through the two-site one
  const double c1s[3] = {0.0, -1.0 / 12.0, -0.331};
  for (int k = 0; k < 3; k++) {
    const double c1 = c1s[k], c0 = 1.0 - 8.0 * c1, coeff = k == 1 ? -0.75 : 1.0;
    std::vector<double> want(72 * V);
    for (size_t l = 0; l < 4 * V; l++) {
      Mat m;
      for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m.a[i][j] = c0 * MP[l].a[i][j] + c1 * MR[l].a[i][j];
      const Mat md = dag(m);
      cd tr = 0;
      for (int i = 0; i < 3; i++) tr += 0.5 * (m.a[i][i] - md.a[i][i]);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          const cd e = 0.5 * (m.a[i][j] - md.a[i][j]) - (i == j ? tr / 3.0 : cd(0.0));
          want[l * 18 + 2 * (3 * i + j)] = e.real(); want[l * 18 + 2 * (3 * i + j) + 1] = e.imag();
        }
    }
    const double scale = max_abs(want);
    for (int depth = (c1 == 0.0 ? 1 : 2); depth <= 2; depth++) {
      double* out = exact_alloc(72 * V);
      for (size_t i = 0; i < 72 * V; i++) out[i] = k == 1 ? 0.25 * (double)(i % 7) : NAN;     // k == 1 accumulates onto a known field
      if (depth == 1) run_force<1>(g, U, beta, c1, coeff, k == 1, out); else run_force<2>(g, U, beta, c1, coeff, k == 1, out);
      double worst = 0;
      for (size_t i = 0; i < 72 * V; i++) {
        const double expect = k == 1 ? 0.25 * (double)(i % 7) + coeff * want[i] : want[i];
        const double d = std::fabs(out[i] - expect);
        if (!(d <= worst)) worst = d;
      }
      CHECK(worst <= 1e-13 * scale, "force c1 %g depth %d: difference %.3e of %.3e", c1, depth, worst, scale);
      printf("%s force c1 %+.4f depth %d: max |G| %.3e difference %.1e: %s\n", name, c1, depth, scale, worst, failures ? "FAILED" : "ok");
      free(out);
    }
  }
  free(U);
}

// exp of one matrix in long double: the series of a / 2^6 to 30 terms, squared back (six squarings: 64 roundings of 5e-20)
struct LMat { std::complex<long double> a[3][3]; };
static LMat lmul(const LMat& x, const LMat& y) {
  LMat r;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { r.a[i][j] = 0; for (int k = 0; k < 3; k++) r.a[i][j] += x.a[i][k] * y.a[k][j]; }
  return r;
}
static Mat series_exp(const Mat& a) {
  LMat s, out;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { s.a[i][j] = std::complex<long double>(a.a[i][j].real(), a.a[i][j].imag()) / 64.0L; out.a[i][j] = i == j ? 1.0L : 0.0L; }
  for (int d = 30; d >= 1; d--) {
    const LMat t = lmul(s, out);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) out.a[i][j] = (i == j ? 1.0L : 0.0L) + t.a[i][j] / (long double)d;
  }
  for (int k = 0; k < 6; k++) out = lmul(out, out);
  Mat r;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r.a[i][j] = cd((double)out.a[i][j].real(), (double)out.a[i][j].imag());
  return r;
}
static Mat random_algebra() {
  Mat m;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m.a[i][j] = cd(urand(), urand());
  const Mat md = dag(m);
  cd tr = 0;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m.a[i][j] = 0.5 * (m.a[i][j] - md.a[i][j]);
  for (int i = 0; i < 3; i++) tr += m.a[i][i];
  for (int i = 0; i < 3; i++) m.a[i][i] -= tr / 3.0;
  return m;
}
static double frobenius(const Mat& m) { double s = 0; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) s += std::norm(m.a[i][j]); return std::sqrt(s); }
static void store(double* p, const Mat& m) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { p[2 * (3 * i + j)] = m.a[i][j].real(); p[2 * (3 * i + j) + 1] = m.a[i][j].imag(); } }

static void run_links_and_momenta() {
  // link_update on a field of 4 V = 300 links (the last workgroup of 256 threads has a tail): arguments of Frobenius norm 0, 1e-9,
  // 1e-3, 1, 10, and degenerate ones (v diag(ia, ia, -2ia) v^dagger) of norm 1 and 10
  const size_t nlinks = 300;
  double* U = exact_alloc(18 * nlinks); double* P = exact_alloc(18 * nlinks);
  std::vector<Mat> want(nlinks);
  const double eps = -0.37;
  const double norms[5] = {0.0, 1e-9, 1e-3, 1.0, 10.0};
  for (size_t l = 0; l < nlinks; l++) {
    Mat a = random_algebra();
    if (l % 7 >= 5) {
      const Mat v = series_exp(random_algebra());
      Mat d; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) d.a[i][j] = 0;
      d.a[0][0] = d.a[1][1] = cd(0, 1); d.a[2][2] = cd(0, -2);
      a = mul(mul(v, d), dag(v));
      if (l % 14 == 5) a = d;
    }
    const double target = l % 7 < 5 ? norms[l % 7] : (l % 7 == 5 ? 1.0 : 10.0), f = frobenius(a);
    Mat arg;      // eps * p = arg
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) arg.a[i][j] = a.a[i][j] * (target / f);
    Mat p;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) p.a[i][j] = arg.a[i][j] / eps;
    const Mat u = series_exp(random_algebra());
    store(U + 18 * l, u); store(P + 18 * l, p);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) arg.a[i][j] = p.a[i][j] * eps;     // as rounded
    want[l] = mul(series_exp(arg), u);
  }
  for (size_t i = 0; i < ((nlinks + 255) / 256) * 256; i++) gmd::link_update(U, P, eps, nlinks, i);
  double worst = 0, unitarity = 0;
  for (size_t l = 0; l < nlinks; l++) {
    const Mat got = matrix_at(U + 18 * l), uu = mul(got, dag(got));
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
      worst = std::fmax(worst, std::abs(got.a[i][j] - want[l].a[i][j]));
      unitarity = std::fmax(unitarity, std::abs(uu.a[i][j] - (i == j ? 1.0 : 0.0)));
    }
  }
  CHECK(worst <= 1e-14 && unitarity <= 1e-14, "link update: difference %.3e, unitarity %.3e", worst, unitarity);
  printf("link update: against the long double series %.1e, |U U^+ - 1| %.1e: %s\n", worst, unitarity, failures ? "FAILED" : "ok");

  // link_reunitarize: perturbed links come back unitary with determinant one, the deviation is the one before, a projected field is
  // a fixed point
  std::vector<double> before(18 * nlinks);
  double dev_want = 0;
  for (size_t l = 0; l < nlinks; l++) {
    for (int k = 0; k < 18; k++) U[18 * l + k] += 2e-6 * urand();
    const Mat u = matrix_at(U + 18 * l), uu = mul(u, dag(u));
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) dev_want = std::fmax(dev_want, std::abs(uu.a[i][j] - (i == j ? 1.0 : 0.0)));
  }
  for (size_t i = 0; i < 18 * nlinks; i++) before[i] = U[i];
  double dev = 0, moved = 0, det_err = 0;
  for (size_t i = 0; i < ((nlinks + 255) / 256) * 256; i++) dev = std::fmax(dev, gmd::link_reunitarize(U, nlinks, i));
  unitarity = 0;
  for (size_t l = 0; l < nlinks; l++) {
    const Mat u = matrix_at(U + 18 * l), uu = mul(u, dag(u));
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) unitarity = std::fmax(unitarity, std::abs(uu.a[i][j] - (i == j ? 1.0 : 0.0)));
    const cd det = u.a[0][0] * (u.a[1][1] * u.a[2][2] - u.a[1][2] * u.a[2][1]) - u.a[0][1] * (u.a[1][0] * u.a[2][2] - u.a[1][2] * u.a[2][0]) +
                   u.a[0][2] * (u.a[1][0] * u.a[2][1] - u.a[1][1] * u.a[2][0]);
    det_err = std::fmax(det_err, std::abs(det - 1.0));
  }
  for (size_t i = 0; i < 18 * nlinks; i++) moved = std::fmax(moved, std::fabs(U[i] - before[i]));
  const double e = 2.220446049250313e-16;
  CHECK(std::fabs(dev - dev_want) <= 1e-12 * dev_want && dev_want > 1e-7, "deviation %.6e, brute force %.6e", dev, dev_want);
  CHECK(unitarity <= 4 * e && det_err <= 8 * e && moved < 1e-5, "reunitarised: |U U^+ - 1| %.3e |det - 1| %.3e moved %.3e", unitarity, det_err, moved);
  for (size_t i = 0; i < 18 * nlinks; i++) before[i] = U[i];
  double again = 0;
  for (size_t i = 0; i < nlinks; i++) again = std::fmax(again, gmd::link_reunitarize(U, nlinks, i));
  moved = 0;
  for (size_t i = 0; i < 18 * nlinks; i++) moved = std::fmax(moved, std::fabs(U[i] - before[i]));
  CHECK(again <= 4 * e && moved <= 4 * e, "a projected field moved by %.3e, deviation %.3e", moved, again);
  printf("reunitarisation: deviation %.3e (brute force %.3e), then |U U^+ - 1| %.1e |det - 1| %.1e, fixed point %.1e: %s\n", dev, dev_want, unitarity, det_err,
         moved, failures ? "FAILED" : "ok");

  // momentum_update and kinetic_part on n = 18 * 300 = 5400 reals: two full workgroups of the kinetic kernel and a tail
  const size_t n = 18 * nlinks;
  double* F = exact_alloc(n);
  std::vector<double> p0(n);
  long double kin = 0;
  for (size_t i = 0; i < n; i++) { F[i] = urand(); p0[i] = P[i]; }
  for (size_t i = 0; i < ((n + 255) / 256) * 256; i++) gmd::momentum_update(P, F, 0.125, n, i);
  worst = 0;
  for (size_t i = 0; i < n; i++) { worst = std::fmax(worst, std::fabs(P[i] - (p0[i] + 0.125 * F[i]))); kin += (long double)P[i] * P[i]; }
  double sum = 0;
  const size_t per_block = (size_t)gmd::REDUCE_THREADS * gmd::KINETIC_BATCH;
  for (size_t b = 0; b < (n + per_block - 1) / per_block; b++)
    for (int tid = 0; tid < gmd::REDUCE_THREADS; tid++) sum += gmd::kinetic_part(P, n, b, tid);
  CHECK(worst == 0.0, "momentum update differs by %.3e", worst);
  CHECK(std::fabs(sum - (double)kin) <= 1e-13 * (double)kin, "sum of squares %.15e, brute force %.15e", sum, (double)kin);
  printf("momenta: update exact, sum of squares %.12e (difference %.1e): %s\n", sum, std::fabs(sum - (double)kin), failures ? "FAILED" : "ok");
  free(F); free(U); free(P);
}

int main() {
  const int L1[4] = {4, 4, 4, 4}, L2[4] = {4, 6, 8, 10}, L3[4] = {4, 4, 12, 12};
  run_lattice("4^4", L1);
  run_lattice("4x6x8x10", L2);
  run_lattice("4x4x12x12", L3);
  run_links_and_momenta();
  if (failures) { printf("%d comparisons FAILED\n", failures); return 1; }
  printf("GAUGE_MD_OK\n");
  return 0;
}
