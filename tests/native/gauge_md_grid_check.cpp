// gauge_md_grid_check.cpp -- a stand-alone host program (no GPU, no HIP) over the gauge sector on a process grid: the link shell of
// depth 1 and 2 (fs::make_shell, fs::make_slab, fs::slab_at, fs::extend_links, fs::slab_copy of csrc/field_strength.h, in the exchange
// order of ExtendedLinks::fill) and the extended forms of the plane kernels' bodies (gmd::stage_offsets with a shell, gmd::stage_links,
// gmd::site_gauge_force, gmd::site_gauge_loops of csrc/gauge_md.h, force::site_assemble behind them), run thread by thread as
// gauge_force_kernel<H> and gauge_loops_kernel<H> run them.  tests/test_gauge_md_grid_native.py builds it with the host compiler under
// -fsanitize=address,undefined and runs it; it prints GAUGE_MD_GRID_OK and exits 0 when every comparison held.
//
// Process grids are emulated: every emulated process cuts its part out of a periodic global field, builds its extended array, and
// the messages are memcpys between the processes' buffers.  Every array is exactly as large as the library makes it, so a load
// outside the extended array is the sanitizer's finding.  The reference is the brute force of gauge_md_check.cpp on the GLOBAL
// lattice: every plaquette and rectangle walked as a closed path, the rotation that starts at each factor given to that factor's
// link.  Links are random complex matrices, not unitary ones, so that no cancellation hides a misplaced factor.
#include "gauge_md.h"
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static double* exact_alloc(size_t doubles) {   // 16-byte aligned and not a byte longer than asked for: the sanitizer guards both ends
  void* p = aligned_alloc(16, ((doubles * sizeof(double) + 15) / 16) * 16);
  if (!p) { printf("out of memory\n"); exit(2); }
  return static_cast<double*>(p);
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

// a periodic global lattice with its links and the brute force on it: the sums, and M of the plaquette part and of the rectangle
// part with weight -beta/3
static const double BETA = 5.6;
struct Global {
  Lattice g;
  std::vector<double> U;
  std::vector<Mat> MP, MR;
  double plaq = 0, rect = 0;
  explicit Global(const int G[4]) {
    g.V = 1;
    for (int d = 0; d < 4; d++) { g.L[d] = G[d]; g.V *= (size_t)G[d]; }
    const size_t V = g.V;
    U.resize(72 * V);
    for (double& v : U) v = urand();
    MP.resize(4 * V);
    for (auto& m : MP) for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m.a[i][j] = 0;
    MR = MP;
    for (size_t ly = 0; ly < V; ly++) {
      int y[4]; g.coords(ly, y);
      for (int mu = 0; mu < 4; mu++)
        for (int nu = 0; nu < 4; nu++) {
          if (nu == mu) continue;
          if (mu < nu) { const int s[4] = {1 + mu, 1 + nu, -1 - mu, -1 - nu}; brute_force_loop(g, U.data(), y, s, 4, -BETA / 3.0, &plaq, MP); }
          const int s[6] = {1 + mu, 1 + mu, 1 + nu, -1 - mu, -1 - mu, -1 - nu};
          brute_force_loop(g, U.data(), y, s, 6, -BETA / 3.0, &rect, MR);
        }
    }
  }
  // G = TA(c0 MP + c1 MR) of every link, [V][4][18]
  std::vector<double> force(double c1) const {
    const double c0 = 1.0 - 8.0 * c1;
    std::vector<double> want(72 * g.V);
    for (size_t l = 0; l < 4 * g.V; l++) {
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
    return want;
  }
};

// the emulated process grid: P processes per direction; a direction is split where P > 1 or where the process is its own neighbour
struct Grid {
  int L[4], P[4]; bool split[4];
  int nranks;
};
static int rank_of(const int P[4], const int pc[4]) { return ((pc[0] * P[1] + pc[1]) * P[2] + pc[2]) * P[3] + pc[3]; }
static void coords_of(const int P[4], int r, int pc[4]) { for (int d = 3; d >= 0; d--) { pc[d] = r % P[d]; r /= P[d]; } }
// as Geometry::build: direction d < 4 is +mu, 4 + mu is -mu
static int neighbor_rank(const Grid& g, int rank, int d) {
  int q[4]; coords_of(g.P, rank, q);
  const int mu = d & 3;
  q[mu] = d < 4 ? (q[mu] + 1) % g.P[mu] : (q[mu] - 1 + g.P[mu]) % g.P[mu];
  return rank_of(g.P, q);
}

struct Rank {
  int O[4];                       // global coordinates of the first own site
  double* U = nullptr;            // the process's links [V][72]
  double* Ue = nullptr; double* sbuf = nullptr; double* rbuf = nullptr;
};

static const double POISON = -7.0e300;

// the extended arrays of every process at one depth, as ExtendedLinks::fill builds them; the bytes of every message are checked
// against the formula of docs/design/06_multi_gpu.md, and the arrays against the global lattice
static void exchange(const char* name, const Grid& g, const Global& glob, const fs::Shell& sh, int depth, std::vector<Rank>& ranks) {
  const size_t V = sh.V, Ve = sh.Ve;
  size_t most = 1;
  for (int mu = 0; mu < 4; mu++) if (sh.h[mu]) { const size_t n = fs::make_slab(sh, mu).sites; if (n > most) most = n; }
  for (Rank& k : ranks) {
    k.Ue = exact_alloc(Ve * 72); k.sbuf = exact_alloc(most * 72); k.rbuf = exact_alloc(most * 72);
    for (size_t i = 0; i < Ve * 72; i++) k.Ue[i] = POISON;
    for (size_t i = 0; i < most * 72; i++) k.sbuf[i] = k.rbuf[i] = POISON;
    const size_t n = ((V * 36 + 255) / 256) * 256;     // links_extend_kernel: whole workgroups of 256 threads
    for (size_t i = 0; i < n; i++) fs::extend_links<2>(sh, k.U, k.Ue, i, 0);
  }
  int messages = 0; size_t bytes = 0;
  for (int mu = 0; mu < 4; mu++) {
    if (!sh.h[mu]) continue;
    CHECK(sh.h[mu] == depth && g.L[mu] >= depth, "%s: direction %d: shell %d deep on a local extent of %d", name, mu, sh.h[mu], g.L[mu]);
    const fs::Slab slab = fs::make_slab(sh, mu);
    CHECK(slab.n[mu] == depth, "%s: the slab of direction %d is %d sites thick", name, mu, slab.n[mu]);
    size_t formula = (size_t)72 * 8 * depth;
    for (int d = 0; d < 4; d++) if (d != mu) formula *= (size_t)((d < mu && g.split[d]) ? g.L[d] + 2 * depth : g.L[d]);
    const size_t threads = ((slab.sites * 36 + 255) / 256) * 256;
    for (int side = 0; side < 2; side++) {
      const int src_c = side == 0 ? g.L[mu] - depth : 0, dst_c = side == 0 ? -depth : g.L[mu];
      const fs::Slab from = fs::slab_at(sh, slab, src_c), to = fs::slab_at(sh, slab, dst_c);
      for (Rank& k : ranks) for (size_t i = 0; i < threads; i++) fs::slab_copy(sh, from, k.Ue, k.sbuf, i, true);
      const size_t copied = slab.sites * 72 * sizeof(double);
      for (int r = 0; r < g.nranks; r++) {
        const int send_peer = neighbor_rank(g, r, side == 0 ? mu : 4 + mu);
        CHECK(neighbor_rank(g, send_peer, side == 0 ? 4 + mu : mu) == r, "%s: rank %d sends to %d, which receives from another rank", name, r, send_peer);
        memcpy(ranks[send_peer].rbuf, ranks[r].sbuf, copied);
      }
      CHECK(copied == formula, "%s: direction %d depth %d: a message of %zu bytes, the formula gives %zu", name, mu, depth, copied, formula);
      messages++; bytes += copied;
      for (Rank& k : ranks) for (size_t i = 0; i < threads; i++) fs::slab_copy(sh, to, k.Ue, k.rbuf, i, false);
    }
  }
  int nsplit = 0;
  for (int mu = 0; mu < 4; mu++) nsplit += g.split[mu] ? 1 : 0;
  CHECK(messages == 2 * nsplit, "%s: %d messages per process for %d split directions", name, messages, nsplit);
  // the whole extended array against the global lattice, corners of every order included
  size_t wrong = 0;
  for (const Rank& k : ranks)
    for (size_t e = 0; e < Ve; e++) {
      int X[4]; size_t q = e;
      for (int d = 3; d >= 0; d--) { X[d] = (int)(q % sh.E[d]) - sh.h[d] + k.O[d]; q /= sh.E[d]; }
      wrong += memcmp(k.Ue + e * 72, glob.U.data() + glob.g.lex(X) * 72, 72 * sizeof(double)) != 0;
    }
  CHECK(wrong == 0, "%s depth %d: %zu sites of the extended arrays differ from the global lattice", name, depth, wrong);
  printf("%s shell of depth %d: %d messages of %zu bytes in all per process, extended array %zu sites for %zu own: %s\n", name, depth, messages, bytes, Ve, V,
         failures ? "FAILED" : "ok");
}

static void release(std::vector<Rank>& ranks) {
  for (Rank& k : ranks) { free(k.Ue); free(k.sbuf); free(k.rbuf); k.Ue = k.sbuf = k.rbuf = nullptr; }
}

// gauge_force_kernel<H> and gauge_force_assemble_kernel of one process, thread by thread
template <int H>
static void run_force(const fs::Shell& sh, const double* Ue, double c1, double coeff, int accumulate, double* out) {
  const fs::Planes planes = fs::make_planes(sh.L);
  const size_t V = sh.V, nslots = (size_t)4 * force::SLOTS * 9 * V;
  double* slots = exact_alloc(nslots);
  for (size_t i = 0; i < nslots; i++) slots[i] = NAN;     // a slot nobody writes poisons the force
  double* lds = exact_alloc(gmd::Nb<H>::LDS_DOUBLES);
  size_t off[2 * gmd::Nb<H>::EXT];
  std::vector<int> writers(4 * 3 * V, 0);
  for (int p = 0; p < 6; p++)
    for (int block = 0; block < planes.nblocks[p]; block++) {
      const fs::Tile t = fs::tile_of(planes, p, block);
      const fs::Tile te = fs::extended_tile(planes, sh, t, block);
      for (int tid = 0; tid < fs::THREADS; tid++) gmd::stage_offsets<H>(planes, te, sh, tid, off);
      for (int i = 0; i < gmd::Nb<H>::LDS_DOUBLES; i++) lds[i] = NAN;
      for (int tid = 0; tid < fs::THREADS; tid++) gmd::stage_links<H>(Ue, te, tid, off, lds);     // reads inside Ue only: the sanitizer watches
      for (int tid = 0; tid < fs::THREADS; tid++) {
        size_t lex = 0; double o[2][9];
        if (!gmd::site_gauge_force<H>(planes, t, tid, lds, BETA, 1.0 - 8.0 * c1, c1, &lex, o)) continue;
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

// gauge_loops_kernel<H> of one process: its sums
template <int H>
static void run_loops(const fs::Shell& sh, const double* Ue, double* plaq, double* rect) {
  const fs::Planes planes = fs::make_planes(sh.L);
  double* lds = exact_alloc(gmd::Nb<H>::LDS_DOUBLES);
  size_t off[2 * gmd::Nb<H>::EXT];
  *plaq = 0; *rect = 0;
  for (int p = 0; p < 6; p++)
    for (int block = 0; block < planes.nblocks[p]; block++) {
      const fs::Tile t = fs::tile_of(planes, p, block);
      const fs::Tile te = fs::extended_tile(planes, sh, t, block);
      for (int tid = 0; tid < fs::THREADS; tid++) gmd::stage_offsets<H>(planes, te, sh, tid, off);
      for (int i = 0; i < gmd::Nb<H>::LDS_DOUBLES; i++) lds[i] = NAN;
      for (int tid = 0; tid < fs::THREADS; tid++) gmd::stage_links<H>(Ue, te, tid, off, lds);
      for (int tid = 0; tid < fs::THREADS; tid++) {
        double pl, re;
        gmd::site_gauge_loops<H>(planes, t, tid, lds, &pl, &re);
        *plaq += pl; *rect += re;
      }
    }
  free(lds);
}

// one emulated grid on the global lattice: P processes per direction; self: the directions ("TZYX") in which a process is split
// with itself as its neighbour
static void run_case(const char* name, const Global& glob, const int P[4], const char* self) {
  Grid g; g.nranks = 1;
  for (int d = 0; d < 4; d++) {
    g.P[d] = P[d]; g.L[d] = glob.g.L[d] / P[d]; g.nranks *= P[d];
    g.split[d] = P[d] > 1 || strchr(self, "TZYX"[d]) != nullptr;
    if (g.L[d] * P[d] != glob.g.L[d]) { printf("%s: the grid does not divide the lattice\n", name); exit(2); }
  }
  size_t V = 1;
  for (int d = 0; d < 4; d++) V *= (size_t)g.L[d];
  std::vector<Rank> ranks(g.nranks);
  for (int r = 0; r < g.nranks; r++) {
    Rank& k = ranks[r];
    int pc[4]; coords_of(g.P, r, pc);
    for (int d = 0; d < 4; d++) k.O[d] = pc[d] * g.L[d];
    k.U = exact_alloc(V * 72);
    for (size_t lx = 0; lx < V; lx++) {
      int x[4]; size_t q = lx;
      for (int d = 3; d >= 0; d--) { x[d] = (int)(q % g.L[d]) + k.O[d]; q /= g.L[d]; }
      memcpy(k.U + lx * 72, glob.U.data() + glob.g.lex(x) * 72, 72 * sizeof(double));
    }
  }
  const double c1s[3] = {0.0, -1.0 / 12.0, -0.331};
  for (int depth = 1; depth <= 2; depth++) {
    const fs::Shell sh = fs::make_shell(g.L, g.split, depth);
    exchange(name, g, glob, sh, depth, ranks);
    for (int k = 0; k < 3; k++) {
      const double c1 = c1s[k], coeff = k == 1 ? -0.75 : 1.0;
      if ((c1 == 0.0 ? 1 : 2) != depth) continue;     // the depth follows the action
      const std::vector<double> want = glob.force(c1);
      double scale = 0;
      for (double v : want) scale = std::fabs(v) > scale ? std::fabs(v) : scale;
      double worst = 0, plaq = 0, rect = 0;
      for (const Rank& rk : ranks) {
        double* out = exact_alloc(72 * V);
        for (size_t i = 0; i < 72 * V; i++) out[i] = k == 1 ? 0.25 * (double)(i % 7) : NAN;     // k == 1 accumulates onto a known field
        double pl, re;
        if (depth == 1) { run_force<1>(sh, rk.Ue, c1, coeff, k == 1, out); run_loops<1>(sh, rk.Ue, &pl, &re); CHECK(re == 0.0, "%s: a rectangle sum at depth 1", name); }
        else { run_force<2>(sh, rk.Ue, c1, coeff, k == 1, out); run_loops<2>(sh, rk.Ue, &pl, &re); }
        plaq += pl; rect += re;
        for (size_t lx = 0; lx < V; lx++) {
          int x[4]; size_t q = lx;
          for (int d = 3; d >= 0; d--) { x[d] = (int)(q % g.L[d]) + rk.O[d]; q /= g.L[d]; }
          const size_t gx = glob.g.lex(x);
          for (int i = 0; i < 72; i++) {
            const double w = want[gx * 72 + i];
            const double expect = k == 1 ? 0.25 * (double)((lx * 72 + i) % 7) + coeff * w : w;
            const double d = std::fabs(out[lx * 72 + i] - expect);
            if (!(d <= worst)) worst = d;
          }
        }
        free(out);
      }
      const double Vg = (double)glob.g.V;
      CHECK(worst <= 1e-13 * scale, "%s force c1 %g depth %d: difference %.3e of %.3e", name, c1, depth, worst, scale);
      printf("%s force c1 %+.4f depth %d: max |G| %.3e difference %.1e: %s\n", name, c1, depth, scale, worst, failures ? "FAILED" : "ok");
      CHECK(std::fabs(plaq - glob.plaq) <= 1e-13 * Vg, "%s: plaquette sum %.15e, brute force %.15e", name, plaq, glob.plaq);
      if (depth == 2) CHECK(std::fabs(rect - glob.rect) <= 1e-13 * Vg, "%s: rectangle sum %.15e, brute force %.15e", name, rect, glob.rect);
      printf("%s loops c1 %+.4f depth %d: plaquette difference %.1e, rectangle difference %.1e: %s\n", name, c1, depth, std::fabs(plaq - glob.plaq),
             depth == 2 ? std::fabs(rect - glob.rect) : 0.0, failures ? "FAILED" : "ok");
    }
    release(ranks);
  }
  for (Rank& k : ranks) free(k.U);
}

int main() {
  {
    const int G[4] = {4, 4, 8, 12};
    const Global glob(G);
    const int a[4] = {2, 1, 1, 1}, b[4] = {1, 1, 2, 2}, c[4] = {2, 2, 2, 2};
    run_case("4x4x8x12 on 2,1,1,1 (T = 2: the depth-2 shell is the whole neighbour)", glob, a, "");
    run_case("4x4x8x12 on 1,1,2,2 (corners of the (Y, X) plane from the diagonal process)", glob, b, "");
    run_case("4x4x8x12 on 2,2,2,2 (all four directions split)", glob, c, "");
  }
  {
    const int G[4] = {4, 6, 8, 10};
    const Global glob(G);
    const int one[4] = {1, 1, 1, 1};
    run_case("4x6x8x10, every direction split with the process its own neighbour (tile tails)", glob, one, "TZYX");
  }
  if (failures) { printf("%d comparisons FAILED\n", failures); return 1; }
  printf("GAUGE_MD_GRID_OK\n");
  return 0;
}
