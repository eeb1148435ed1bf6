// force_shell_check.cpp -- a stand-alone host program (no GPU, no HIP) over the kernel bodies of csrc/force.h and
// csrc/field_strength.h that the force on a process grid adds or uses in a new way: extended_site, tensor_slab_copy (pack and
// unpack), and extended_tile / stage_offsets<true> / stage_links / stage_tensor / site_clover_derivative on the extended arrays,
// run thread by thread as the kernels of force.hip run them.  tests/test_force_shell_native.py builds it with the host compiler
// under -fsanitize=address,undefined and runs it; it prints FORCE_SHELL_OK and exits 0 when every comparison held.
//
// A process grid is emulated inside the program: every rank has its own arrays and a message is a memcpy that follows
// neighbor_rank.  Two passes per case:
//   tags  every real of A carries its global site, plane and component as its value: the whole extended array, and every real
//         that stage_tensor stages for a site of the lattice (its 3 x 3 neighbourhood in the plane, the corners included), must be
//         the one the periodic global lattice holds there;
//   bits  random W and A: site_clover_derivative on the emulated ranks gives the bits of the same bodies on the undivided
//         lattice -- the same function on the same numbers.
#include "force.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ddamg;

static int failures = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (failures < 20) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
      failures++;                                                              \
    }                                                                          \
  } while (0)

static const double POISON = -7.0e300;

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

struct Grid {
  int L[4], P[4], G[4]; bool split[4];
  int nranks; size_t GV;
  size_t global_site(const int X[4]) const {   // periodic
    int w[4];
    for (int d = 0; d < 4; d++) w[d] = ((X[d] % G[d]) + G[d]) % G[d];
    return (((size_t)w[0] * G[1] + w[1]) * G[2] + w[2]) * G[3] + w[3];
  }
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
  int O[4];
  double* W = nullptr;       // own links [V][72]
  double* We = nullptr;      // extended links [Ve][72]
  double* Ae = nullptr;      // extended tensor [54][Ve]
  double* sbuf = nullptr; double* rbuf = nullptr;
};

// the shell of every rank's Ae (tensor != 0) or We, direction by direction and side by side, as exchange_tensor_shell and
// ExtendedLinks::fill do; the kernels run whole workgroups of 256 threads, so some threads lie beyond the last element
static void exchange_shell(const char* name, const Grid& g, const fs::Shell& sh, std::vector<Rank>& ranks, bool tensor) {
  const size_t per_site = tensor ? 54 : 72, threads_per_site = tensor ? 54 : 36;
  for (int mu = 0; mu < 4; mu++) {
    if (!sh.h[mu]) continue;
    const fs::Slab slab = fs::make_slab(sh, mu);
    const size_t threads = ((slab.sites * threads_per_site + 255) / 256) * 256;
    for (int side = 0; side < 2; side++) {
      const int src_c = side == 0 ? g.L[mu] - 1 : 0, dst_c = side == 0 ? -1 : g.L[mu];
      const fs::Slab from = fs::slab_at(sh, slab, src_c), to = fs::slab_at(sh, slab, dst_c);
      for (Rank& k : ranks)
        for (size_t i = 0; i < threads; i++) {
          if (tensor) force::tensor_slab_copy(sh, from, k.Ae, k.sbuf, i, true); else fs::slab_copy(sh, from, k.We, k.sbuf, i, true);
        }
      for (int r = 0; r < g.nranks; r++) {
        const int send_peer = neighbor_rank(g, r, side == 0 ? mu : 4 + mu);
        CHECK(neighbor_rank(g, send_peer, side == 0 ? 4 + mu : mu) == r, "%s: rank %d sends to %d, which receives from another rank", name, r, send_peer);
        memcpy(ranks[send_peer].rbuf, ranks[r].sbuf, slab.sites * per_site * sizeof(double));
      }
      for (Rank& k : ranks)
        for (size_t i = 0; i < threads; i++) {
          if (tensor) force::tensor_slab_copy(sh, to, k.Ae, k.rbuf, i, false); else fs::slab_copy(sh, to, k.We, k.rbuf, i, false);
        }
    }
  }
}

static double tag(size_t global_site, int comp) { return (double)(global_site * 54 + comp + 1); }

static void run_case(const char* name, const int L[4], const int P[4], const char* split_dirs) {
  Grid g; g.nranks = 1; g.GV = 1;
  for (int d = 0; d < 4; d++) {
    g.L[d] = L[d]; g.P[d] = P[d]; g.G[d] = L[d] * P[d]; g.nranks *= P[d]; g.GV *= (size_t)g.G[d];
    g.split[d] = P[d] > 1 || strchr(split_dirs, "TZYX"[d]) != nullptr;
  }
  const int before = failures;
  const fs::Shell sh = fs::make_shell(g.L, g.split);
  const fs::Planes planes = fs::make_planes(g.L), gplanes = fs::make_planes(g.G);
  const size_t V = sh.V, Ve = sh.Ve, GV = g.GV;
  size_t most = 1;
  for (int mu = 0; mu < 4; mu++) if (sh.h[mu]) { const size_t n = fs::make_slab(sh, mu).sites; if (n > most) most = n; }

  // the global fields of the second pass, and the derivative on the undivided lattice: gout[((p * GV + site) * 2 + w) * 9 + r]
  double* GW = exact_alloc(GV * 72); double* GA = exact_alloc(GV * 54);
  for (size_t i = 0; i < GV * 72; i++) GW[i] = urand();
  for (size_t i = 0; i < GV * 54; i++) GA[i] = urand();
  std::vector<double> gout(GV * 6 * 18, POISON);
  double* lds = exact_alloc(fs::LDS_DOUBLES); double* lds_a = exact_alloc(force::LDS_A_DOUBLES);
  size_t off[2 * fs::EXT]; int flip[fs::EXT];
  for (int p = 0; p < 6; p++)
    for (int block = 0; block < gplanes.nblocks[p]; block++) {
      const fs::Tile t = fs::tile_of(gplanes, p, block);
      for (int tid = 0; tid < fs::THREADS; tid++) fs::stage_offsets(gplanes, t, 0, tid, off, flip);
      for (int tid = 0; tid < fs::THREADS; tid++) { fs::stage_links(GW, t, tid, off, flip, lds); force::stage_tensor(GA, GV, p, t, tid, off, lds_a); }
      for (int tid = 0; tid < fs::THREADS; tid++) {
        size_t lx = 0; double o[2][9];
        if (force::site_clover_derivative(gplanes, t, tid, lds, lds_a, &lx, o)) memcpy(&gout[((size_t)p * GV + lx) * 18], o, sizeof o);
      }
    }

  std::vector<Rank> ranks(g.nranks);
  for (int r = 0; r < g.nranks; r++) {
    Rank& k = ranks[r];
    int pc[4]; coords_of(g.P, r, pc);
    for (int d = 0; d < 4; d++) k.O[d] = pc[d] * g.L[d];
    k.W = exact_alloc(V * 72); k.We = exact_alloc(Ve * 72); k.Ae = exact_alloc(Ve * 54);
    k.sbuf = exact_alloc(most * 72); k.rbuf = exact_alloc(most * 72);
  }
  // the global site of site e of a rank's extended array
  auto global_of_extended = [&](const Rank& k, size_t e) {
    int X[4]; size_t q = e;
    for (int d = 3; d >= 0; d--) { X[d] = (int)(q % sh.E[d]) - sh.h[d] + k.O[d]; q /= sh.E[d]; }
    return g.global_site(X);
  };
  auto global_of_own = [&](const Rank& k, size_t lx) {
    int X[4]; size_t q = lx;
    for (int d = 3; d >= 0; d--) { X[d] = (int)(q % g.L[d]) + k.O[d]; q /= g.L[d]; }
    return g.global_site(X);
  };

  for (int pass = 0; pass < 2; pass++) {   // 0: tags, 1: bits
    for (Rank& k : ranks) {
      for (size_t i = 0; i < Ve * 72; i++) k.We[i] = POISON;
      for (size_t i = 0; i < Ve * 54; i++) k.Ae[i] = POISON;
      for (size_t i = 0; i < most * 72; i++) k.sbuf[i] = k.rbuf[i] = POISON;
      // the interior: W by links_extend_kernel, A where the tensor kernels write it (fs::extended_site)
      for (size_t lx = 0; lx < V; lx++) {
        const size_t gs = global_of_own(k, lx), e = fs::extended_site(sh, lx);
        CHECK(e < Ve, "%s: extended_site outside the extended array", name);
        memcpy(k.W + lx * 72, GW + gs * 72, 72 * sizeof(double));
        for (int c = 0; c < 54; c++) {
          CHECK(k.Ae[(size_t)c * Ve + e] == POISON, "%s: two sites share a place in the extended array", name);
          k.Ae[(size_t)c * Ve + e] = pass == 0 ? tag(gs, c) : GA[(size_t)c * GV + gs];
        }
      }
      const size_t n = ((V * 36 + 255) / 256) * 256;
      for (size_t i = 0; i < n; i++) fs::extend_links<2>(sh, k.W, k.We, i, 0);
    }
    exchange_shell(name, g, sh, ranks, false);
    exchange_shell(name, g, sh, ranks, true);

    for (int r = 0; r < g.nranks; r++) {
      Rank& k = ranks[r];
      if (pass == 0) {
        size_t wrong = 0, unwritten = 0;
        for (size_t e = 0; e < Ve; e++) {
          const size_t gs = global_of_extended(k, e);
          for (int c = 0; c < 54; c++) { unwritten += k.Ae[(size_t)c * Ve + e] == POISON; wrong += k.Ae[(size_t)c * Ve + e] != tag(gs, c); }
        }
        CHECK(unwritten == 0, "%s: rank %d: %zu reals of the extended tensor were never written", name, r, unwritten);
        CHECK(wrong == 0, "%s: rank %d: %zu reals of the extended tensor differ from the global lattice", name, r, wrong);
      }
      std::vector<int> visits(V * 6, 0);
      for (int p = 0; p < 6; p++)
        for (int block = 0; block < planes.nblocks[p]; block++) {
          const fs::Tile t = fs::tile_of(planes, p, block);
          const fs::Tile te = fs::extended_tile(planes, sh, t, block);
          for (int i = 0; i < fs::LDS_DOUBLES; i++) lds[i] = POISON;
          for (int i = 0; i < force::LDS_A_DOUBLES; i++) lds_a[i] = POISON;
          for (int tid = 0; tid < fs::THREADS; tid++) fs::stage_offsets<true>(planes, te, 0, tid, off, flip, &sh);
          for (int tid = 0; tid < fs::THREADS; tid++) {   // reads inside We and Ae only: the sanitizer watches
            fs::stage_links(k.We, te, tid, off, flip, lds);
            force::stage_tensor(k.Ae, Ve, p, te, tid, off, lds_a);
          }
          for (int tid = 0; tid < fs::THREADS; tid++) {
            const int a = tid / fs::TILE, b = tid % fs::TILE;
            const bool inside = t.a0 + a < g.L[t.mu] && t.b0 + b < g.L[t.nu];
            size_t lx = 0; double o[2][9];
            const bool did = force::site_clover_derivative(planes, t, tid, lds, lds_a, &lx, o);
            CHECK(did == inside, "%s: thread %d of a tile at (%d, %d) %s", name, tid, t.a0, t.b0, did ? "computes outside the lattice" : "skips a site");
            if (!did || !inside) continue;
            CHECK(lx < V, "%s: the slots would be written outside the own lattice", name);
            if (lx >= V) continue;
            visits[(size_t)p * V + lx]++;
            int x[4]; size_t q = lx;
            for (int d = 3; d >= 0; d--) { x[d] = (int)(q % g.L[d]); q /= g.L[d]; }
            CHECK(x[t.mu] == t.a0 + a && x[t.nu] == t.b0 + b, "%s: the output index is not the thread's site", name);
            if (pass == 0) {
              // the 3 x 3 neighbourhood of the site in the plane: the corners of both plaquettes of both links lie in it
              for (int da = -1; da <= 1; da++)
                for (int db = -1; db <= 1; db++) {
                  int X[4] = {x[0] + k.O[0], x[1] + k.O[1], x[2] + k.O[2], x[3] + k.O[3]};
                  X[t.mu] += da; X[t.nu] += db;
                  const size_t gs = g.global_site(X);
                  const int e = (a + 1 + da) * fs::EXT + (b + 1 + db);
                  for (int c = 0; c < 9; c++) {
                    const double got = lds_a[e * force::APITCH + c], want = tag(gs, p * 9 + c);
                    CHECK(got == want, "%s: rank %d plane %d site (%d %d %d %d): A at (%+d, %+d) real %d is %.0f, the global lattice holds %.0f", name, r, p,
                          x[0], x[1], x[2], x[3], da, db, c, got, want);
                  }
                }
            } else {
              const size_t gs = global_of_own(k, lx);
              CHECK(memcmp(o, &gout[((size_t)p * GV + gs) * 18], sizeof o) == 0,
                    "%s: rank %d plane %d site (%d %d %d %d): the derivative differs in its bits from the undivided lattice's", name, r, p, x[0], x[1], x[2], x[3]);
            }
          }
        }
      size_t not_once = 0;
      for (int v : visits) not_once += v != 1;
      CHECK(not_once == 0, "%s: rank %d: %zu (site, plane) pairs are not computed exactly once", name, r, not_once);
    }
  }
  for (Rank& k : ranks) { free(k.W); free(k.We); free(k.Ae); free(k.sbuf); free(k.rbuf); }
  free(GW); free(GA); free(lds); free(lds_a);
  printf("%-44s local %dx%dx%dx%d grid %dx%dx%dx%d split %-4s: %s\n", name, L[0], L[1], L[2], L[3], P[0], P[1], P[2], P[3], split_dirs,
         failures == before ? "ok" : "FAILED");
}

int main() {
  const int one[4] = {1, 1, 1, 1};
  const int L4[4] = {4, 4, 4, 4}, Lr[4] = {2, 4, 6, 4}, Lbig[4] = {4, 6, 8, 10};   // Lr: extent 2; Lbig: tile tails
  // the process as its own neighbour in the split directions
  run_case("4^4, T", L4, one, "T");
  for (const char* s : {"T", "X", "TY", "TZYX"}) run_case("2x4x6x4, its own neighbour", Lr, one, s);
  run_case("4x6x8x10, a wrapped and a shell direction", Lbig, one, "ZX");
  run_case("4x6x8x10, all four", Lbig, one, "TZYX");
  // emulated process grids: corners from a diagonal rank
  const int Pt[4] = {2, 1, 1, 1}, Px[4] = {1, 1, 1, 2}, Ptz[4] = {2, 2, 1, 1}, Pall[4] = {2, 2, 2, 2};
  run_case("grid 2x1x1x1", L4, Pt, "");
  run_case("grid 2x1x1x1", Lr, Pt, "");
  run_case("grid 1x1x1x2", Lr, Px, "");
  run_case("grid 1x1x1x2, tile tails", Lbig, Px, "");
  run_case("grid 2x2x1x1", Lr, Ptz, "");
  run_case("grid 2x2x1x1, the rest its own neighbour", Lbig, Ptz, "YX");
  run_case("grid 2x2x2x2", L4, Pall, "");
  run_case("grid 2x2x2x2", Lr, Pall, "");
  if (failures) { printf("%d comparisons failed\n", failures); return 1; }
  printf("FORCE_SHELL_OK\n");
  return 0;
}
