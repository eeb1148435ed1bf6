// link_shell_check.cpp -- a stand-alone host program (no GPU, no HIP) over the kernel bodies of csrc/field_strength.h that take links
// in device memory on a process grid: extend_links, slab_copy (pack and unpack), extended_tile, stage_offsets<true>, stage_links and
// site_field_strength, run thread by thread as the kernels of gauge_device.hip run them.  tests/test_link_shell_native.py builds it
// with the host compiler under -fsanitize=address,undefined and runs it; it prints LINK_SHELL_OK and exits 0 when every comparison
// held.
//
// Every real of every link carries its own global site, direction and component as its value, so a factor that a leaf reads can be
// compared with the link a brute-force periodic GLOBAL lattice holds at that place, the anti-periodic sign included.  A process grid
// is emulated inside the program: every rank has its own arrays and a message is a memcpy that follows neighbor_rank, which tells a
// diagonal neighbour from oneself, a wrong peer from the right one and a slab that is off by one from the one that was meant.
#include "field_strength.h"
#include <cmath>
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

struct Grid {
  int L[4], P[4]; bool split[4];
  int G[4]; int nranks;
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

// the value of real k of the link in direction mu at the global site X of the periodic global lattice
static double global_link(const Grid& g, const int X[4], int mu, int k, int anti_pbc) {
  int W[4];
  for (int d = 0; d < 4; d++) W[d] = ((X[d] % g.G[d]) + g.G[d]) % g.G[d];
  const size_t gs = (((size_t)W[0] * g.G[1] + W[1]) * g.G[2] + W[2]) * g.G[3] + W[3];
  const double v = (double)((gs * 4 + mu) * 18 + k + 1);
  return (anti_pbc && mu == 0 && W[0] == g.G[0] - 1) ? -v : v;
}

struct Rank {
  int pc[4], O[4];
  double* U_alloc = nullptr; double* U = nullptr;   // the caller's links [V][72], exactly as large as they are
  std::vector<double> U_copy;
  double* Ue = nullptr; double* sbuf = nullptr; double* rbuf = nullptr;
};

static double* exact_alloc(size_t doubles) {   // 16-byte aligned and not a byte longer than asked for: the sanitizer guards both ends
  void* p = aligned_alloc(16, ((doubles * sizeof(double) + 15) / 16) * 16);
  if (!p) { printf("out of memory\n"); exit(2); }
  return static_cast<double*>(p);
}

static const double POISON = -7.0e300;

static void run_case(const char* name, const int L[4], const int P[4], const char* split_dirs, int anti_pbc, bool misaligned) {
  Grid g; g.nranks = 1;
  for (int d = 0; d < 4; d++) {
    g.L[d] = L[d]; g.P[d] = P[d]; g.G[d] = L[d] * P[d]; g.nranks *= P[d];
    g.split[d] = P[d] > 1 || strchr(split_dirs, "TZYX"[d]) != nullptr;
  }
  const int before = failures;
  const fs::Shell sh = fs::make_shell(g.L, g.split);
  const fs::Planes planes = fs::make_planes(g.L);
  const size_t V = sh.V, Ve = sh.Ve;
  size_t most = 1;
  for (int mu = 0; mu < 4; mu++) if (sh.h[mu]) { const size_t n = fs::make_slab(sh, mu).sites; if (n > most) most = n; }
  std::vector<Rank> ranks(g.nranks);
  for (int r = 0; r < g.nranks; r++) {
    Rank& k = ranks[r];
    coords_of(g.P, r, k.pc);
    for (int d = 0; d < 4; d++) k.O[d] = k.pc[d] * g.L[d];
    k.U_alloc = exact_alloc(V * 72 + (misaligned ? 1 : 0));
    k.U = k.U_alloc + (misaligned ? 1 : 0);          // 8 bytes off a 16-byte boundary: the one-real form of the copy
    for (size_t lx = 0; lx < V; lx++) {
      int x[4]; size_t q = lx;
      for (int d = 3; d >= 0; d--) { x[d] = (int)(q % g.L[d]) + k.O[d]; q /= g.L[d]; }
      for (int mu = 0; mu < 4; mu++) for (int c = 0; c < 18; c++) k.U[lx * 72 + mu * 18 + c] = global_link(g, x, mu, c, 0);   // unsigned, as the caller holds them
    }
    k.U_copy.assign(k.U, k.U + V * 72);
    k.Ue = exact_alloc(Ve * 72); k.sbuf = exact_alloc(most * 72); k.rbuf = exact_alloc(most * 72);
    for (size_t i = 0; i < Ve * 72; i++) k.Ue[i] = POISON;
    for (size_t i = 0; i < most * 72; i++) k.sbuf[i] = k.rbuf[i] = POISON;
  }
  // links_extend_kernel: a grid of whole workgroups of 256 threads, so some threads lie beyond the last element
  for (Rank& k : ranks) {
    const int negate = (anti_pbc && k.pc[0] == g.P[0] - 1) ? 1 : 0;
    if (misaligned) { const size_t n = ((V * 72 + 255) / 256) * 256; for (size_t i = 0; i < n; i++) fs::extend_links<1>(sh, k.U, k.Ue, i, negate); }
    else { const size_t n = ((V * 36 + 255) / 256) * 256; for (size_t i = 0; i < n; i++) fs::extend_links<2>(sh, k.U, k.Ue, i, negate); }
  }
  // the shell, one direction after the other, both sides; every rank packs, the messages travel, every rank unpacks
  for (int mu = 0; mu < 4; mu++) {
    if (!sh.h[mu]) continue;
    const fs::Slab slab = fs::make_slab(sh, mu);
    const size_t threads = ((slab.sites * 36 + 255) / 256) * 256;
    for (int side = 0; side < 2; side++) {
      const int src_c = side == 0 ? g.L[mu] - 1 : 0, dst_c = side == 0 ? -1 : g.L[mu];
      const fs::Slab from = fs::slab_at(sh, slab, src_c), to = fs::slab_at(sh, slab, dst_c);
      for (Rank& k : ranks) for (size_t i = 0; i < threads; i++) fs::slab_copy(sh, from, k.Ue, k.sbuf, i, true);
      for (int r = 0; r < g.nranks; r++) {
        const int send_peer = neighbor_rank(g, r, side == 0 ? mu : 4 + mu);
        CHECK(neighbor_rank(g, send_peer, side == 0 ? 4 + mu : mu) == r, "%s: rank %d sends to %d, which receives from another rank", name, r, send_peer);
        memcpy(ranks[send_peer].rbuf, ranks[r].sbuf, slab.sites * 72 * sizeof(double));
      }
      for (Rank& k : ranks) for (size_t i = 0; i < threads; i++) fs::slab_copy(sh, to, k.Ue, k.rbuf, i, false);
    }
  }
  for (int r = 0; r < g.nranks; r++) {
    Rank& k = ranks[r];
    CHECK(memcmp(k.U, k.U_copy.data(), V * 72 * sizeof(double)) == 0, "%s: rank %d: the caller's links were written", name, r);
    size_t unwritten = 0;
    for (size_t i = 0; i < Ve * 72; i++) unwritten += k.Ue[i] == POISON;
    CHECK(unwritten == 0, "%s: rank %d: %zu reals of the extended array were never written", name, r, unwritten);
    // the whole extended array against the global lattice (more than the leaves read: triple corners as well)
    size_t wrong = 0;
    for (size_t e = 0; e < Ve; e++) {
      int X[4]; size_t q = e;
      for (int d = 3; d >= 0; d--) { X[d] = (int)(q % sh.E[d]) - sh.h[d] + k.O[d]; q /= sh.E[d]; }
      for (int mu = 0; mu < 4; mu++) for (int c = 0; c < 18; c++) wrong += k.Ue[e * 72 + mu * 18 + c] != global_link(g, X, mu, c, anti_pbc);
    }
    CHECK(wrong == 0, "%s: rank %d: %zu reals of the extended array differ from the global lattice", name, r, wrong);
    // field_strength_kernel<true>, workgroup by workgroup and thread by thread
    std::vector<double> lds(fs::LDS_DOUBLES), lds_read(fs::LDS_DOUBLES);
    size_t off[2 * fs::EXT]; int flip[fs::EXT];
    std::vector<int> visits(V * 6, 0);
    for (int p = 0; p < 6; p++)
      for (int block = 0; block < planes.nblocks[p]; block++) {
        const fs::Tile t = fs::tile_of(planes, p, block);
        const fs::Tile te = fs::extended_tile(planes, sh, t, block);
        for (int tid = 0; tid < fs::THREADS; tid++) fs::stage_offsets<true>(planes, te, 0, tid, off, flip, &sh);
        for (double& v : lds) v = POISON;
        for (int tid = 0; tid < fs::THREADS; tid++) fs::stage_links(k.Ue, te, tid, off, flip, lds.data());   // reads inside Ue only: the sanitizer watches
        for (int i = 0; i < fs::EXT; i++) CHECK(flip[i] == 0, "%s: the extended instantiation flips a row", name);
        for (int tid = 0; tid < fs::THREADS; tid++) {
          const int a = tid / fs::TILE, b = tid % fs::TILE;
          const bool inside = t.a0 + a < g.L[t.mu] && t.b0 + b < g.L[t.nu];
          // the factors of the four leaves (site_field_strength): (w, steps in mu, steps in nu), w = 0: U_mu, 1: U_nu
          static const int reads[12][3] = {{0, 0, 0}, {1, 1, 0}, {0, 0, 1}, {1, 0, 0}, {0, -1, 1}, {1, -1, 0}, {0, -1, 0}, {1, -1, -1},
                                           {0, -1, -1}, {1, 0, -1}, {0, 0, -1}, {1, 1, -1}};
          for (double& v : lds_read) v = NAN;
          size_t lex = 0; double F[9], pl = 0;
          if (inside) {
            // own coordinates of the site from the tile and the lexicographic index of its outside coordinates
            int x[4]; size_t q = t.outside;
            for (int d = 3; d >= 0; d--) { x[d] = (int)(q % g.L[d]); q /= g.L[d]; }
            x[t.mu] = t.a0 + a; x[t.nu] = t.b0 + b;
            for (const int* rd : reads) {
              int X[4] = {x[0] + k.O[0], x[1] + k.O[1], x[2] + k.O[2], x[3] + k.O[3]};
              X[t.mu] += rd[1]; X[t.nu] += rd[2];
              const int e = (a + 1 + rd[1]) * fs::EXT + (b + 1 + rd[2]), dir = rd[0] ? t.nu : t.mu;
              for (int c = 0; c < 18; c++) {
                const double got = lds[(rd[0] * fs::NEXT + e) * fs::PITCH + c], want = global_link(g, X, dir, c, anti_pbc);
                CHECK(got == want, "%s: rank %d plane %d site (%d %d %d %d): U_%d at (%+d, %+d) real %d is %.0f, the global lattice holds %.0f", name, r, p,
                      x[0], x[1], x[2], x[3], dir, rd[1], rd[2], c, got, want);
                lds_read[(rd[0] * fs::NEXT + e) * fs::PITCH + c] = got;
              }
            }
          }
          // on a neighbourhood that holds these twelve links and nothing else: a finite result means no other link was read
          const bool did = fs::site_field_strength(planes, t, tid, lds_read.data(), &lex, F, &pl);
          CHECK(did == inside, "%s: thread %d of a tile at (%d, %d) %s", name, tid, t.a0, t.b0, did ? "computes outside the lattice" : "skips a site");
          if (did && inside) {
            bool finite = std::isfinite(pl);
            for (double f : F) finite = finite && std::isfinite(f);
            CHECK(finite, "%s: a leaf reads a link outside the twelve that were compared", name);
            CHECK(lex < V, "%s: F would be written outside the own lattice", name);
            if (lex < V) visits[(size_t)p * V + lex]++;
          }
        }
      }
    size_t not_once = 0;
    for (int v : visits) not_once += v != 1;
    CHECK(not_once == 0, "%s: rank %d: %zu (site, plane) pairs are not computed exactly once", name, r, not_once);
  }
  for (Rank& k : ranks) { free(k.U_alloc); free(k.Ue); free(k.sbuf); free(k.rbuf); }
  printf("%-44s local %dx%dx%dx%d grid %dx%dx%dx%d split %-4s anti_pbc %d%s: %s\n", name, L[0], L[1], L[2], L[3], P[0], P[1], P[2], P[3], split_dirs, anti_pbc,
         misaligned ? " (links 8 bytes off)" : "", failures == before ? "ok" : "FAILED");
}

int main() {
  const int one[4] = {1, 1, 1, 1};
  const int L4[4] = {4, 4, 4, 4}, Lr[4] = {2, 4, 6, 4}, Lbig[4] = {4, 6, 8, 10};
  for (int anti = 0; anti < 2; anti++) {
    // the process as its own neighbour in the split directions
    run_case("4^4, T", L4, one, "T", anti, false);
    for (const char* s : {"T", "Z", "Y", "X"}) run_case("2x4x6x4, one direction", Lr, one, s, anti, false);
    for (const char* s : {"TZ", "YX", "TZYX"}) run_case("2x4x6x4, several directions", Lr, one, s, anti, false);
    run_case("2x4x6x4, links not 16-byte aligned", Lr, one, "TZYX", anti, true);
    run_case("4x6x8x10, all four", Lbig, one, "TZYX", anti, false);
    // emulated process grids: the last time slice on another rank than the first, corners from a diagonal rank
    const int P2[4] = {2, 1, 1, 1}, P22[4] = {2, 2, 1, 1};
    run_case("grid 2x1x1x1", L4, P2, "", anti, false);
    run_case("grid 2x1x1x1", Lr, P2, "", anti, false);
    run_case("grid 2x1x1x1, the rest its own neighbour", Lr, P2, "ZYX", anti, false);
    run_case("grid 2x2x1x1", L4, P22, "", anti, false);
    run_case("grid 2x2x1x1", Lr, P22, "", anti, false);
    run_case("grid 2x2x1x1, the rest its own neighbour", Lr, P22, "YX", anti, true);
  }
  if (failures) { printf("%d comparisons failed\n", failures); return 1; }
  printf("LINK_SHELL_OK\n");
  return 0;
}
