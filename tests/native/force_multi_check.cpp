// force_multi_check.cpp -- a stand-alone host program (no GPU, no HIP) over the kernel bodies of csrc/force.h that the many-pair
// force adds: site_planes_multi and site_hop_multi, on the undivided lattice and in their process-grid form, with face_spinor_pack for the faces of a group,
// run thread by thread as force_planes_multi_kernel, force_hop_multi_kernel and face_spinor_pack_multi_kernel of force.hip run them.
// tests/test_force_multi_native.py builds it with the host compiler under -fsanitize=address,undefined and runs it; it prints
// FORCE_MULTI_OK and exits 0 when every comparison held.
//
// The reference is  sum_s w_s x  what force::site_force_tensor writes for the pair s alone on the undivided periodic lattice: A_p(x)
// in 54 reals per site and the hopping slot of the four own links.  n pairs run as groups of force::GROUP, the first in the write
// form onto poisoned arrays, the others in the add form, the last one partial.  A process grid is emulated inside the program as in
// force_shell_check.cpp: every rank has its own site tables, fields and extended A, and a message is a memcpy that follows the
// neighbour ranks; every buffer is exactly as long as the group needs, so the sanitizer guards a partial group's end.
// Bar: 1e-13 of the norm, the project's fp64 bar (every number is a sum of at most 9 x 8 products of three numbers of order one).
#include "force.h"
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

// a lattice with the device's site order (even sites first, each parity lexicographic) and the tables of force::Sites.  On a rank
// of a grid `split` directions have no + mu neighbour of their own at x_mu = L - 1: the table holds -1 - slot there, slot the rank of
// the site's other coordinates among the face sites in lexicographic order
struct Box {
  int L[4], O[4]; size_t V;
  std::vector<int> lex_of_site, site_of_lex, nb;
  std::vector<unsigned char> parity;
  std::vector<int> face[4];      // device sites with x_mu = 0, in slot order
  size_t lex(const int c[4]) const {
    int w[4];
    for (int d = 0; d < 4; d++) w[d] = ((c[d] % L[d]) + L[d]) % L[d];
    return (((size_t)w[0] * L[1] + w[1]) * L[2] + w[2]) * L[3] + w[3];
  }
  void coords(size_t lx, int c[4]) const { for (int d = 3; d >= 0; d--) { c[d] = (int)(lx % L[d]); lx /= L[d]; } }
  void build(const int l[4], const int origin[4], const bool split[4]) {
    V = 1;
    for (int d = 0; d < 4; d++) { L[d] = l[d]; O[d] = origin[d]; V *= (size_t)l[d]; }
    lex_of_site.resize(V); site_of_lex.resize(V); nb.resize(8 * V); parity.resize(V);
    size_t n = 0;
    for (int pass = 0; pass < 2; pass++)
      for (size_t lx = 0; lx < V; lx++) {
        int c[4]; coords(lx, c);
        if (((c[0] + c[1] + c[2] + c[3] + O[0] + O[1] + O[2] + O[3]) & 1) == pass) { lex_of_site[n] = (int)lx; site_of_lex[lx] = (int)n; parity[n] = (unsigned char)pass; n++; }
      }
    for (int mu = 0; mu < 4; mu++) {
      face[mu].clear();
      if (!split[mu]) continue;
      for (size_t lx = 0; lx < V; lx++) {
        int c[4]; coords(lx, c);
        if (c[mu] == 0) face[mu].push_back(site_of_lex[lx]);
      }
    }
    for (size_t s = 0; s < V; s++) {
      int c[4]; coords((size_t)lex_of_site[s], c);
      for (int mu = 0; mu < 4; mu++) {
        c[mu]++;
        if (split[mu] && c[mu] == L[mu]) {
          int z[4] = {c[0], c[1], c[2], c[3]}; z[mu] = 0;
          const int target = site_of_lex[lex(z)];
          int slot = -1;
          for (size_t k = 0; k < face[mu].size(); k++) if (face[mu][k] == target) slot = (int)k;
          nb[mu * V + s] = -1 - slot;
        } else {
          nb[mu * V + s] = site_of_lex[lex(c)];
        }
        c[mu] -= 2; nb[(4 + mu) * V + s] = site_of_lex[lex(c)];   // not read by the force
        c[mu]++;
      }
    }
  }
};

static int rank_of(const int P[4], const int pc[4]) { return ((pc[0] * P[1] + pc[1]) * P[2] + pc[2]) * P[3] + pc[3]; }
static void coords_of(const int P[4], int r, int pc[4]) { for (int d = 3; d >= 0; d--) { pc[d] = r % P[d]; r /= P[d]; } }
static int neighbor_rank(const int P[4], int rank, int d) {   // d < 4: + mu, 4 + mu: - mu
  int q[4]; coords_of(P, rank, q);
  const int mu = d & 3;
  q[mu] = d < 4 ? (q[mu] + 1) % P[mu] : (q[mu] - 1 + P[mu]) % P[mu];
  return rank_of(P, q);
}

// a lexicographic [V][24] field into the chunked-SoA field of the box's sites
static void to_device_order(const Box& b, const Box& global, const double* glex, double* dev) {
  for (size_t s = 0; s < b.V; s++) {
    int c[4]; b.coords((size_t)b.lex_of_site[s], c);
    for (int d = 0; d < 4; d++) c[d] += b.O[d];
    const size_t gl = global.lex(c);
    for (int r = 0; r < 24; r++) dev[force::soa2(b.V, s, r)] = glex[gl * 24 + r];
  }
}

struct RankData {
  Box box;
  double* W = nullptr;
  std::vector<double*> X, Y;
  double* A = nullptr; double* slots = nullptr;
  double* send = nullptr; double* recv[4] = {nullptr, nullptr, nullptr, nullptr};
};

static void run_case(const char* name, const int L[4], const int P[4], double csw, int npairs) {
  const int before = failures;
  const bool clover = csw != 0.0;
  int GL[4], zero[4] = {0, 0, 0, 0}; bool split[4], none[4] = {false, false, false, false};
  int nranks = 1; bool grid = false;
  for (int d = 0; d < 4; d++) { GL[d] = L[d] * P[d]; split[d] = P[d] > 1; nranks *= P[d]; grid = grid || split[d]; }
  Box global; global.build(GL, zero, none);
  const size_t GV = global.V;
  const double scale_even = 1.1, scale_odd = 0.9;
  const force::Gammas gm = force::make_gammas();

  // the fields of the undivided lattice, and the reference: the single-pair body pair by pair
  double* GW = exact_alloc(72 * GV);
  for (size_t i = 0; i < 72 * GV; i++) GW[i] = urand();
  std::vector<double*> GX(npairs), GY(npairs), DX(npairs), DY(npairs);
  std::vector<double> weights(npairs);
  for (int s = 0; s < npairs; s++) {
    GX[s] = exact_alloc(24 * GV); GY[s] = exact_alloc(24 * GV); DX[s] = exact_alloc(24 * GV); DY[s] = exact_alloc(24 * GV);
    for (size_t i = 0; i < 24 * GV; i++) { GX[s][i] = urand(); GY[s][i] = urand(); }
    to_device_order(global, global, GX[s], DX[s]); to_device_order(global, global, GY[s], DY[s]);
    weights[s] = (s % 2 ? -1.0 : 1.0) * (0.3 + 0.8 * s) * (s % 3 == 2 ? 10.0 : 1.0);     // mixed sign and magnitude
  }
  std::vector<double> refA(54 * GV, 0.0), refH(36 * GV, 0.0);     // refH[(mu * 9 + r) * GV + lex]
  {
    const force::Sites gs{GV, global.nb.data(), global.lex_of_site.data(), global.parity.data(), csw, scale_even, scale_odd};
    double* A1 = exact_alloc(54 * GV); double* S1 = exact_alloc(144 * GV);
    for (int s = 0; s < npairs; s++) {
      for (size_t site = 0; site < GV; site++) force::site_force_tensor(gs, gm, DX[s], DY[s], GW, (int)clover, A1, S1, site);
      if (clover) for (size_t i = 0; i < 54 * GV; i++) refA[i] += weights[s] * A1[i];
      for (int mu = 0; mu < 4; mu++)
        for (size_t i = 0; i < 9 * GV; i++) refH[(size_t)mu * 9 * GV + i] += weights[s] * S1[(size_t)(mu * force::SLOTS + force::HOP_SLOT) * 9 * GV + i];
    }
    free(A1); free(S1);
  }

  // the ranks (one, the undivided lattice itself, where no direction is split)
  const fs::Shell shell = fs::make_shell(L, split);
  const size_t V = shell.V, Ve = shell.Ve;
  std::vector<RankData> ranks(nranks);
  for (int r = 0; r < nranks; r++) {
    RankData& k = ranks[r];
    int pc[4], O[4]; coords_of(P, r, pc);
    for (int d = 0; d < 4; d++) O[d] = pc[d] * L[d];
    k.box.build(L, O, split);
    k.W = exact_alloc(72 * V);
    for (size_t lx = 0; lx < V; lx++) {
      int c[4]; k.box.coords(lx, c);
      for (int d = 0; d < 4; d++) c[d] += O[d];
      memcpy(k.W + lx * 72, GW + global.lex(c) * 72, 72 * sizeof(double));
    }
    for (int s = 0; s < npairs; s++) {
      k.X.push_back(exact_alloc(24 * V)); k.Y.push_back(exact_alloc(24 * V));
      to_device_order(k.box, global, GX[s], k.X[s]); to_device_order(k.box, global, GY[s], k.Y[s]);
    }
    k.A = exact_alloc(54 * (grid ? Ve : V)); k.slots = exact_alloc(144 * V);
    for (size_t i = 0; i < 54 * (grid ? Ve : V); i++) k.A[i] = POISON;
    for (size_t i = 0; i < 144 * V; i++) k.slots[i] = POISON;
  }

  int launches = 0;
  for (int first = 0; first < npairs; first += force::GROUP, launches++) {
    const int n = npairs - first < force::GROUP ? npairs - first : force::GROUP;
    std::vector<force::Pairs> pr(nranks);
    std::vector<force::Grid> gr(nranks);
    for (int r = 0; r < nranks; r++) {
      for (int q = 0; q < force::GROUP; q++) {
        pr[r].x[q] = q < n ? ranks[r].X[first + q] : nullptr; pr[r].y[q] = q < n ? ranks[r].Y[first + q] : nullptr;
        pr[r].w[q] = q < n ? weights[first + q] : 0.0;
      }
      pr[r].n = n; pr[r].add = first > 0;
      gr[r].shell = shell;
      for (int mu = 0; mu < 4; mu++) { gr[r].face[mu] = nullptr; gr[r].F[mu] = 0; }
    }
    // the faces of the whole group: one message per split direction, towards - mu
    for (int mu = 0; mu < 4; mu++) {
      if (!split[mu]) continue;
      const size_t F = ranks[0].box.face[mu].size();
      for (int r = 0; r < nranks; r++) { ranks[r].send = exact_alloc(48 * F * n); ranks[r].recv[mu] = exact_alloc(48 * F * n); }
      for (int r = 0; r < nranks; r++) {
        const size_t threads = ((24 * F + 255) / 256) * 256;     // whole workgroups, as the kernel has
        for (int q = 0; q < n; q++)
          for (size_t i = 0; i < threads; i++)
            force::face_spinor_pack(pr[r].x[q], pr[r].y[q], V, ranks[r].box.face[mu].data(), F, ranks[r].send + (size_t)q * 48 * F, i);
        const int to = neighbor_rank(P, r, 4 + mu);
        CHECK(neighbor_rank(P, to, mu) == r, "%s: rank %d sends to %d, which receives from another rank", name, r, to);
        memcpy(ranks[to].recv[mu], ranks[r].send, 48 * F * n * sizeof(double));
      }
      for (int r = 0; r < nranks; r++) { free(ranks[r].send); gr[r].face[mu] = ranks[r].recv[mu]; gr[r].F[mu] = (int)F; }
    }
    for (int r = 0; r < nranks; r++) {
      RankData& k = ranks[r];
      const force::Sites sites{V, k.box.nb.data(), k.box.lex_of_site.data(), k.box.parity.data(), csw, scale_even, scale_odd};
      for (size_t s = 0; s < V + 3; s++) {     // a few threads beyond the last site, as a grid of workgroups has
        if (clover) force::site_planes_multi(sites, gm, pr[r], k.A, s, grid, &gr[r]);
        for (int mu = 0; mu < 4; mu++) force::site_hop_multi(sites, gm, pr[r], k.W, k.slots, s, mu, grid, &gr[r]);
      }
      for (int mu = 0; mu < 4; mu++) if (k.recv[mu]) { free(k.recv[mu]); k.recv[mu] = nullptr; }
    }
  }

  // every rank's numbers against the reference at the same global site; what the bodies do not own stays untouched
  double d2 = 0, n2 = 0; size_t touched = 0;
  for (int r = 0; r < nranks; r++) {
    const RankData& k = ranks[r];
    const size_t AV = grid ? Ve : V;
    std::vector<char> interior(AV, 0);
    for (size_t lx = 0; lx < V; lx++) {
      int c[4]; k.box.coords(lx, c);
      for (int d = 0; d < 4; d++) c[d] += k.box.O[d];
      const size_t gl = global.lex(c), ax = grid ? fs::extended_site(shell, lx) : lx;
      interior[ax] = 1;
      if (clover)
        for (int q = 0; q < 54; q++) { const double got = k.A[(size_t)q * AV + ax], want = refA[(size_t)q * GV + gl]; d2 += (got - want) * (got - want); n2 += want * want; }
      for (int mu = 0; mu < 4; mu++)
        for (int q = 0; q < 9; q++) {
          const double got = k.slots[((size_t)(mu * force::SLOTS + force::HOP_SLOT) * 9 + q) * V + lx], want = refH[((size_t)mu * 9 + q) * GV + gl];
          d2 += (got - want) * (got - want); n2 += want * want;
          for (int plane = 0; plane < force::HOP_SLOT; plane++) touched += k.slots[((size_t)(mu * force::SLOTS + plane) * 9 + q) * V + lx] != POISON;
        }
    }
    for (size_t e = 0; e < AV; e++)
      for (int q = 0; q < 54; q++) touched += (!interior[e] || !clover) && k.A[(size_t)q * AV + e] != POISON;
  }
  const double err = std::sqrt(d2 / n2);
  CHECK(n2 > 1.0, "%s: the reference vanishes", name);
  CHECK(std::isfinite(err) && err <= 1e-13, "%s: relative difference %.3e against 1e-13", name, err);
  CHECK(touched == 0, "%s: %zu reals outside A's interior and the hopping slots were written", name, touched);
  printf("%-18s local %dx%dx%dx%d grid %dx%dx%dx%d csw %.1f pairs %2d in %d launches: norm %.3e relative difference %.2e%s\n", name, L[0], L[1], L[2], L[3], P[0],
         P[1], P[2], P[3], csw, npairs, launches, std::sqrt(n2), err, failures == before ? ": ok" : ": FAILED");
  for (RankData& k : ranks) {
    free(k.W); free(k.A); free(k.slots);
    for (double* p : k.X) free(p);
    for (double* p : k.Y) free(p);
  }
  for (int s = 0; s < npairs; s++) { free(GX[s]); free(GY[s]); free(DX[s]); free(DY[s]); }
  free(GW);
}

int main() {
  const int G = force::GROUP;
  const int one[4] = {1, 1, 1, 1}, Pt[4] = {2, 1, 1, 1}, Ptz[4] = {2, 2, 1, 1};
  const int L4[4] = {4, 4, 4, 4}, L6[4] = {4, 4, 6, 6};
  const int counts[4] = {1, G, G + 1, 2 * G + 1};
  for (const int* L : {L4, L6})
    for (double csw : {1.3, 0.0})
      for (int n : counts) run_case("undivided", L, one, csw, n);
  for (const int* P : {Pt, Ptz})
    for (double csw : {1.3, 0.0}) {
      run_case("emulated grid", L4, P, csw, G + 1);
      run_case("emulated grid", L6, P, csw, 2 * G + 1);
      run_case("emulated grid", L4, P, csw, 1);
    }
  if (failures) { printf("%d comparisons FAILED\n", failures); return 1; }
  printf("FORCE_MULTI_OK group %d\n", G);
  return 0;
}
