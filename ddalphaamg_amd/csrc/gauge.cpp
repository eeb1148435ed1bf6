// gauge.cpp -- gauge links -> Wilson-Clover operator data on a process grid: the own links (D = U/2, anti-periodic sign on the
// last global time slice) and the neighbouring processes' links that the clover leaves reach, one site deep; the clover term
// and the plaquette are then computed on the device (gauge_device.hip).
// Reference: dirac_setup src/dirac.c:60-168 (D = U/2 at :80, ghost shell of the gauge field :88-120), anti-periodic sign
// src/io.c:536-541.  Output is in the reference's own storage (D: [V][4][9] complex, clover: [V][42] complex, lexicographic
// sites) so it can be compared one-to-one with g.op_double.
#include "gauge.h"
#include "common.h"
#include "geometry.h"
#include "halo.h"
#include <cstring>
#include <vector>

namespace ddamg {

namespace {
// the local lattice extended by a halo of depth h[mu] (0: the direction wraps periodically inside the process, 1: coordinates
// -1 .. L[mu] are valid and hold the neighbouring processes' links)
struct ExtLattice {
  int L[4]; int h[4] = {0, 0, 0, 0};
  inline size_t lex(const int c[4]) const {
    size_t i = 0;
    for (int mu = 0; mu < 4; mu++) i = i * (L[mu] + 2 * h[mu]) + (c[mu] + h[mu]);
    return i;
  }
};
}  // namespace

double gauge_to_operator_dist(const Geometry& g, Comm* comm, const double* gauge_in, int anti_pbc, double m0, double csw,
                              double* D_out, double* clover_out, hipStream_t st) {
  const int* L = g.L;
  const int V = g.V;
  ExtLattice f; for (int i = 0; i < 4; i++) { f.L[i] = L[i]; f.h[i] = g.split[i] ? 1 : 0; }
  int E[4]; size_t Ve = 1;
  for (int mu = 0; mu < 4; mu++) { E[mu] = L[mu] + 2 * f.h[mu]; Ve *= E[mu]; }
  std::vector<double> Ue(Ve * 72, 0.0);
  // my own links into the interior of the extended field; anti-periodic sign on the last global time slice
  for (int lx = 0; lx < V; lx++) {
    int x[4]; int r = lx;
    x[3] = r % L[3]; r /= L[3]; x[2] = r % L[2]; r /= L[2]; x[1] = r % L[1]; r /= L[1]; x[0] = r;
    double* dst = Ue.data() + f.lex(x) * 72;
    const double* src = gauge_in + (size_t)lx * 72;
    for (int k = 0; k < 72; k++) dst[k] = src[k];
    if (anti_pbc && g.pc[0] == g.P[0] - 1 && x[0] == L[0] - 1)
      for (int k = 0; k < 18; k++) dst[DIR_T * 18 + k] = -dst[DIR_T * 18 + k];
    for (int k = 0; k < 72; k++) D_out[(size_t)lx * 72 + k] = 0.5 * dst[k];
  }
  // halo, one direction after the other so that the corners travel along (a slab spans the full extended range of
  // the other directions, including the halos received before)
  for (int mu = 0; mu < 4; mu++) {
    if (!f.h[mu]) continue;
    size_t slab = Ve / E[mu];
    std::vector<double> sbuf(slab * 72), rbuf(slab * 72);
    for (int side = 0; side < 2; side++) {
      // side 0: my slice x_mu = L-1 goes to the +mu neighbour (its x_mu = -1); side 1: x_mu = 0 to the -mu neighbour (its x_mu = L)
      const int src_c = side == 0 ? L[mu] - 1 : 0, dst_c = side == 0 ? -1 : L[mu];
      size_t k = 0;
      int c[4];
      for (c[0] = -f.h[0]; c[0] < L[0] + f.h[0]; c[0]++) for (c[1] = -f.h[1]; c[1] < L[1] + f.h[1]; c[1]++)
      for (c[2] = -f.h[2]; c[2] < L[2] + f.h[2]; c[2]++) for (c[3] = -f.h[3]; c[3] < L[3] + f.h[3]; c[3]++) {
        if (c[mu] != src_c) continue;
        memcpy(sbuf.data() + k * 72, Ue.data() + f.lex(c) * 72, sizeof(double) * 72); k++;
      }
      comm_sendrecv_host(comm, sbuf.data(), g.neighbor_rank[side == 0 ? mu : 4 + mu], rbuf.data(), g.neighbor_rank[side == 0 ? 4 + mu : mu],
                         sizeof(double) * slab * 72, 100 + 2 * mu + side);
      k = 0;
      for (c[0] = -f.h[0]; c[0] < L[0] + f.h[0]; c[0]++) for (c[1] = -f.h[1]; c[1] < L[1] + f.h[1]; c[1]++)
      for (c[2] = -f.h[2]; c[2] < L[2] + f.h[2]; c[2]++) for (c[3] = -f.h[3]; c[3] < L[3] + f.h[3]; c[3]++) {
        if (c[mu] != src_c) continue;
        int d[4] = {c[0], c[1], c[2], c[3]}; d[mu] = dst_c;
        memcpy(Ue.data() + f.lex(d) * 72, rbuf.data() + k * 72, sizeof(double) * 72); k++;
      }
    }
  }
  double acc[2] = {clover_and_plaquette_extended_device(L, f.h, Ue.data(), m0, csw, clover_out, st), (double)V * 6.0};
  comm_allreduce_host(comm, acc, 2);
  return acc[0] / acc[1];
}

}  // namespace ddamg
