// extended_links.h -- the lattice extended by the neighbours' links, on the device (kernels and fill: gauge_device.hip).
// Used by ddamg_hip_set_gauge_device_grid for the caller's links and by the ddamg_hip_force_*_grid calls for W = 2 D.
#pragma once
#include "common.h"
#include "field_strength.h"
#include "geometry.h"
#include "halo.h"
#include <algorithm>

namespace ddamg {

// The lattice extended by the neighbours' links, on the device: the caller's links go into the interior (with the anti-periodic
// sign, on the processes that hold the last global time slice), then the shell arrives direction by direction, device to device
// (comm_sendrecv_device), each slab spanning what the directions before it brought so that the corners travel along -- a corner
// of a (T, Z) plane comes from the diagonal process in two hops.  A full extended copy, not a compact shell next to the caller's
// array: it costs one streaming pass and (E/L)^4 of the field for the duration of the call, and keeps the staging of
// field_strength_kernel a sum of a row and a column offset.  All four links of a shell site travel (72 doubles), though the
// leaves never read U_mu at x + mu: trimming the slab at L would save a quarter of half the messages and cost a second layout.
//
// depth: how many sites deep the shell is, 1 for the leaves of Q and the plaquette staples, 2 for the rectangle staples of the gauge
// force (gauge_md.h).  Still two messages per split direction and call, one slab `depth` sites thick each way, of
//   72 * 8 * depth * prod_{d != mu} (L_d + 2 depth if d < mu and split, else L_d)  bytes.
// A split direction whose local extent is below the depth is refused (the shell would have to come from the neighbour's neighbour).
struct ExtendedLinks {
  fs::Shell shell;
  DeviceBuffer<double> Ue, sbuf, rbuf;
  explicit ExtendedLinks(const Geometry& g, int depth = 1) : shell(fs::make_shell(g.L, g.split, depth)) {
    for (int mu = 0; mu < 4; mu++)
      DDAMG_REQUIRE(!shell.h[mu] || g.L[mu] >= depth, "the shell of the links is deeper than the local lattice in a split direction");
    Ue.alloc(72 * shell.Ve);
    size_t most = 0;
    for (int mu = 0; mu < 4; mu++) if (shell.h[mu]) most = std::max(most, fs::make_slab(shell, mu).sites);
    if (most) { sbuf.alloc(72 * most); rbuf.alloc(72 * most); }
  }
  // enqueued on st; collective over the process grid.  dU is read, never written.  anti_pbc == 0: no sign is applied (links that
  // carry it already, as W = 2 D does)
  void fill(const Geometry& g, Comm* comm, const double* dU, int anti_pbc, hipStream_t st);
};

}  // namespace ddamg
