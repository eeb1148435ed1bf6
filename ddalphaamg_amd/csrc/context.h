// context.h -- solver context behind the C-ABI (include/ddamg_hip.h).
// Reference counterpart: global_struct g + level_struct l (src/main.h:263-390).
#pragma once
#include "common.h"
#include "geometry.h"
#include "fine_op.h"
#include "mg.h"
#include "krylov.h"
#include "bicgstab.h"
#include "eo_system.h"
#include "force.h"
#include "gauge_md.h"
#include "multishift.h"
#include "../../include/ddamg_hip.h"
#include <vector>
#include <memory>

struct ddamg_hip_vec {
  int level = 0;
  int precision = 32;
  int ndof = 12;
  int V = 0;
  int aos = 0;  // 0: chunked SoA (fine level), 1: site-major AoS (coarse levels)
  ddamg::DeviceBuffer<char> data;
};

// a store of past solutions (ddamg_hip_chrono_*, solver.cpp): fine fp64 vectors in the solver's layout, n reals each
struct ddamg_hip_chrono {
  const ddamg_hip_ctx* owner = nullptr;
  int depth = 0, count = 0, next = 0;      // a ring: slot `next` takes the next push, the newest vector is in slot next - 1
  size_t n = 0;
  ddamg::DeviceBuffer<double> V;           // [depth][n]
  // workspace of a guess, from the first one on: the orthonormalised images Q = A V, their companions W (the same operations on
  // V), and the predicted residual
  ddamg::DeviceBuffer<double> Q, W, r;
  double* slot(int age) const { return V + (size_t)((next - 1 - age + 2 * depth) % depth) * n; }   // age 0: the newest
};

namespace ddamg {

struct Level {
  int depth = 0;
  int ndof = 12;  // complex dof per site
  Geometry geom;
  DeviceBuffer<int> d_lex_of_site;
};

}  // namespace ddamg

// the stream and the timer events: a base, so that they are destroyed after every member of the context that may still use them
struct ddamg_hip_ctx_handles {
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~ddamg_hip_ctx_handles() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

struct ddamg_hip_ctx : ddamg_hip_ctx_handles {
  explicit ddamg_hip_ctx(const ddamg::Knobs& k) : knobs(k) {}
  // selects the device, waits for the stream, then drops the hierarchies and the transport before the operators they point into;
  // the remaining members free themselves in reverse order of declaration, the stream and the events go last
  ~ddamg_hip_ctx();
  const ddamg::Knobs knobs;   // the DDAMG_* switches as the environment held them at ddamg_hip_create (knobs.h)
  ddamg_hip_params par;
  int device = 0;
  std::vector<std::unique_ptr<ddamg::Level>> levels;
  // fine operator in the reference's host storage (fp64) + device copies in both precisions
  std::vector<double> D_host, clover_host;
  bool have_operator = false;
  // whether D_host / clover_host show the operator that is set: cleared by ddamg_hip_set_gauge*_device, which fills neither; who
  // needs them then rebuilds them from the fp64 operator first (ddamg_hip_get_operator)
  bool mirror_valid = false;
  // whether the operator came from ONE link field (ddamg_hip_set_gauge*, _set_gauge*_device, _load_ildg_conf; kept by shift_mass and
  // scale_clover): then D and the clover term are functions of the links W = 2 D, which is what ddamg_hip_force_* differentiate.
  // ddamg_hip_set_operator and the two-field ddamg_hip_set_gauge2* forms clear it
  bool from_links = false;
  // scale_clover: unscaled fp64 copy of the clover field on the device while the operator is scaled (ddamg_hip_scale_clover)
  ddamg::DeviceBuffer<double> clover_base;
  double scale_even = 1.0, scale_odd = 1.0;
  ddamg::FineOp<float> fop32;
  ddamg::FineOp<double> fop64;
  ddamg::Comm* comm = nullptr;  // halo transport of a decomposed lattice (halo.h)
  // staging buffer for host<->device vector transfers (lexicographic fp64)
  ddamg::DeviceBuffer<double> d_stage;
  double* stage(size_t bytes);

  // multigrid preconditioner (V-cycle precision float when mixed_precision >= 1, double otherwise)
  std::unique_ptr<ddamg::Multigrid<float>> mg32;
  std::unique_ptr<ddamg::Multigrid<double>> mg64;
  bool setup_done = false;
  // bits per real, 32 or 16, of what the solve may read from a 16-bit copy (half_storage.h; ddamg_hip_set_*_storage, initial
  // values from knobs.*_half); handed to mg32 when the hierarchy is created
  ddamg::StorageBits storage;
  // outer FGMRES (fp64) and its workspace
  ddamg::Gmres<double> outer;
  ddamg::ReduceWork rw_outer;
  bool outer_ready = false;
  ddamg::ReduceWork rw_blas;
  bool rw_blas_ready = false;
  ddamg::DeviceBuffer<float> p32_in, p32_out;
  // fgmres_MP (mixed_precision 2): fp32 Krylov basis, fp64 residual/solution (src/linsolve.c:153-424)
  ddamg::Gmres<float> mp_inner;
  ddamg::ReduceWork rw_mp;
  bool mp_ready = false;
  ddamg::DeviceBuffer<double> mp_x, mp_b, mp_r;
  // method 5: FGMRES preconditioned by BiCGstab on the odd-even Schur complement of the fine operator, no multigrid
  ddamg::OddEvenBicgstab<float> bicg32;
  ddamg::OddEvenBicgstab<double> bicg64;
  bool bicg_ready = false;
  // the even-odd preconditioned system (ddamg_hip_schur_*, ddamg_hip_solve_schur_*): two work vectors per precision, from the first use on
  ddamg::EoWork eo;
  // the fermion force (ddamg_hip_force_*): links, site tensors and per-plane parts, from the first use on
  ddamg::ForceWork force;
  // the gauge sector (ddamg_hip_gauge_*, ddamg_hip_links_*, ddamg_hip_momentum_*): the partial sums of its reductions, from the first use on;
  // the plane slots of the gauge force are force.slots
  ddamg::GaugeMdWork gauge_md;
  // multi-shift CG on Dhat^dagger Dhat + sigma_s (ddamg_hip_solve_schur_multishift_*): the loop's reduction workspace and the list of
  // even sites, from the first use on; the vectors of a solve live for the call
  ddamg::MultishiftWork ms;
  // results of the last solve
  int last_iter = 0, last_coarse_iter = 0;
  double last_relres = 0;
  std::vector<double> last_history;
};

// the *_device entry points (capi.cpp): throws unless [p, p + bytes) lies in one allocation in the memory of the context's device
void ddamg_require_device_array(const ddamg_hip_ctx* c, const void* p, size_t bytes, const char* what);
// ... and unless the output and the input array of a call are disjoint
void ddamg_require_disjoint(const void* out, const void* in, size_t bytes, const char* what);
