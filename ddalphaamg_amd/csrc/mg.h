// mg.h -- the multigrid hierarchy (2 to 4 levels), V/K-cycle and setup: host orchestration of the HIP kernels.
// Reference: vcycle_PRECISION / smoother_PRECISION src/vcycle_generic.c:25-141 (post-smoothing only; K-cycle =
//   FGMRES(kcycle_restart, kcycle_max_restart, kcycle_tol) on every intermediate level, :110-114),
//   coarse_solve_odd_even_PRECISION / coarse_apply_schur_complement_PRECISION src/coarse_oddeven_generic.c:1139-1189,
//   next_level_setup src/init.c:32-120, interpolation_PRECISION_define src/setup_generic.c:191-275,
//   coarse_grid_correction_PRECISION_setup :29-108, re_setup_PRECISION :278-321,
//   inv_iter_inv_fcycle_PRECISION / test_vector_PRECISION_update :418-503,
//   coarse_operator_PRECISION_setup src/coarse_operator_generic.c:53-100.
#pragma once
#include "common.h"
#include "geometry.h"
#include "fine_op.h"
#include "sap.h"
#include "transfer.h"
#include "coarse_op.h"
#include "coarse_mg.h"
#include "coarse_lockstep.h"
#include "coarse_multi.h"
#include "coarse_half.h"
#include "transfer_half.h"
#include "half_storage.h"
#include "krylov.h"
#include "../../include/ddamg_hip.h"
#include <memory>
#include <vector>
#include <string>
#include <utility>

namespace ddamg {

template <typename T>
struct MGLevel {
  int depth = 0;
  const Geometry* g = nullptr;
  int n = 12;            // complex dof per site
  int nvec = 0;          // test vectors on this level (0 on the coarsest)
  bool coarsest = false;
  size_t nel = 0;        // reals per vector
  // operators
  const FineOp<T>* fop = nullptr;   // depth 0
  CoarseOp<T> cop;                  // depth > 0
  CoarseHalf half;                  // depth > 0, fp32: the 16-bit copy of cop's couplings, allocated by its first use (Multigrid::half_of)
  // smoother + transfer to the next level (not on the coarsest level)
  SapSmoother<T> fsap; Interpolation<T> fip;     // depth 0
  CoarseSap<T> csap; CoarseTransfer<T> cip;      // depth > 0
  // Krylov solver of this level: K-cycle FGMRES (intermediate) or even-site Schur GMRES (coarsest)
  Gmres<T> gm;
  ReduceWork rw;
  DeviceBuffer<T> buf[4];
  // GMRES smoother (method 4): GMRES(block_iter) restarted post_smooth_iter times on the global odd-even Schur complement
  Gmres<T> sgm;
  ReduceWork srw;
  DeviceBuffer<T> sbuf[3];
  DeviceBuffer<int> d_parity_sites[2];           // depth > 0: even / odd sites of this level
  int n_parity_sites[2] = {0, 0};
  // setup helpers
  DeviceBuffer<unsigned char> d_agg_face;
  AggFaces agg_faces;                    // depth 0: the forward faces of an aggregate in compact form (Galerkin construction)
  DeviceBuffer<unsigned short> d_agg_tables;   // what agg_faces.rank / .list point into
  DeviceBuffer<unsigned char> d_dir_mask[4];
  std::vector<int> ref_order;   // site visited i-th by the reference's vector loops on this level
};

// The coarsest level gathered on every process (ddamg_hip_params::gather_coarsest; purpose of the reference's idle-process
// gathering, src/gathering_generic.c:24-346): the whole coarsest lattice, its operator collected from all processes after
// every (re)build, and the odd-even Schur GMRES on it without any communication.
template <typename T>
struct GatheredCoarsest {
  bool on = false;
  Geometry g;            // the GLOBAL coarsest lattice, not decomposed
  CoarseOp<T> cop;
  CoarseHalf half;       // as MGLevel::half
  Gmres<T> gm;
  ReduceWork rw;         // no transport: every process computes the same sums
  DeviceBuffer<T> buf[2];
  DeviceBuffer<T> raw;        // all-gather landing zone: [process][local site][...]
  DeviceBuffer<int> d_g2d;    // gathered site -> process * V_local + local site
  DeviceBuffer<int> d_d2g;    // my local site -> gathered site
  int V_local = 0;
};

template <typename T>
class Multigrid {
 public:
  typedef T real;
  // knobs: the context's switches (knobs.h); they outlive the hierarchy and reach every object created for it
  Multigrid(const ddamg_hip_params& par, const Knobs& knobs, const std::vector<const Geometry*>& geoms, const FineOp<T>* fop, hipStream_t st);
  ~Multigrid();   // waits for the stream; the members free themselves

  // ---- setup -------------------------------------------------------------------------------
  void initial_setup();                 // method_setup
  void initial_setup_from(int l0);
  void iterative_setup(int iters);      // method_update
  void import_test_vectors(const double* tv_lex_host);   // level-0 test vectors, then re_setup(0)
  void import_interpolation(const double* P_lex_host);   // level-0 interpolation vectors as they are
  void operator_changed();              // fine operator re-uploaded: rebuild the coarse operators
  void mass_shifted(double diff);       // fine operator's mass changed by diff: the same shift on every coarse self coupling
  void set_kcycle_tol(double tol);
  void release_setup_workspace();       // large temporaries of the Galerkin construction (kept across the builds of one setup)
  void set_comm(Comm* c) { comm_ = c; for (auto& lv : lv_) { lv->rw.comm = c; lv->srw.comm = c; lv->cop.set_comm(c); } }
  bool coarsest_gathered() const { return gath_.on; }
  void regather_coarsest_operator();   // after every (re)build / import of the coarsest operator

  // ---- hot path -----------------------------------------------------------------------------
  void apply_op(int l, T* out, const T* in);
  void smoother(int l, T* phi, T* Dphi, const T* eta, int cycles, int res);
  void restrict_to(int l, T* phi_c, const T* phi);               // level l -> l+1
  void interpolate(int l, T* phi, const T* phi_c, bool add);     // level l+1 -> l
  int coarse_solve();                                            // coarsest level, vectors coarse_x()/coarse_b()
  // ncols right-hand sides in lockstep (coarse_lockstep.h); X, B: columns of ordinary coarsest-level vectors; false if the shape is not covered
  bool coarse_solve_many(T* X, size_t xstride, const T* B, size_t bstride, int ncols, int* iters);
  bool coarsest_apply_many(T* out, size_t ostride, const T* in, size_t istride, int ncols);   // the coarsest operator itself, all columns (ls_self_kernel + ls_hop_kernel)
  void release_many_workspace() { lockstep_.release(); for (auto& m : multi_) m.release(); }                  // what the *_many entry points allocate lazily
  void import_interpolation_level(int l, const double* P_lex_host);                           // level-l interpolation vectors as they are, then the operators below
  void vcycle(int l, T* phi, T* Dphi, const T* eta, int res);
  // ---- many right-hand sides on the intermediate levels (coarse_multi.h; fp32, single process): level 1 of three levels, levels 1
  // and 2 of four -- the V-cycle of level 1 then runs the K-cycles of level 2 for all columns inside it ------
  // columns: ordinary level-l vectors, column c at base + c * stride.  false if the shape is not covered.
  // multi_ready: level l AND every intermediate level below it take the many-vector path (else none of them does)
  bool multi_ready(int l, int ncols);
  bool multi_apply_many(int l, T* out, size_t ostride, const T* in, size_t istride, int ncols);
  bool multi_smooth_many(int l, T* phi, size_t pstride, const T* eta, size_t estride, int ncols, int cycles, int res);
  bool multi_vcycle_many(int l, T* phi, size_t pstride, const T* eta, size_t estride, int ncols);
  bool multi_kcycle_many(int l, T* x, size_t xstride, const T* b, size_t bstride, int ncols, int* iters);
  int kcycle_solve(int l);                                       // the K-cycle FGMRES of level l on level(l).gm.b -> gm.x, one vector
  // ---- 16-bit storage for the solve (half_storage.h; fp32 V-cycle): bits 32 or 16 per kind ----
  // 16: the kind's products read a 16-bit copy that their first use makes.  Coarse: the one-right-hand-side coarsest Schur complement
  // and apply_op on the coarsest level (odd-even); Transfer: restrict_to(0, ...) and interpolate(0, ...); Intermediate: apply_op(l, ...)
  // and smoother(l, ...) on the levels between, one copy per level (methods 1-3).  32 frees the kind's copies.  The many-vector
  // paths, the Galerkin construction and every setup phase (SetupStorage) read the fp32 numbers whatever the setting.
  void set_storage(StorageKind kind, int bits);
  void set_storage(const StorageBits& b) { for (int k = 0; k < 3; k++) set_storage((StorageKind)k, b.bits[k]); }
  // the two products the coarsest Schur complement is made of, on the sites of one parity (0: even, 1: odd) of the parity-ordered
  // coarsest level, in the storage that is set: CoarseOp::hop / self_mul over that half of the sites (ddamg_hip_coarse_hop, ..._self_mul)
  void coarsest_hop_parity(T* out, const T* in, int parity, double sign, bool accumulate);
  void coarsest_self_mul_parity(T* out, const T* in, int parity, bool inverse);

  int num_levels() const { return (int)lv_.size(); }
  MGLevel<T>& level(int l) { return *lv_[l]; }
  T* coarse_x() { return lv_.back()->gm.x; }
  T* coarse_b() { return lv_.back()->gm.b; }
  int coarse_iter_count = 0;

 private:
  ddamg_hip_params par_;
  const Knobs& knobs_;
  hipStream_t st_;
  Comm* comm_ = nullptr;
  unsigned long long rng_stream_ = 0;
  DeviceBuffer<T> gal_W_, gal_C_;           // batched Galerkin workspace (the bootstrap borrows the two between the builds)
  DeviceBuffer<T> gal_cwork_;               // the same for coarse levels (sized for level 1, the largest)
  int gal_batch_ = 0;
  int gal_slab_aggs_ = 0;                   // > 0: all columns, the lattice in slabs of this many aggregates
 public:
  // wall-clock seconds per setup phase (stream-synchronised), filled when DDAMG_SETUP_TIMING is set
  std::vector<std::pair<std::string, double>> setup_times;
 private:
  double tick(const char* phase, double t0);
  std::vector<std::unique_ptr<MGLevel<T>>> lv_;
  bool p_orthonormal_ = true;   // false after interpolation vectors were imported as they are: then P^H P = 1 cannot be assumed
  DeviceBuffer<int> d_lex0_, d_identity0_;
  DeviceBuffer<double> d_stage_;
  DeviceBuffer<T> W_;        // 5 level-0 vectors (Galerkin)
  DeviceBuffer<T> cwork_;    // coarse work space (5 vectors of the largest coarse level)

  GatheredCoarsest<T> gath_;
  StorageBits storage_;             // a 16-bit copy is allocated by its first use, never while its kind is set to 32
  TransferHalf thalf_;              // the 16-bit copy of the fine level's P
  // the copy that level l's products read in the storage that is set (gathered: those of the gathered coarsest operator), or
  // nullptr: the fp32 couplings
  CoarseHalf* half_of(int l, bool gathered = false) {
    MGLevel<T>& lv = *lv_[l];
    if (sizeof(T) != 4 || l == 0) return nullptr;
    if (lv.coarsest) {
      if (storage_.bits[Coarse] != 16) return nullptr;
      if (gathered) return gath_.cop.distributed() ? nullptr : &gath_.half;
    } else if (storage_.bits[Intermediate] != 16 || par_.method > 3) return nullptr;
    return lv.cop.distributed() ? nullptr : &lv.half;
  }
  // CoarseOp::hop / self_mul of the coarsest level (gathered: of the gathered coarsest operator) in the storage that is set
  void coarsest_hop(bool gathered, T* out, const T* in, int s0, int s1, double sign, bool accumulate);
  void coarsest_self_mul(bool gathered, T* out, const T* in, int s0, int s1, bool inverse);
  // 32-bit storage of all kinds for the lifetime of the object (a setup phase), the settings restored afterwards
  struct SetupStorage {
    StorageBits& bits; const StorageBits saved;
    explicit SetupStorage(Multigrid& mg) : bits(mg.storage_), saved(mg.storage_) { bits = StorageBits(); }
    ~SetupStorage() { bits = saved; }
  };
  LockstepCoarseSolver lockstep_;   // the bootstrap's coarsest-level solves, all test vectors at once (fp32, single process)
  CoarseMulti multi_[DDAMG_HIP_MAX_LEVELS];   // [l]: intermediate level l for all test vectors at once (coarse_multi.h); l = 1, 2
  bool multi_noticed_[DDAMG_HIP_MAX_LEVELS] = {};
  void ensure_lockstep();
  bool multi_refuse(int l, const char* why);                 // the DDAMG_SETUP_TIMING notice, once per level; returns false
  // the K-cycle parameters of the levels below l for the nested V-cycle (chain: storage of the caller); nullptr: l + 1 is the coarsest
  const CoarseMulti::Nested* multi_nested(int l, CoarseMulti::Nested* chain);
  int multi_vcycle(int l, float2* phi, const float2* eta, int ncols);
  int multi_kcycle(int l, float2* X, const float2* B, int ncols, int* iters);
  // test_vector_PRECISION_update of the intermediate levels below l from the K-cycle iterates the last multi_vcycle / multi_kcycle
  // of level l left (the first ncols test vectors of each)
  void multi_update_deeper(int l, int ncols);
  void setup_gathered_coarsest();
  void schur(T* out, const T* in);
  void schur_on(bool gathered, int V, T* t0, T* t1, T* out, const T* in);
  std::vector<int> ref_order0_;   // fine-level vector-loop order of the reference when odd_even == 0
  void smoother_schur(int l, T* out, const T* in);            // (apply_schur_complement / coarse_apply_schur_complement on level l)
  void gmres_smoother(int l, T* phi, const T* eta, int cycles, int res);
  double norm_of(int l, const T* v);
  void random_vector(int l, T* dst);
  void define_interpolation(int l);     // interpolation_PRECISION_define(NULL, level l)
  void re_setup(int l);                 // recursive re_setup_PRECISION
  void build_coarse_operator(int l);    // D_{l+1} = P_l^H D_l P_l
  void orthonormalize(int l);
  void bootstrap(int l, int iters);     // inv_iter_inv_fcycle_PRECISION
  bool bootstrap_vcycles_batched();     // the fine level's Nvec V-cycles with ONE restriction and ONE interpolation for all of them
  T* test_vector(int l, int j) { return l == 0 ? lv_[0]->fip.test_vector(j) : lv_[l]->cip.test_vector(j); }
  T* tv_base(int l) { return l == 0 ? lv_[0]->fip.tv : lv_[l]->cip.tv; }
  size_t tv_stride(int l) { return l == 0 ? lv_[0]->fip.pstride : lv_[l]->cip.pstride; }
};

}  // namespace ddamg
