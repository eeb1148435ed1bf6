// solver.cpp -- setup / solve entry points of the C-ABI (include/ddamg_hip.h) on top of mg.h and krylov.h.
// Reference: method_setup / method_update src/init.c:134-374, wilson_driver src/top_level.c:64-104,
// fgmres_double + preconditioner (mixed precision 1) src/linsolve_generic.c:219-413, src/preconditioner.c:25-69.
#include <chrono>
#include "capi_common.h"
#include "chrono.h"
#include <cstring>
#include <cstdio>
#include <cmath>

using namespace ddamg;

static void ensure_mg(ddamg_hip_ctx* c) {
  if (c->levels[0]->geom.distributed()) {
    DDAMG_REQUIRE(c->comm != nullptr, "process grid > 1 but no transport: call ddamg_hip_comm_init_rccl or ddamg_hip_comm_init_host first");
  }
  DDAMG_REQUIRE(c->have_operator, "no operator set (call ddamg_hip_set_gauge / ddamg_hip_set_operator first)");
  DDAMG_REQUIRE(c->par.num_levels >= 2, "multigrid needs at least two levels");
  DDAMG_REQUIRE(c->par.method >= 1 && c->par.method <= 4, "multigrid preconditioner needs method 1 (additive), 2 (red-black), 3 (sixteen-colour SAP) or 4 (GMRES smoother)");
  std::vector<const Geometry*> geoms;
  for (auto& lv : c->levels) geoms.push_back(&lv->geom);
  if (c->par.mixed_precision == 0) {
    if (!c->mg64) { c->mg64.reset(new Multigrid<double>(c->par, c->knobs, geoms, &c->fop64, c->stream)); c->mg64->set_comm(c->comm); }
  } else {
    if (!c->mg32) { c->mg32.reset(new Multigrid<float>(c->par, c->knobs, geoms, &c->fop32, c->stream)); c->mg32->set_comm(c->comm); c->mg32->set_storage(c->storage); }
  }
}

static void ensure_outer(ddamg_hip_ctx* c) {
  if (c->outer_ready) return;
  const size_t n = (size_t)24 * c->levels[0]->geom.V;
  c->rw_outer.init(c->par.restart + 4);
  // mixed precision 1 with a multigrid preconditioner: the iterates Z_j of the outer FGMRES stay in fp32, as the
  // V-cycle leaves them (Gmres::z_fp32)
  c->outer.single_allreduce = c->knobs.single_allreduce_arnoldi;
  c->outer.z_fp32 = c->par.method >= 1 && c->par.method <= 4 && c->par.mixed_precision == 1;
  // pure CGN keeps its 8 vectors in a 4-vector Krylov structure, as the reference does (src/init.c:178-180)
  c->outer.alloc(n, c->par.method == -1 ? 4 : c->par.restart, c->par.method > 0);
  c->outer.num_restart = c->par.max_restart;
  c->outer.view = whole(n);
  c->outer.st = c->stream;
  c->outer.rw = &c->rw_outer;
  c->outer.track_history = true;
  c->outer.op = [c](double* out, const double* in) { c->fop64.apply(out, in, c->stream); };
  if (c->par.method == 5) {
    // preconditioner(): solve_oddeven with bicgstab to the tolerance the outer iteration sets at the start of every step
    // (src/preconditioner.c:39-55, src/linsolve_generic.c:292-296)
    const Geometry& g0 = c->levels[0]->geom;
    if (c->par.mixed_precision == 0) {
      c->bicg64.init(g0, &c->fop64, c->stream); c->bicg64.set_comm(c->comm);
      c->outer.prec = [c](double* phi, double*, const double* eta, int) { c->bicg64.solve(phi, eta, c->outer.tol); };
    } else {
      c->bicg32.init(g0, &c->fop32, c->stream); c->bicg32.set_comm(c->comm);
      c->p32_in.alloc(n);
      c->p32_out.alloc(n);
      c->outer.prec = [c](double* phi, double*, const double* eta, int) {
        const size_t V = c->levels[0]->geom.V;
        const double rel = c->outer.gamma_jp1 / c->outer.norm_r0;
        const double tol = std::max(1e-3, (c->outer.tol / rel) * 0.5);
        vec_convert<float, double>(c->p32_in, eta, V, 24, c->stream);
        c->bicg32.solve(c->p32_out, c->p32_in, tol);
        vec_convert<double, float>(phi, c->p32_out, V, 24, c->stream);
      };
    }
    c->bicg_ready = true;
  } else if (c->par.method > 0) {
    if (c->par.mixed_precision == 0) {
      c->outer.prec = [c](double* phi, double* Dphi, const double* eta, int res) { c->mg64->vcycle(0, phi, Dphi, eta, res); };
    } else {
      c->p32_in.alloc(n);
      c->p32_out.alloc(n);
      // preconditioner(): trans_float -> vcycle_float -> trans_back_float (src/preconditioner.c:31-33)
      c->outer.prec = [c](double* phi, double* Dphi, const double* eta, int res) {
        const size_t V = c->levels[0]->geom.V;
        vec_convert<float, double>(c->p32_in, eta, V, 24, c->stream);
        c->mg32->vcycle(0, c->p32_out, nullptr, c->p32_in, res);
        vec_convert<double, float>(phi, c->p32_out, V, 24, c->stream);
      };
      if (c->outer.z_fp32) {
        c->outer.sites32 = c->levels[0]->geom.V; c->outer.nreal32 = 24;
        c->outer.prec32 = [c](float* z, const double* eta, int res) {
          vec_convert<float, double>(c->p32_in, eta, c->levels[0]->geom.V, 24, c->stream);
          c->mg32->vcycle(0, z, nullptr, c->p32_in, res);
        };
        c->outer.op32 = [c](double* out, const float* z) { c->fop64.apply_f32in(out, z, c->stream); };
      }
    }
  }
  c->outer_ready = true;
}

// cgn_double (src/linsolve_generic.c:503-640; method -1, src/top_level.c:82-83): conjugate gradients on the normal
// equations D^H D x = D^H b with D^H = g5 D g5 in one pass (FineOp::apply_dagger; d_plus_clover_dagger_PRECISION, src/dirac_generic.c:281-285);
// once the normal-equation residual has dropped by tol the loop goes on on the true residual of D x = b (CGNR phase).
// At most restart*max_restart iterations (src/init.c:179).
static int solve_cgn(ddamg_hip_ctx* c, double tol, double* relres) {
  typedef std::complex<double> cd;
  Gmres<double>& g = c->outer;
  const size_t n = g.vec_elems;
  const View all = whole(n);
  ReduceWork& rw = c->rw_outer;
  hipStream_t st = c->stream;
  double *x = g.x, *b = g.b, *r_true = g.r, *p = g.w, *pp = g.V(0), *Dp = g.V(1), *r_old = g.V(2), *r_new = g.V(3);
  auto D = [&](double* out, const double* in) { c->fop64.apply(out, in, st); };
  auto Ddag = [&](double* out, const double* in) { c->fop64.apply_dagger(out, in, st); };
  auto dot = [&](const double* a, const double* v) {   // <a, v>, conjugate-linear in a
    vec_multi_dot<double>(a, 0, 1, v, all, rw, rw.d_result, st);
    DDAMG_HIP_CHECK(hipMemcpyAsync(rw.h_result, rw.d_result, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    DDAMG_HIP_CHECK(hipStreamSynchronize(st));
    return cd(rw.h_result[0], rw.h_result[1]);
  };
  auto norm = [&](const double* a) { return host_norm<double>(a, all, rw, st); };
  auto axpy = [&](double* z, const double* xx, const double* y, cd a) { vec_axpy<double>(z, xx, y, a.real(), a.imag(), all, st); };
  const int maxiter = c->par.restart * c->par.max_restart;
  int iter = 0;
  vec_zero<double>(x, all, st);
  D(Dp, x);
  vec_minus<double>(pp, b, Dp, all, st);
  Ddag(r_old, pp);
  vec_copy<double>(p, r_old, all, st);
  double r0_norm = norm(r_old);
  cd prod_rr_old = dot(r_old, r_old);
  c->last_history.clear();
  if (!(r0_norm > 0)) { *relres = 0; return 0; }
  auto step = [&](bool true_residual, double* r_norm) {
    D(pp, p);
    Ddag(Dp, pp);
    const cd alpha = prod_rr_old / dot(p, Dp);
    axpy(x, x, p, alpha);
    axpy(r_new, r_old, Dp, -alpha);
    if (true_residual) { axpy(r_true, r_true, pp, -alpha); *r_norm = norm(r_true); }
    const cd gamma = dot(r_new, r_new);
    const cd beta = gamma / prod_rr_old;
    axpy(p, r_new, p, beta);
    vec_copy<double>(r_old, r_new, all, st);
    prod_rr_old = gamma;
  };
  while (std::sqrt(prod_rr_old.real()) / r0_norm > tol && iter < maxiter) {
    iter++;
    step(false, nullptr);
    c->last_history.push_back(std::sqrt(prod_rr_old.real()) / r0_norm);
  }
  r0_norm = norm(b);
  D(Dp, x);
  vec_minus<double>(r_true, b, Dp, all, st);
  double r_norm = norm(r_true);
  while (r_norm / r0_norm > tol && iter < maxiter) {
    iter++;
    step(true, &r_norm);
    c->last_history.push_back(r_norm / r0_norm);
  }
  // reported residual: the true one, recomputed (the reference prints it the same way, :612-615)
  D(Dp, x);
  vec_minus<double>(pp, b, Dp, all, st);
  *relres = norm(pp) / r0_norm;
  return iter;
}

// fgmres_MP (src/linsolve.c:153-300): outer loop in fp64 (true residual, solution update), one restart
// cycle of right-preconditioned FGMRES in fp32 per outer step; the cycle stops when the fp64 target is
// met (gamma/||r0|| < tol) or when it has gained max(tol,1e-5) on its own start residual.
static void ensure_mp(ddamg_hip_ctx* c) {
  if (c->mp_ready) return;
  const size_t n = (size_t)24 * c->levels[0]->geom.V;
  c->rw_mp.init(c->par.restart + 4);
  c->mp_inner.single_allreduce = c->knobs.single_allreduce_arnoldi;
  c->mp_inner.alloc(n, c->par.restart, c->par.method > 0);
  c->mp_inner.num_restart = 1;
  c->mp_inner.view = whole(n);
  c->mp_inner.st = c->stream;
  c->mp_inner.rw = &c->rw_mp;
  c->mp_inner.breakdown_tol = 1e-15;
  c->mp_inner.track_history = true;
  c->mp_inner.op = [c](float* out, const float* in) { c->fop32.apply(out, in, c->stream); };
  if (c->par.method > 0) {
    // arnoldi_step_MP: prec( Z[j], w, V[j], _NO_RES ) -- the smoother hands back w = D Z[j] (src/linsolve.c:338-343)
    c->mp_inner.prec = [c](float* phi, float* Dphi, const float* eta, int res) { c->mg32->vcycle(0, phi, c->par.method <= 2 ? Dphi : nullptr, eta, res); };
    c->mp_inner.prec_gives_Dphi = c->par.method <= 2;   // g.method >= 1 && g.method <= 2, src/linsolve.c:338
  }
  for (DeviceBuffer<double>* p : {&c->mp_x, &c->mp_b, &c->mp_r}) p->alloc(n);
  if (!c->rw_blas_ready) { c->rw_blas.init(8); c->rw_blas_ready = true; }
  c->mp_ready = true;
}

static int solve_mp(ddamg_hip_ctx* c, double tol, double* relres) {
  const size_t V = c->levels[0]->geom.V, n = 24 * V;
  const View all = whole(n);
  ReduceWork& rw = c->rw_blas;
  Gmres<float>& in = c->mp_inner;
  int iter = 0, finish = 0;
  double norm_r0 = 1, gamma_jp1 = 1;
  c->last_history.clear();
  auto dnorm = [&](const double* v) { return host_norm<double>(v, all, rw, c->stream); };
  for (int ol = 0; ol < c->par.max_restart && !finish; ol++) {
    if (ol == 0) vec_copy<double>(c->mp_r, c->mp_b, all, c->stream);
    else { c->fop64.apply(c->mp_r, c->mp_x, c->stream); vec_minus<double>(c->mp_r, c->mp_b, c->mp_r, all, c->stream); }
    const double gamma0 = dnorm(c->mp_r);
    if (ol == 0) norm_r0 = gamma0;
    if (!(gamma0 > 0)) { gamma_jp1 = 0; break; }
    vec_convert<float, double>(in.b, c->mp_r, V, 24, c->stream);
    in.initial_guess_zero = true;
    in.tol = std::max(tol * norm_r0 / gamma0, std::max(tol, 1e-5));
    const int it = in.solve();
    iter += it;
    gamma_jp1 = in.gamma_jp1 * (gamma0 / in.norm_r0);
    for (double h : in.history) c->last_history.push_back(h * gamma0 / norm_r0);
    if (gamma_jp1 / norm_r0 < tol || gamma_jp1 / norm_r0 > 1e5 || it == 0) finish = 1;
    // x += (correction of this cycle), accumulated in fp64
    vec_convert<double, float>(c->mp_r, in.x, V, 24, c->stream);
    if (ol == 0) vec_copy<double>(c->mp_x, c->mp_r, all, c->stream);
    else vec_plus<double>(c->mp_x, c->mp_x, c->mp_r, all, c->stream);
  }
  // FGMRES_RESTEST
  c->fop64.apply(c->mp_r, c->mp_x, c->stream);
  vec_minus<double>(c->mp_r, c->mp_b, c->mp_r, all, c->stream);
  *relres = norm_r0 > 0 ? dnorm(c->mp_r) / norm_r0 : 0.0;
  return iter;
}

// coarsest-level iterations since the last reset, of whichever hierarchy exists
static void reset_coarse_iterations(ddamg_hip_ctx* c) { for_each_mg(c, [](auto& mg) { mg.coarse_iter_count = 0; }); }
static int coarse_iterations_of(ddamg_hip_ctx* c) {
  int n = 0;
  for_each_mg(c, [&](auto& mg) { n += mg.coarse_iter_count; });
  return n;
}

static void shift_mass_or_throw(ddamg_hip_ctx* c, double m0) {
  if (ddamg_hip_shift_mass(c, m0)) throw std::runtime_error(g_ddamg_last_error);
}

// the num_vect[0] fine-level vectors column(mg, k) names, one after the other in lattice order into host memory
template <typename Column>
static void download_columns(ddamg_hip_ctx* c, double* host_lex, Column column) {
  const int V = c->levels[0]->geom.V;
  const size_t nel = (size_t)24 * V;
  double* st = c->stage(sizeof(double) * nel);
  with_mg(c, [&](auto& mg) {
    for (int k = 0; k < c->par.num_vect[0]; k++) {
      vec_to_lex(st, column(mg, k), c->levels[0]->d_lex_of_site, V, 12, c->stream);
      DDAMG_HIP_CHECK(hipMemcpyAsync(host_lex + (size_t)k * nel, st, sizeof(double) * nel, hipMemcpyDeviceToHost, c->stream));
      DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
  });
}

// the vector's numbers, once it is known to live on `level` in the precision of the hierarchy
template <typename MG>
static typename MG::real* check_vec(const MG&, const ddamg_hip_vec* v, int level) {
  DDAMG_REQUIRE(v && v->level == level, "vector lives on the wrong level");
  DDAMG_REQUIRE(v->precision == 8 * (int)sizeof(typename MG::real), "vector precision does not match the V-cycle precision");
  return vec_data<typename MG::real>(v);
}

// whole-vector copy between a vector of the boundary and one that a Krylov solver owns
static void copy_bytes(ddamg_hip_ctx* c, void* dst, const void* src, const ddamg_hip_vec* shape) {
  DDAMG_HIP_CHECK(hipMemcpyAsync(dst, src, shape->data.bytes(), hipMemcpyDeviceToDevice, c->stream));
}

// ---- many right-hand sides on a coarse level: the kernels of the batched setup through the boundary (tests, measurements) ----
namespace {
// columns next to each other in one device buffer, as the bootstrap holds them
struct Columns {
  DeviceBuffer<float> p; size_t cs = 0;
  Columns(size_t cs_, int ncols) : cs(cs_) { p.alloc(cs * ncols); }
};
// the level the columns a[k], b[k] live on, once every one of them is known to be an fp32 vector of that coarse level
int many_level(ddamg_hip_ctx* c, int ncols, ddamg_hip_vec* const* a, const ddamg_hip_vec* const* b) {
  DDAMG_REQUIRE(a && b, "null context or null vector array");
  DDAMG_REQUIRE(c->mg32, "the many-right-hand-side entry points need the fp32 hierarchy (mixed_precision >= 1)");
  DDAMG_REQUIRE(ncols >= 2 && ncols <= 32, "2 <= ncols <= 32");
  for (int k = 0; k < ncols; k++) DDAMG_REQUIRE(a[k] && b[k], "null vector among the columns");
  const int lvl = a[0]->level;
  DDAMG_REQUIRE(lvl >= 1 && lvl < c->par.num_levels, "coarse-level vectors expected");
  for (int k = 0; k < ncols; k++) { check_vec(*c->mg32, a[k], lvl); check_vec(*c->mg32, b[k], lvl); }
  return lvl;
}
void pack(ddamg_hip_ctx* c, Columns& C, const ddamg_hip_vec* const* v, int ncols) {
  for (int k = 0; k < ncols; k++) DDAMG_HIP_CHECK(hipMemcpyAsync(C.p + (size_t)k * C.cs, v[k]->data.get(), v[k]->data.bytes(), hipMemcpyDeviceToDevice, c->stream));
}
void unpack(ddamg_hip_ctx* c, ddamg_hip_vec* const* v, const Columns& C, int ncols) {
  for (int k = 0; k < ncols; k++) DDAMG_HIP_CHECK(hipMemcpyAsync(v[k]->data.get(), C.p + (size_t)k * C.cs, v[k]->data.bytes(), hipMemcpyDeviceToDevice, c->stream));
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
}
// the body of a *_many entry point: the columns of `in` (and, where the call starts from them, of `out`) packed, call(mg, level, O, I)
// on the packed columns, O back into `out` where it returned true, the many-vector workspace released, `not_covered` thrown where not
template <typename Call>
void many_call(ddamg_hip_ctx* c, int ncols, ddamg_hip_vec* const* out, const ddamg_hip_vec* const* in, bool out_is_input, const char* not_covered, Call call) {
  const int lvl = many_level(c, ncols, out, in);
  const size_t cs = in[0]->data.bytes() / sizeof(float);
  Columns I(cs, ncols), O(cs, ncols);     // freed on every path out of here
  pack(c, I, in, ncols);
  if (out_is_input) pack(c, O, out, ncols);
  const bool ok = call(*c->mg32, lvl, O, I);
  if (ok) unpack(c, out, O, ncols);
  c->mg32->release_many_workspace();      // the batches are setup workspace: not kept next to the production solves
  DDAMG_REQUIRE(ok, not_covered);
}
}  // namespace

extern "C" {

static int setup_impl(ddamg_hip_ctx* c, int setup_iterations, int* coarse_iterations, const double* setup_m0);
int ddamg_hip_setup(ddamg_hip_ctx* c, int setup_iterations, int* coarse_iterations) { return setup_impl(c, setup_iterations, coarse_iterations, nullptr); }
int ddamg_hip_setup_at_mass(ddamg_hip_ctx* c, int setup_iterations, double setup_m0, int* coarse_iterations) { return setup_impl(c, setup_iterations, coarse_iterations, &setup_m0); }

// method_setup, then -- on the operator shifted to *setup_m0 where that is given and differs (method_update, src/init.c:326-357) --
// the iterative setup, then the solver mass again; ONE lifetime of the setup workspace around all of it
static int setup_impl(ddamg_hip_ctx* c, int setup_iterations, int* coarse_iterations, const double* setup_m0) {
  DDAMG_API_BEGIN
  enter(c);
  if (c->par.method == 5) {   // no hierarchy: the reference switches the interpolation off (src/init.c:976-979)
    if (coarse_iterations) *coarse_iterations = 0;
    c->setup_done = true;
    return 0;
  }
  const auto wall = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_h0 = wall();
  ensure_mg(c);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  const double t_hier = wall() - t_h0;
  const int iters = setup_iterations < 0 ? c->par.setup_iter[0] : setup_iterations;
  const double solver_m0 = c->par.m0;
  const bool other_mass = setup_m0 != nullptr && *setup_m0 != solver_m0 && iters > 0;
  with_mg(c, [&](auto& mg) {
    mg.coarse_iter_count = 0;
    mg.initial_setup();
    c->setup_done = true;       // the hierarchy exists: the mass shift below reaches every level
    if (other_mass) shift_mass_or_throw(c, *setup_m0);
    try {
      mg.iterative_setup(iters);
    } catch (...) {
      // no exit at the setup mass, and no hierarchy that stopped half-way through an iteration behind setup_done
      if (other_mass) (void)ddamg_hip_shift_mass(c, solver_m0);
      c->setup_done = false;
      throw;
    }
    if (other_mass) shift_mass_or_throw(c, solver_m0);
    if (coarse_iterations) *coarse_iterations = mg.coarse_iter_count;
    const double t_r0 = wall();
    mg.release_setup_workspace();
    const double t_rel = wall() - t_r0;
    if (mg.setup_times.empty()) return;      // DDAMG_SETUP_TIMING not set
    fprintf(stderr, "[ddamg setup] %-28s %8.3f s\n", "hierarchy: tables, buffers", t_hier);
    for (auto& e : mg.setup_times) fprintf(stderr, "[ddamg setup] %-28s %8.3f s\n", e.first.c_str(), e.second);
    fprintf(stderr, "[ddamg setup] %-28s %8.3f s\n", "workspace released", t_rel);
  });
  DDAMG_API_END
}

int ddamg_hip_setup_update(ddamg_hip_ctx* c, int iterations, int* coarse_iterations) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->setup_done, "setup has not been run");
  with_mg(c, [&](auto& mg) {
    mg.coarse_iter_count = 0;
    mg.iterative_setup(iterations);
    if (coarse_iterations) *coarse_iterations = mg.coarse_iter_count;
    mg.release_setup_workspace();
  });
  DDAMG_API_END
}

int ddamg_hip_set_test_vectors(ddamg_hip_ctx* c, const double* tv_lex, int orthonormalised) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(tv_lex, "null argument");
  ensure_mg(c);
  with_mg(c, [&](auto& mg) {
    if (orthonormalised) mg.import_interpolation(tv_lex); else mg.import_test_vectors(tv_lex);
    mg.release_setup_workspace();
  });
  c->setup_done = true;
  DDAMG_API_END
}

int ddamg_hip_get_interpolation(ddamg_hip_ctx* c, double* P_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->setup_done && P_lex, "setup has not been run");
  // P is stored aggregate by aggregate (transfer.hip): column k into a vector in lattice order first
  download_columns(c, P_lex, [&](auto& mg, int k) {
    real_of<decltype(mg)>* v = mg.level(0).buf[0];
    mg.level(0).fip.get_column(k, v, c->stream);
    return v;
  });
  DDAMG_API_END
}

int ddamg_hip_get_test_vectors(ddamg_hip_ctx* c, double* tv_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->setup_done && tv_lex, "setup has not been run");
  download_columns(c, tv_lex, [](auto& mg, int k) { return mg.level(0).fip.test_vector(k); });
  DDAMG_API_END
}

int ddamg_hip_get_coarse_operator_level(ddamg_hip_ctx* c, int level, double* D_lex, double* clover_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->setup_done, "setup has not been run");
  DDAMG_REQUIRE(level >= 1 && level < c->par.num_levels, "coarse operator: 1 <= level < num_levels");
  with_mg(c, [&](auto& mg) { mg.level(level).cop.export_reference(c->levels[level]->geom, D_lex, clover_lex, c->stream); });
  DDAMG_API_END
}
int ddamg_hip_get_coarse_operator(ddamg_hip_ctx* c, double* D_lex, double* clover_lex) { return ddamg_hip_get_coarse_operator_level(c, 1, D_lex, clover_lex); }

int ddamg_hip_set_coarse_operator_level(ddamg_hip_ctx* c, int level, const double* D_lex, const double* clover_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(D_lex && clover_lex, "null argument");
  DDAMG_REQUIRE(level >= 1 && level < c->par.num_levels, "coarse operator: 1 <= level < num_levels");
  ensure_mg(c);
  with_mg(c, [&](auto& mg) {
    mg.level(level).cop.import_reference(c->levels[level]->geom, D_lex, clover_lex, c->stream);
    if (level == c->par.num_levels - 1) mg.regather_coarsest_operator();
  });
  DDAMG_API_END
}
int ddamg_hip_set_coarse_operator(ddamg_hip_ctx* c, const double* D_lex, const double* clover_lex) { return ddamg_hip_set_coarse_operator_level(c, 1, D_lex, clover_lex); }

int ddamg_hip_set_interpolation_level(ddamg_hip_ctx* c, int level, const double* P_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(P_lex, "null argument");
  DDAMG_REQUIRE(level >= 0 && level + 1 < c->par.num_levels, "interpolation vectors: 0 <= level < num_levels - 1");
  ensure_mg(c);
  with_mg(c, [&](auto& mg) { mg.import_interpolation_level(level, P_lex); mg.release_setup_workspace(); });
  c->setup_done = true;
  DDAMG_API_END
}

int ddamg_hip_smoother(ddamg_hip_ctx* c, ddamg_hip_vec* phi, const ddamg_hip_vec* eta, int cycles, int initial_guess_zero) {
  DDAMG_API_BEGIN
  enter(c);
  ensure_mg(c);
  DDAMG_REQUIRE(phi && phi->level >= 0 && phi->level + 1 < c->par.num_levels, "smoother: the coarsest level has none");
  const int lvl = phi->level;
  with_mg(c, [&](auto& mg) { mg.smoother(lvl, check_vec(mg, phi, lvl), nullptr, check_vec(mg, eta, lvl), cycles, initial_guess_zero ? NO_RES : RES); });
  DDAMG_API_END
}

int ddamg_hip_restrict(ddamg_hip_ctx* c, ddamg_hip_vec* coarse, const ddamg_hip_vec* fine) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->setup_done, "setup has not been run");
  DDAMG_REQUIRE(fine && fine->level >= 0 && fine->level + 1 < c->par.num_levels, "restrict: no coarser level below this vector");
  with_mg(c, [&](auto& mg) { mg.restrict_to(fine->level, check_vec(mg, coarse, fine->level + 1), check_vec(mg, fine, fine->level)); });
  DDAMG_API_END
}

int ddamg_hip_interpolate(ddamg_hip_ctx* c, ddamg_hip_vec* fine, const ddamg_hip_vec* coarse, int add) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->setup_done, "setup has not been run");
  DDAMG_REQUIRE(fine && fine->level >= 0 && fine->level + 1 < c->par.num_levels, "interpolate: no coarser level below this vector");
  with_mg(c, [&](auto& mg) { mg.interpolate(fine->level, check_vec(mg, fine, fine->level), check_vec(mg, coarse, fine->level + 1), add != 0); });
  DDAMG_API_END
}

int ddamg_hip_coarse_apply(ddamg_hip_ctx* c, ddamg_hip_vec* out, const ddamg_hip_vec* in) {
  DDAMG_API_BEGIN
  enter(c);
  with_mg(c, [&](auto& mg) {
    DDAMG_REQUIRE(out && in && out->level >= 1 && out->level == in->level, "coarse vectors of one level expected");
    mg.apply_op(out->level, check_vec(mg, out, out->level), check_vec(mg, in, in->level));
  }, "no coarse operator");
  DDAMG_API_END
}

int ddamg_hip_coarse_hop(ddamg_hip_ctx* c, ddamg_hip_vec* out, const ddamg_hip_vec* in, int parity, double sign, int accumulate) {
  DDAMG_API_BEGIN
  enter(c);
  const int lc = c->par.num_levels - 1;
  with_mg(c, [&](auto& mg) {
    auto* o = check_vec(mg, out, lc); auto* i = check_vec(mg, in, lc);
    DDAMG_REQUIRE(o != i, "in-place hopping term is not supported");
    mg.coarsest_hop_parity(o, i, parity, sign, accumulate != 0);
  }, "no coarse operator");
  DDAMG_API_END
}

int ddamg_hip_coarse_self_mul(ddamg_hip_ctx* c, ddamg_hip_vec* out, const ddamg_hip_vec* in, int parity, int inverse) {
  DDAMG_API_BEGIN
  enter(c);
  const int lc = c->par.num_levels - 1;
  with_mg(c, [&](auto& mg) {
    auto* o = check_vec(mg, out, lc); auto* i = check_vec(mg, in, lc);
    DDAMG_REQUIRE(o != i, "in-place self coupling is not supported");
    mg.coarsest_self_mul_parity(o, i, parity, inverse != 0);
  }, "no coarse operator");
  DDAMG_API_END
}

int ddamg_hip_coarse_solve(ddamg_hip_ctx* c, ddamg_hip_vec* x, const ddamg_hip_vec* b, int* iterations) {
  DDAMG_API_BEGIN
  enter(c);
  const int lc = c->par.num_levels - 1;   // the coarsest level
  with_mg(c, [&](auto& mg) {
    check_vec(mg, x, lc);
    copy_bytes(c, mg.coarse_b(), check_vec(mg, b, lc), b);
    const int it = mg.coarse_solve();
    copy_bytes(c, x->data.get(), mg.coarse_x(), x);
    if (iterations) *iterations = it;
  }, "no coarse operator");
  DDAMG_API_END
}

int ddamg_hip_vcycle(ddamg_hip_ctx* c, ddamg_hip_vec* phi, const ddamg_hip_vec* eta) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->setup_done, "setup has not been run");
  DDAMG_REQUIRE(phi && phi->level >= 0 && phi->level + 1 < c->par.num_levels, "vcycle: the coarsest level has none");
  const int lvl = phi->level;
  with_mg(c, [&](auto& mg) { mg.vcycle(lvl, check_vec(mg, phi, lvl), nullptr, check_vec(mg, eta, lvl), NO_RES); });
  DDAMG_API_END
}

int ddamg_hip_kcycle(ddamg_hip_ctx* c, ddamg_hip_vec* x, const ddamg_hip_vec* b, int* iterations) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->setup_done && x && b, "setup has not been run");
  const int lvl = x->level;
  DDAMG_REQUIRE(lvl >= 1 && lvl + 1 < c->par.num_levels, "kcycle: an intermediate level");
  with_mg(c, [&](auto& mg) {
    check_vec(mg, x, lvl);
    copy_bytes(c, mg.level(lvl).gm.b, check_vec(mg, b, lvl), b);
    const int it = mg.kcycle_solve(lvl);
    copy_bytes(c, x->data.get(), mg.level(lvl).gm.x, x);
    if (iterations) *iterations = it;
  });
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

// kept apart from many_call: a column comes back only where its solve converged (iterations[k] >= 0), and the level is the coarsest
int ddamg_hip_coarse_solve_many(ddamg_hip_ctx* c, int ncols, ddamg_hip_vec* const* x, const ddamg_hip_vec* const* b, int* iterations) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->mg32 && x && b && iterations, "coarse_solve_many needs the fp32 hierarchy (mixed_precision >= 1)");
  DDAMG_REQUIRE(ncols >= 2 && ncols <= 32, "2 <= ncols <= 32");
  const int lc = c->par.num_levels - 1;
  for (int k = 0; k < ncols; k++) { check_vec(*c->mg32, x[k], lc); check_vec(*c->mg32, b[k], lc); }
  const size_t cs = b[0]->data.bytes() / sizeof(float);
  Columns B(cs, ncols), X(cs, ncols);     // freed on every path out of here
  pack(c, B, b, ncols);
  const bool ok = c->mg32->coarse_solve_many(X.p, cs, B.p, cs, ncols, iterations);
  if (ok)
    for (int k = 0; k < ncols; k++)
      if (iterations[k] >= 0) DDAMG_HIP_CHECK(hipMemcpyAsync(x[k]->data.get(), X.p + (size_t)k * cs, x[k]->data.bytes(), hipMemcpyDeviceToDevice, c->stream));
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->mg32->release_many_workspace();      // the lockstep batches are setup workspace: not kept next to the production solves
  DDAMG_REQUIRE(ok, "coarse_solve_many: shape not covered (fp32, single process, odd-even, at most 64 dof per site)");
  DDAMG_API_END
}

int ddamg_hip_coarse_apply_many(ddamg_hip_ctx* c, int ncols, ddamg_hip_vec* const* out, const ddamg_hip_vec* const* in) {
  DDAMG_API_BEGIN
  enter(c);
  many_call(c, ncols, out, in, false, "coarse_apply_many: shape not covered (fp32, single process; the coarsest level, or an intermediate level of three or four levels)",
            [&](Multigrid<float>& mg, int lvl, Columns& O, Columns& I) {
              return lvl == c->par.num_levels - 1 ? mg.coarsest_apply_many(O.p, O.cs, I.p, I.cs, ncols) : mg.multi_apply_many(lvl, O.p, O.cs, I.p, I.cs, ncols);
            });
  DDAMG_API_END
}

int ddamg_hip_smoother_many(ddamg_hip_ctx* c, int ncols, ddamg_hip_vec* const* phi, const ddamg_hip_vec* const* eta, int cycles, int initial_guess_zero) {
  DDAMG_API_BEGIN
  enter(c);
  many_call(c, ncols, phi, eta, true, "smoother_many: shape not covered (an intermediate level of three or four levels, red-black Schwarz, fp32, single process)",
            [&](Multigrid<float>& mg, int lvl, Columns& P, Columns& E) { return mg.multi_smooth_many(lvl, P.p, P.cs, E.p, E.cs, ncols, cycles, initial_guess_zero ? NO_RES : RES); });
  DDAMG_API_END
}

int ddamg_hip_vcycle_many(ddamg_hip_ctx* c, int ncols, ddamg_hip_vec* const* phi, const ddamg_hip_vec* const* eta) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->setup_done, "setup has not been run");
  many_call(c, ncols, phi, eta, false, "vcycle_many: shape not covered (an intermediate level of three or four levels, red-black Schwarz, fp32, single process)",
            [&](Multigrid<float>& mg, int lvl, Columns& P, Columns& E) { return mg.multi_vcycle_many(lvl, P.p, P.cs, E.p, E.cs, ncols); });
  DDAMG_API_END
}

int ddamg_hip_kcycle_many(ddamg_hip_ctx* c, int ncols, ddamg_hip_vec* const* x, const ddamg_hip_vec* const* b, int* iterations) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(iterations, "null context, null vector array or null iteration counts");
  DDAMG_REQUIRE(c->setup_done, "setup has not been run");
  many_call(c, ncols, x, b, false, "kcycle_many: shape not covered (an intermediate level of three or four levels with the K-cycle, red-black Schwarz, fp32, single process)",
            [&](Multigrid<float>& mg, int lvl, Columns& X, Columns& B) { return mg.multi_kcycle_many(lvl, X.p, X.cs, B.p, B.cs, ncols, iterations); });
  DDAMG_API_END
}

}  // extern "C"

// the solve proper, on device vectors in the fine fp64 layout: load_b(dst) fills the right-hand side, store_x(src)
// takes the solution
template <typename LoadB, typename StoreX>
static void solve_core(ddamg_hip_ctx* c, double tol, LoadB load_b, StoreX store_x, int* iterations, int* coarse_iterations, double* relres) {
  DDAMG_REQUIRE(c->have_operator, "no operator set");
  DDAMG_REQUIRE(c->par.method <= 0 || c->par.method == 5 || c->setup_done, "setup has not been run");
  int it; double rr = 0;
  if (c->bicg_ready) { c->bicg32.total_iter = 0; c->bicg64.total_iter = 0; }
  reset_coarse_iterations(c);
  if (c->par.method == -1) {
    ensure_outer(c);
    load_b(c->outer.b);
    it = solve_cgn(c, tol > 0 ? tol : c->par.tol, &rr);
    store_x(c->outer.x);
  } else if (c->par.mixed_precision == 2) {
    ensure_mp(c);
    load_b(c->mp_b);
    it = solve_mp(c, tol > 0 ? tol : c->par.tol, &rr);
    store_x(c->mp_x);
  } else {
    ensure_outer(c);
    load_b(c->outer.b);
    c->outer.tol = tol > 0 ? tol : c->par.tol;
    c->outer.initial_guess_zero = true;
    it = c->outer.solve();
    // FGMRES_RESTEST: true residual in the outer precision (src/linsolve_generic.c:351-357)
    rr = c->outer.norm_r0 > 0 ? c->outer.true_residual() : 0.0;
    store_x(c->outer.x);
    c->last_history = c->outer.history;
  }
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->last_iter = it;
  c->last_coarse_iter = c->par.method == 5 ? c->bicg32.total_iter + c->bicg64.total_iter   // inner BiCGstab iterations
                                           : coarse_iterations_of(c);
  c->last_relres = rr;
  if (iterations) *iterations = it;
  if (coarse_iterations) *coarse_iterations = c->last_coarse_iter;
  if (relres) *relres = rr;
}

// the multigrid preconditioner on one vector, with the callbacks of solve_core
template <typename Load, typename Store>
static void precondition_core(ddamg_hip_ctx* c, Load load, Store store) {
  ensure_outer(c);
  load(c->outer.b);
  reset_coarse_iterations(c);
  c->outer.prec(c->outer.x, nullptr, c->outer.b, NO_RES);
  store(c->outer.x);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->last_coarse_iter = coarse_iterations_of(c);
}

// load / store callbacks for a fine vector `lex` in lattice order: in device memory, or (st given) in host memory through that staging buffer;
// g5: gamma5 times the vector arrives (the D^dagger solves)
static auto load_lex(ddamg_hip_ctx* c, const double* lex, double* st = nullptr, bool g5 = false) {
  return [=](double* dst) {
    const int V = c->levels[0]->geom.V;
    if (st) DDAMG_HIP_CHECK(hipMemcpyAsync(st, lex, sizeof(double) * 24 * V, hipMemcpyHostToDevice, c->stream));
    vec_from_lex<double>(dst, st ? st : lex, c->levels[0]->d_lex_of_site, V, 12, c->stream, g5);
  };
}
static auto store_lex(ddamg_hip_ctx* c, double* lex, double* st = nullptr, bool g5 = false) {
  return [=](const double* src) {
    const int V = c->levels[0]->geom.V;
    vec_to_lex<double>(st ? st : lex, src, c->levels[0]->d_lex_of_site, V, 12, c->stream, g5);
    if (st) DDAMG_HIP_CHECK(hipMemcpyAsync(lex, st, sizeof(double) * 24 * V, hipMemcpyDeviceToHost, c->stream));
  };
}
// the two fine fp64 vectors of a *_vec solve
static void require_solve_vecs(const ddamg_hip_vec* x, const ddamg_hip_vec* b, const char* msg) {
  DDAMG_REQUIRE(x && b, "null argument");
  DDAMG_REQUIRE(x->level == 0 && b->level == 0 && x->precision == 64 && b->precision == 64, msg);
}
// load / store callbacks for fine fp64 vectors of the boundary (or of the solver's layout); g5: gamma5 times the vector arrives
static auto load_dev(ddamg_hip_ctx* c, const double* v, bool g5 = false) {
  return [=](double* dst) {
    const View all = whole((size_t)24 * c->levels[0]->geom.V);
    if (g5) vec_gamma5<double>(dst, v, all, c->stream); else vec_copy<double>(dst, v, all, c->stream);
  };
}
static auto store_dev(ddamg_hip_ctx* c, double* v, bool g5 = false) {
  return [=](const double* src) {
    const View all = whole((size_t)24 * c->levels[0]->geom.V);
    if (g5) vec_gamma5<double>(v, src, all, c->stream); else vec_copy<double>(v, src, all, c->stream);
  };
}

// ||b - D^dagger D x|| / ||b|| in fp64: load_b(dst) fills the plain b; y and t are workspace
template <typename LoadB>
static double squared_residual(ddamg_hip_ctx* c, const double* x, LoadB load_b, double* y, double* t) {
  const View all = whole((size_t)24 * c->levels[0]->geom.V);
  ReduceWork& rw = blas_rw(c);
  c->fop64.apply(t, x, c->stream);
  c->fop64.apply_dagger(y, t, c->stream);
  load_b(t);
  const double nb = host_norm<double>(t, all, rw, c->stream);
  vec_minus<double>(t, t, y, all, c->stream);
  return nb > 0 ? host_norm<double>(t, all, rw, c->stream) / nb : 0.0;
}

// D^dagger D x = b by two solves through the hierarchy of D: y = gamma5 D^-1 gamma5 b (the signs in the callbacks load_g5b and, here,
// in the store of y), then x = D^-1 y.  y and the residual's workspace live for this call only; load_b(dst) fills the plain b once more
// for the residual of the system the caller asked for, ||b - D^dagger D x|| / ||b||, in fp64.
template <typename LoadG5B, typename LoadB, typename StoreX>
static void solve_squared_core(ddamg_hip_ctx* c, double tol, LoadG5B load_g5b, LoadB load_b, StoreX store_x, int* iterations, int* coarse_iterations,
                               double* relres) {
  const size_t n = (size_t)24 * c->levels[0]->geom.V;
  DeviceBuffer<double> y, t;
  y.alloc(n);
  t.alloc(n);
  solve_core(c, tol, load_g5b, store_dev(c, y, true), iterations, coarse_iterations, nullptr);
  double rr = 0;
  solve_core(c, tol, load_dev(c, y), [&](const double* x) {
    rr = squared_residual(c, x, load_b, y, t);
    store_x(x);
  }, iterations ? iterations + 1 : nullptr, coarse_iterations ? coarse_iterations + 1 : nullptr, nullptr);
  c->last_relres = rr;
  if (relres) *relres = rr;
}

// the two arrays of a *_device entry point: in the memory of the context's device, and apart
static void require_device_pair(ddamg_hip_ctx* c, double* out, const double* in, const char* name) {
  const size_t nb = sizeof(double) * 24 * c->levels[0]->geom.V;
  ddamg_require_device_array(c, out, nb, name);
  ddamg_require_device_array(c, in, nb, name);
  ddamg_require_disjoint(out, in, nb, name);
}

// ---- solves from a starting vector, and the guess extrapolated from past solutions (chrono.h) -----------------------------------
static void require_system(int system) {
  DDAMG_REQUIRE(system == DDAMG_HIP_SYSTEM_D || system == DDAMG_HIP_SYSTEM_DDAGGER, "system: 0 (D x = b) or 1 (D^dagger x = b)");
}
static void apply_system(ddamg_hip_ctx* c, int system, double* out, const double* in) {
  if (system == DDAMG_HIP_SYSTEM_DDAGGER) c->fop64.apply_dagger(out, in, c->stream); else c->fop64.apply(out, in, c->stream);
}
// r = b - y (r == b allowed); returns (||b||, ||r||), both from the one reduction of chrono_residual
static std::pair<double, double> residual_norms(ddamg_hip_ctx* c, double* r, const double* b, const double* y) {
  ReduceWork& rw = blas_rw(c);
  chrono_residual(r, b, y, whole((size_t)24 * c->levels[0]->geom.V), rw, rw.d_result, c->stream);
  publish_to_host(rw.d_result, 2, rw, c->stream);
  wait_published(rw, c->stream);
  return {std::sqrt(rw.h_result[0]), std::sqrt(rw.h_result[1])};
}

// A x = b from a guess, A = D or D^dagger by `system`, in residual-correction form through solve_core: r0 = b - A x0, A e = r0 from
// zero to tol ||b|| / ||r0||, x = x0 + e.  load_x(dst) fills the guess, load_b(dst) the right-hand side (twice: once more for the
// residual of the x that is returned), store_x(src) takes the solution; all three in the solver's layout.  zero_fallback: a guess
// that is no better than zero is replaced by zero.
template <typename LoadX, typename LoadB, typename StoreX>
static void solve_guess_core(ddamg_hip_ctx* c, int system, double tol, LoadX load_x, LoadB load_b, StoreX store_x, bool zero_fallback, int* iterations,
                             int* coarse_iterations, double* relres, double* guess_relres) {
  require_system(system);
  DDAMG_REQUIRE(c->have_operator, "no operator set");
  DDAMG_REQUIRE(c->par.method <= 0 || c->par.method == 5 || c->setup_done, "setup has not been run");
  const size_t n = (size_t)24 * c->levels[0]->geom.V;
  const View all = whole(n);
  const bool g5 = system == DDAMG_HIP_SYSTEM_DDAGGER;
  if (!(tol > 0)) tol = c->par.tol;
  DeviceBuffer<double> x, r, t;
  for (DeviceBuffer<double>* p : {&x, &r, &t}) p->alloc(n);
  load_x(x);
  apply_system(c, system, t, x);
  load_b(r);
  auto [nb, nr] = residual_norms(c, r, r, t);
  if (zero_fallback && nb > 0 && !(nr < nb)) {
    vec_zero<double>(x, all, c->stream);
    load_b(r);
    nr = nb;
  }
  int it = 0, cit = 0;
  double rr = 0, gr = 0;
  c->last_history.clear();
  if (!(nb > 0)) {
    vec_zero<double>(x, all, c->stream);
  } else {
    gr = nr / nb;
    if (nr <= tol * nb) {
      rr = gr;
    } else {
      // the correction of D^dagger through the gamma5 signs of the D^dagger solves; nb / nr first: a zero guess gives tol * 1
      solve_core(c, tol * (nb / nr), load_dev(c, r, g5), store_dev(c, t, g5), &it, &cit, nullptr);
      vec_plus<double>(x, x, t, all, c->stream);
      apply_system(c, system, t, x);
      load_b(r);
      const auto [nb1, nr1] = residual_norms(c, r, r, t);
      rr = nr1 / nb1;
    }
  }
  store_x(x);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->last_iter = it; c->last_coarse_iter = cit; c->last_relres = rr;
  if (iterations) *iterations = it;
  if (coarse_iterations) *coarse_iterations = cit;
  if (relres) *relres = rr;
  if (guess_relres) *guess_relres = gr;
}

static void require_store(const ddamg_hip_ctx* c, const ddamg_hip_chrono* h) {
  DDAMG_REQUIRE(h, "null argument");
  DDAMG_REQUIRE(h->owner == c, "the store belongs to another context");
}
static void chrono_push(ddamg_hip_ctx* c, ddamg_hip_chrono* h, const double* x) {
  vec_copy<double>(h->V + (size_t)h->next * h->n, x, whole(h->n), c->stream);
  h->next = (h->next + 1) % h->depth;
  h->count = std::min(h->count + 1, h->depth);
}

// x0 = the combination of the stored vectors that minimises ||b - A x0|| (x0 and b in the solver's layout, apart): the images
// q = A v_j, newest first, orthonormalised by classical Gram-Schmidt applied twice, the same operations carried on the v_j; an image
// that the projection takes below 1e-12 of its norm (rounding noise is k 2^-53, the smallest ratio of a useful history about 1e-7) is
// dropped.  Then c = Q^H b, x0 = W c, r = b - Q c.  One read-back per column.
static void chrono_guess(ddamg_hip_ctx* c, ddamg_hip_chrono* h, int system, double* x0, const double* b, int* kept, double* predicted_relres) {
  DDAMG_REQUIRE(c->have_operator, "no operator set");
  const size_t n = h->n;
  const View all = whole(n);
  hipStream_t st = c->stream;
  ReduceWork& rw = blas_rw(c);
  double* norms = rw.d_result + 2 * CHRONO_MAX;     // behind the coefficients of vec_multi_dot
  auto read_norms = [&] { publish_to_host(norms, 2, rw, st); wait_published(rw, st); };
  if (h->count && !h->Q.get()) {
    h->Q.alloc((size_t)h->depth * n);
    h->W.alloc((size_t)h->depth * n);
    h->r.alloc(n);
  }
  int m = 0;
  for (int age = 0; age < h->count; age++) {
    double *q = h->Q + (size_t)m * n, *w = h->W + (size_t)m * n;
    apply_system(c, system, q, h->slot(age));
    vec_copy<double>(w, h->slot(age), all, st);
    vec_norm<double>(q, all, rw, norms, st);
    for (int pass = 0; pass < 2 && m > 0; pass++) {
      vec_multi_dot<double>(h->Q, n, m, q, all, rw, rw.d_result, st);
      chrono_project_pair(q, h->Q, w, h->W, n, m, rw.d_result, all, st);
    }
    vec_norm<double>(q, all, rw, norms + 1, st);
    read_norms();
    const double before = rw.h_result[0], after = rw.h_result[1];
    if (!(after > 1e-12 * before)) continue;        // a duplicate, a zero vector, or not a number
    vec_scale<double>(q, q, 1.0 / after, 0.0, all, st);
    vec_scale<double>(w, w, 1.0 / after, 0.0, all, st);
    m++;
  }
  double predicted = 1.0;
  if (m == 0) {
    vec_zero<double>(x0, all, st);
  } else {
    vec_multi_dot<double>(h->Q, n, m, b, all, rw, rw.d_result, st);
    chrono_combine(x0, h->W, h->r, b, h->Q, n, m, rw.d_result, all, st);
    vec_norm<double>(h->r, all, rw, norms, st);
    vec_norm<double>(b, all, rw, norms + 1, st);
    read_norms();
    predicted = rw.h_result[1] > 0 ? rw.h_result[0] / rw.h_result[1] : 0.0;
  }
  DDAMG_HIP_CHECK(hipStreamSynchronize(st));
  if (kept) *kept = m;
  if (predicted_relres) *predicted_relres = predicted;
}

// the guess from the store h (null: zero), the solve from it, the solution pushed
template <typename LoadB, typename StoreX>
static void solve_chrono_core(ddamg_hip_ctx* c, ddamg_hip_chrono* h, int system, double tol, LoadB load_b, StoreX store_x, int* iterations,
                              int* coarse_iterations, double* relres, double* guess_relres) {
  require_system(system);
  if (h) require_store(c, h);
  const size_t n = (size_t)24 * c->levels[0]->geom.V;
  solve_guess_core(c, system, tol, [&](double* x) {
    if (!h || h->count == 0) { vec_zero<double>(x, whole(n), c->stream); return; }
    DeviceBuffer<double> b;
    b.alloc(n);
    load_b(b);
    chrono_guess(c, h, system, x, b, nullptr, nullptr);
  }, load_b, [&](const double* x) {
    store_x(x);
    if (h) chrono_push(c, h, x);
  }, true, iterations, coarse_iterations, relres, guess_relres);
}

// D^dagger D x = b as solve_squared_core, each of the two solves from the guess of its own store
template <typename LoadB, typename StoreX>
static void solve_squared_chrono_core(ddamg_hip_ctx* c, ddamg_hip_chrono* hy, ddamg_hip_chrono* hx, double tol, LoadB load_b, StoreX store_x,
                                      int* iterations, int* coarse_iterations, double* relres) {
  const size_t n = (size_t)24 * c->levels[0]->geom.V;
  for (const ddamg_hip_chrono* h : {hy, hx})
    if (h) require_store(c, h);
  DeviceBuffer<double> y, t, u;
  for (DeviceBuffer<double>* p : {&y, &t, &u}) p->alloc(n);
  solve_chrono_core(c, hy, DDAMG_HIP_SYSTEM_DDAGGER, tol, load_b, store_dev(c, y), iterations, coarse_iterations, nullptr, nullptr);
  double rr = 0;
  solve_chrono_core(c, hx, DDAMG_HIP_SYSTEM_D, tol, load_dev(c, y), [&](const double* x) {
    rr = squared_residual(c, x, load_b, u, t);
    store_x(x);
  }, iterations ? iterations + 1 : nullptr, coarse_iterations ? coarse_iterations + 1 : nullptr, nullptr, nullptr);
  c->last_relres = rr;
  if (relres) *relres = rr;
}

// ---- the even-odd preconditioned system  Dhat = D_ee - D_eo D_oo^-1 D_oe  (eo_system.h) ----------------------------------------
// Ahat x_e = b_e, Ahat = Dhat or Dhat^dagger, through the identity [A^-1]_ee = Ahat^-1: the solve of the full system A E = (r, 0)
// by solve_core gives E_e = Ahat^-1 r.  The full solve stops on the residual of the full system, which bounds the residual of
// the Schur system only up to ||D_eo D_oo^-1||, so the loop measures the Schur residual itself with the fp64 operator and
// corrects: r = b_e - Ahat x_e; done where ||r|| <= tol ||b||; else A E = (r, 0) from zero to tol ||b|| / ||r||, x_e += E_e.
// At most MAX_SCHUR_SOLVES full solves: the cap makes the call terminate, relres says what was reached.
// load_x(dst) fills the guess and load_b(dst) the right-hand side, both with zeros on the odd sites; store_x(src) takes the
// full-lattice vector X with A X = (b_e, 0): x_e on the even sites, the odd part that belongs to it on the odd ones.  Everything
// in the solver's layout.
constexpr int MAX_SCHUR_SOLVES = 3;

static void require_schur_solve(ddamg_hip_ctx* c, const char* name) {
  require_even_extents(c, name);
  DDAMG_REQUIRE(c->have_operator, "no operator set");
  DDAMG_REQUIRE(c->par.method <= 0 || c->par.method == 5 || c->setup_done, "setup has not been run");
}

template <typename LoadX, typename LoadB, typename StoreX>
static void solve_schur_core(ddamg_hip_ctx* c, bool dagger, bool use_guess, double tol, LoadX load_x, LoadB load_b, StoreX store_x, int* iterations,
                             int* coarse_iterations, double* relres) {
  const int V = c->levels[0]->geom.V;
  const size_t n = (size_t)24 * V;
  const View all = whole(n);
  const unsigned char* parity = c->fop64.dev().parity;
  if (!(tol > 0)) tol = c->par.tol;
  DeviceBuffer<double> x, b, r, y;
  for (DeviceBuffer<double>* p : {&x, &b, &r, &y}) p->alloc(n);
  load_b(b);
  if (use_guess) load_x(x); else vec_zero<double>(x, all, c->stream);
  int it = 0, cit = 0;
  double rr = 0;
  c->last_history.clear();
  for (int solves = 0;; solves++) {
    // a zero start: r = b without an application (x is the zero vector); both norms from one reduction in either case
    const bool zero_start = solves == 0 && !use_guess;
    if (!zero_start) schur_apply<double>(c->fop64, y, x, dagger, c->eo, c->stream);
    const auto [nb, nr] = residual_norms(c, r, b, zero_start ? x.get() : y.get());
    if (!(nb > 0)) {
      vec_zero<double>(x, all, c->stream);
      rr = 0;
      break;
    }
    rr = nr / nb;
    if (nr <= tol * nb || solves == MAX_SCHUR_SOLVES) break;
    int it1 = 0, cit1 = 0;
    // the odd sites of r hold zeros: the right-hand side (r, 0).  The correction of Dhat^dagger through the gamma5 signs of the
    // D^dagger solves.
    solve_core(c, tol * (nb / nr), load_dev(c, r, dagger), [&](const double* E) {
      parity_update<double>(x, E, parity, 0, ParityOp::Add, dagger, V, c->stream);
    }, &it1, &cit1, nullptr);
    it += it1; cit += cit1;
  }
  // X_o = -D_oo^-1 D_oe x_e (Dhat^dagger: -gamma5 D_oo^-1 D_oe gamma5 x_e), from the x_e that is returned
  const double* t = schur_odd_part<double>(c->fop64, x, dagger, c->eo, c->stream);
  parity_update<double>(x, t, parity, 1, ParityOp::MinusAssign, dagger, V, c->stream);
  store_x(x);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->last_iter = it; c->last_coarse_iter = cit; c->last_relres = rr;
  if (iterations) *iterations = it;
  if (coarse_iterations) *coarse_iterations = cit;
  if (relres) *relres = rr;
}

// Dhat^dagger Dhat x_e = b_e: y_e = Dhat^-dagger b_e, then x_e = Dhat^-1 y_e; y stays on the device and lives for this call only.
// relres = ||b_e - Dhat^dagger Dhat x_e|| / ||b_e|| in fp64, of the system the caller asked for.
template <typename LoadB, typename StoreX>
static void solve_schur_squared_core(ddamg_hip_ctx* c, double tol, LoadB load_b, StoreX store_x, int* iterations, int* coarse_iterations, double* relres) {
  const int V = c->levels[0]->geom.V;
  const size_t n = (size_t)24 * V;
  const View all = whole(n);
  DeviceBuffer<double> y, t, u;
  for (DeviceBuffer<double>* p : {&y, &t, &u}) p->alloc(n);
  auto no_guess = [&](double* dst) { vec_zero<double>(dst, all, c->stream); };
  solve_schur_core(c, true, false, tol, no_guess, load_b, [&](const double* X) {
    c->fop64.parity_select(y, X, nullptr, 0, c->stream);      // y_e; the odd part of that solve is not wanted
  }, iterations, coarse_iterations, nullptr);
  double rr = 0;
  solve_schur_core(c, false, false, tol, no_guess, load_dev(c, y), [&](const double* X) {
    schur_apply<double>(c->fop64, t, X, false, c->eo, c->stream);
    schur_apply<double>(c->fop64, u, t, true, c->eo, c->stream);
    load_b(t);
    const auto [nb, nr] = residual_norms(c, t, t, u);
    rr = nb > 0 ? nr / nb : 0.0;
    store_x(X);
  }, iterations ? iterations + 1 : nullptr, coarse_iterations ? coarse_iterations + 1 : nullptr, nullptr);
  c->last_relres = rr;
  if (relres) *relres = rr;
}

// load / store callbacks of the Schur solves.  _vec: the even sites of a fine fp64 vector (its odd sites are not read); the
// store writes the whole vector.  _device: half fields, the odd one optional.
static auto load_even_vec(ddamg_hip_ctx* c, const double* v) {
  return [=](double* dst) { c->fop64.parity_select(dst, v, nullptr, 0, c->stream); };
}
static auto load_even_half(ddamg_hip_ctx* c, const double* half_dev) {
  return [=](double* dst) {
    vec_from_half<double>(dst, half_dev, c->levels[0]->d_lex_of_site.get(), c->fop64.dev().parity, 0, true, false, c->levels[0]->geom.V, c->stream);
  };
}
static auto store_halves(ddamg_hip_ctx* c, double* x_e_dev, double* x_o_dev) {
  return [=](const double* src) {
    const int* lex = c->levels[0]->d_lex_of_site.get();
    const unsigned char* par = c->fop64.dev().parity;
    vec_to_half<double>(x_e_dev, src, lex, par, 0, false, c->levels[0]->geom.V, c->stream);
    if (x_o_dev) vec_to_half<double>(x_o_dev, src, lex, par, 1, false, c->levels[0]->geom.V, c->stream);
  };
}
// the half fields of a Schur *_device solve: in the memory of the context's device, and apart; x_o_dev may be null
static void require_device_halves(ddamg_hip_ctx* c, double* x_e_dev, double* x_o_dev, const double* b_e_dev, const char* name) {
  const size_t nb = sizeof(double) * 12 * c->levels[0]->geom.V;
  ddamg_require_device_array(c, x_e_dev, nb, name);
  ddamg_require_device_array(c, b_e_dev, nb, name);
  ddamg_require_disjoint(x_e_dev, b_e_dev, nb, name);
  if (x_o_dev) {
    ddamg_require_device_array(c, x_o_dev, nb, name);
    ddamg_require_disjoint(x_o_dev, b_e_dev, nb, name);
    ddamg_require_disjoint(x_o_dev, x_e_dev, nb, name);
  }
}

// ---- multi-shift CG on A_s = Dhat^dagger Dhat + sigma_s (multishift.h) ---------------------------------------------------------
// load_b(dst) fills the right-hand side with zeros on the odd sites; want_odd(s) says whether shift s gets its odd part
// -D_oo^-1 D_oe x_s; store_x(s, X) takes the full-length vector of shift s (x_s on the even sites, the odd part or zeros on the odd
// ones), all in the solver's layout.  Per iteration two read-backs (<p, A p> and <r, r>) through publish_to_host, one upload of the
// coefficients, and on top of the four hopping launches of Dhat^dagger Dhat a dot product, the residual kernel and the update
// kernel.  Works on a process grid as it is: schur_apply exchanges the faces and every reduction goes through rw.comm.
static void require_multishift(const ddamg_hip_ctx* c, int nshift, const double* shifts, const char* name) {
  const std::string n(name);
  DDAMG_REQUIRE(shifts != nullptr, "null argument");
  DDAMG_REQUIRE(nshift >= 1 && nshift <= DDAMG_HIP_MAX_SHIFTS, (n + ": nshift must lie between 1 and DDAMG_HIP_MAX_SHIFTS (32)").c_str());
  for (int s = 0; s < nshift; s++)
    DDAMG_REQUIRE(std::isfinite(shifts[s]) && shifts[s] >= 0, (n + ": every shift must be finite and not negative").c_str());
  require_even_extents(c, name);
  DDAMG_REQUIRE(c->have_operator, (n + ": no operator set (call ddamg_hip_set_gauge / ddamg_hip_set_operator)").c_str());
  DDAMG_REQUIRE(!c->levels[0]->geom.distributed() || c->comm != nullptr, (n + " on a process grid is collective: install a transport first").c_str());
}

template <typename LoadB, typename WantOdd, typename StoreX>
static void solve_schur_multishift_core(ddamg_hip_ctx* c, int nshift, const double* shifts, const double* tols, int max_iterations, LoadB load_b,
                                        WantOdd want_odd, StoreX store_x, int* iterations, double* relres, double* ritz) {
  const int V = c->levels[0]->geom.V;
  const size_t n = (size_t)24 * V, half = (size_t)12 * V;
  const View all = whole(n);
  hipStream_t st = c->stream;
  const unsigned char* parity = c->fop64.dev().parity;
  multishift_prepare(c->ms, c->levels[0]->geom.parity, st);
  ReduceWork& rw = c->ms.rw;
  rw.comm = c->comm;
  const int* even = c->ms.even_site.get();
  const int maxit = max_iterations > 0 ? max_iterations : c->par.restart * c->par.max_restart;
  int base = 0;
  for (int s = 1; s < nshift; s++)
    if (shifts[s] < shifts[base]) base = s;
  const double sigma = shifts[base];
  std::vector<double> tol(nshift);
  for (int s = 0; s < nshift; s++) tol[s] = tols && tols[s] > 0 ? tols[s] : c->par.tol;

  DeviceBuffer<double> b, r, p, t, u, slab;
  for (DeviceBuffer<double>* v : {&b, &r, &p, &t, &u}) v->alloc(n);
  slab.alloc(2 * (size_t)nshift * half);
  double* xs = slab;
  double* ps = slab + (size_t)nshift * half;
  load_b(b);
  vec_dot_and_norm2<double>(b, b, all, rw, rw.d_result, st);
  publish_to_host(rw.d_result, 3, rw, st);
  wait_published(rw, st);
  const double bb = rw.h_result[2];
  std::vector<int> its(nshift, 0);
  std::vector<double> res(nshift, 0.0), al, be;
  double rz[2] = {0, 0};
  c->last_history.clear();
  DDAMG_HIP_CHECK(hipMemsetAsync(slab.get(), 0, slab.bytes(), st));
  if (bb > 0) {
    const double nb = std::sqrt(bb);
    vec_copy<double>(r, b, all, st);
    vec_copy<double>(p, b, all, st);
    for (int s = 0; s < nshift; s++)
      if (s != base) multishift_gather(ps + s * half, b, even, V, st);
    std::vector<double> zeta(nshift, 1.0), zeta_old(nshift, 1.0);
    std::vector<char> active(nshift, 1);
    int nactive = nshift, k = 0;
    for (int s = 0; s < nshift; s++)
      if (nb <= tol[s] * nb) { active[s] = 0; nactive--; }   // a tolerance of one or more: x_s = 0 meets it
    double alpha_old = 1.0, beta_old = 0.0, rr = bb;
    while (nactive > 0 && k < maxit) {
      schur_apply<double>(c->fop64, t, p, false, c->eo, st);
      schur_apply<double>(c->fop64, u, t, true, c->eo, st);
      vec_dot_and_norm2<double>(p, u, all, rw, rw.d_result, st);
      publish_to_host(rw.d_result, 3, rw, st);
      wait_published(rw, st);
      const double pAp = rw.h_result[0] + sigma * rw.h_result[2];
      if (!(pAp > 0) || !std::isfinite(pAp)) break;   // the direction has run out: what is reached is reported
      const double alpha = rr / pAp;
      multishift_residual(r, u, p, alpha, sigma, even, V, rw, rw.d_result, st);
      publish_to_host(rw.d_result, 1, rw, st);
      wait_published(rw, st);
      const double rr_new = rw.h_result[0];
      k++;
      const double beta = rr_new / rr, rnorm = std::sqrt(rr_new);
      // INVARIANT (h_coef, krylov.h): written only here, after the wait above, which the previous upload cannot outlive
      double* hc = rw.h_coef;
      int na = 0;
      hc[1] = beta; hc[2] = alpha; hc[3] = active[base] ? (double)base : -1.0;
      for (int s = 0; s < nshift; s++) {
        if (!active[s]) continue;
        const double ds = shifts[s] - sigma;
        const double zn = zeta[s] * zeta_old[s] * alpha_old / (alpha * beta_old * (zeta_old[s] - zeta[s]) + zeta_old[s] * alpha_old * (1.0 + ds * alpha));
        bool done = false;
        if (std::fpclassify(zn) != FP_NORMAL) {
          done = true;   // its residual zeta_s r has left the number format: frozen as it is, without this step
        } else {
          const double ratio = zn / zeta[s];
          if (s != base) {
            double* e = hc + MS_COEF_HEAD + MS_COEF_PER * na++;
            e[0] = (double)s; e[1] = alpha * ratio; e[2] = beta * ratio * ratio; e[3] = zn;
          }
          zeta_old[s] = zeta[s]; zeta[s] = zn;
          done = std::fabs(zn) * rnorm <= tol[s] * nb;
        }
        its[s] = k;
        if (done) { active[s] = 0; nactive--; }
      }
      hc[0] = (double)na;
      upload_coefficients(rw, MS_COEF_HEAD + MS_COEF_PER * na, st);
      multishift_update(p, r, xs, ps, rw.d_coef, even, V, st);
      al.push_back(alpha); be.push_back(beta);
      alpha_old = alpha; beta_old = beta; rr = rr_new;
      c->last_history.push_back(rnorm / nb);
    }
    lanczos_extremes(al, be, rz);
    if (!al.empty()) { rz[0] -= sigma; rz[1] -= sigma; }
  }
  // per shift: the residual of the x_s that is returned with the fp64 operator, its odd part, the store.  X and w reuse r and p.
  double* X = r;
  double* w = p;
  int total = 0;
  double worst = 0;
  for (int s = 0; s < nshift; s++) {
    vec_zero<double>(X, all, st);
    if (bb > 0) {
      multishift_scatter(X, xs + s * half, even, V, st);
      schur_apply<double>(c->fop64, t, X, false, c->eo, st);
      schur_apply<double>(c->fop64, u, t, true, c->eo, st);
      vec_axpy<double>(w, u, X, shifts[s], 0.0, all, st);
      const auto [nb, nr] = residual_norms(c, t, b, w);
      res[s] = nb > 0 ? nr / nb : 0.0;
      if (want_odd(s)) {
        const double* o = schur_odd_part<double>(c->fop64, X, false, c->eo, st);
        parity_update<double>(X, o, parity, 1, ParityOp::MinusAssign, false, V, st);
      }
    }
    store_x(s, X);
    total = std::max(total, its[s]);
    worst = std::max(worst, res[s]);
  }
  DDAMG_HIP_CHECK(hipStreamSynchronize(st));
  c->last_iter = total; c->last_coarse_iter = 0; c->last_relres = worst;
  for (int s = 0; s < nshift; s++) {
    if (iterations) iterations[s] = its[s];
    if (relres) relres[s] = res[s];
  }
  if (ritz) { ritz[0] = rz[0]; ritz[1] = rz[1]; }
}

extern "C" {

int ddamg_hip_solve_schur_vec(ddamg_hip_ctx* c, int dagger, int use_guess, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol, int* iterations,
                              int* coarse_iterations, double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_solve_vecs(x, b, "solve_schur_vec needs fine-level fp64 vectors");
  DDAMG_REQUIRE(x != b, "solve_schur_vec: the solution and the right-hand side must be two vectors");
  require_schur_solve(c, "ddamg_hip_solve_schur_vec");
  solve_schur_core(c, dagger != 0, use_guess != 0, tol, load_even_vec(c, vec_data<double>(x)), load_even_vec(c, vec_data<double>(b)),
                   store_dev(c, vec_data<double>(x)), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

int ddamg_hip_solve_schur_device(ddamg_hip_ctx* c, int dagger, int use_guess, double* x_e_dev, double* x_o_dev, const double* b_e_dev, double tol,
                                 int* iterations, int* coarse_iterations, double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_device_halves(c, x_e_dev, x_o_dev, b_e_dev, "ddamg_hip_solve_schur_device");
  require_schur_solve(c, "ddamg_hip_solve_schur_device");
  solve_schur_core(c, dagger != 0, use_guess != 0, tol, load_even_half(c, x_e_dev), load_even_half(c, b_e_dev), store_halves(c, x_e_dev, x_o_dev),
                   iterations, coarse_iterations, relres);
  DDAMG_API_END
}

int ddamg_hip_solve_schur_squared_vec(ddamg_hip_ctx* c, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol, int iterations[2], int coarse_iterations[2],
                                      double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_solve_vecs(x, b, "solve_schur_squared_vec needs fine-level fp64 vectors");
  DDAMG_REQUIRE(x != b, "solve_schur_squared_vec: the solution and the right-hand side must be two vectors");
  require_schur_solve(c, "ddamg_hip_solve_schur_squared_vec");
  solve_schur_squared_core(c, tol, load_even_vec(c, vec_data<double>(b)), store_dev(c, vec_data<double>(x)), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

int ddamg_hip_solve_schur_squared_device(ddamg_hip_ctx* c, double* x_e_dev, double* x_o_dev, const double* b_e_dev, double tol, int iterations[2],
                                         int coarse_iterations[2], double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_device_halves(c, x_e_dev, x_o_dev, b_e_dev, "ddamg_hip_solve_schur_squared_device");
  require_schur_solve(c, "ddamg_hip_solve_schur_squared_device");
  solve_schur_squared_core(c, tol, load_even_half(c, b_e_dev), store_halves(c, x_e_dev, x_o_dev), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

int ddamg_hip_solve_schur_multishift_device(ddamg_hip_ctx* c, int nshift, const double* shifts, const double* tols, double* const* x_e_dev,
                                            double* const* x_o_dev, const double* b_e_dev, int max_iterations, int* iterations, double* relres,
                                            double ritz[2]) {
  DDAMG_API_BEGIN
  enter(c);
  const char* name = "ddamg_hip_solve_schur_multishift_device";
  DDAMG_REQUIRE(x_e_dev != nullptr, "null argument");
  require_multishift(c, nshift, shifts, name);
  const size_t nb = sizeof(double) * 12 * c->levels[0]->geom.V;
  ddamg_require_device_array(c, b_e_dev, nb, name);
  std::vector<double*> outs;
  for (int s = 0; s < nshift; s++) {
    outs.push_back(x_e_dev[s]);
    if (x_o_dev && x_o_dev[s]) outs.push_back(x_o_dev[s]);
  }
  for (size_t i = 0; i < outs.size(); i++) {
    ddamg_require_device_array(c, outs[i], nb, name);
    ddamg_require_disjoint(outs[i], b_e_dev, nb, name);
    for (size_t j = 0; j < i; j++)
      DDAMG_REQUIRE(outs[i] + nb / sizeof(double) <= outs[j] || outs[j] + nb / sizeof(double) <= outs[i], (std::string(name) + ": two output arrays overlap").c_str());
  }
  const int* lex = c->levels[0]->d_lex_of_site.get();
  const unsigned char* par = c->fop64.dev().parity;
  const int V = c->levels[0]->geom.V;
  solve_schur_multishift_core(c, nshift, shifts, tols, max_iterations, load_even_half(c, b_e_dev),
                              [&](int s) { return x_o_dev && x_o_dev[s]; },
                              [&](int s, const double* X) {
                                vec_to_half<double>(x_e_dev[s], X, lex, par, 0, false, V, c->stream);
                                if (x_o_dev && x_o_dev[s]) vec_to_half<double>(x_o_dev[s], X, lex, par, 1, false, V, c->stream);
                              }, iterations, relres, ritz);
  DDAMG_API_END
}

int ddamg_hip_solve_schur_multishift_vec(ddamg_hip_ctx* c, int nshift, const double* shifts, const double* tols, ddamg_hip_vec* const* x,
                                         const ddamg_hip_vec* b, int max_iterations, int* iterations, double* relres, double ritz[2]) {
  DDAMG_API_BEGIN
  enter(c);
  const char* name = "ddamg_hip_solve_schur_multishift_vec";
  DDAMG_REQUIRE(x != nullptr && b != nullptr, "null argument");
  require_multishift(c, nshift, shifts, name);
  for (int s = 0; s < nshift; s++) {
    require_solve_vecs(x[s], b, "solve_schur_multishift_vec needs fine-level fp64 vectors");
    DDAMG_REQUIRE(x[s] != b, "solve_schur_multishift_vec: a solution and the right-hand side must be two vectors");
    for (int t = 0; t < s; t++) DDAMG_REQUIRE(x[s] != x[t], "solve_schur_multishift_vec: the solutions must be distinct vectors");
  }
  solve_schur_multishift_core(c, nshift, shifts, tols, max_iterations, load_even_vec(c, vec_data<double>(b)), [](int) { return true; },
                              [&](int s, const double* X) { vec_copy<double>(vec_data<double>(x[s]), X, whole((size_t)24 * c->levels[0]->geom.V), c->stream); },
                              iterations, relres, ritz);
  DDAMG_API_END
}

int ddamg_hip_solve_guess(ddamg_hip_ctx* c, int system, double* x_lex, const double* b_lex, double tol, int* iterations, int* coarse_iterations,
                          double* relres, double* guess_relres) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(x_lex && b_lex, "null argument");
  double* st = c->stage(sizeof(double) * 24 * c->levels[0]->geom.V);
  solve_guess_core(c, system, tol, load_lex(c, x_lex, st), load_lex(c, b_lex, st), store_lex(c, x_lex, st), false, iterations, coarse_iterations, relres,
                   guess_relres);
  DDAMG_API_END
}

int ddamg_hip_solve_guess_device(ddamg_hip_ctx* c, int system, double* x_dev_lex, const double* b_dev_lex, double tol, int* iterations,
                                 int* coarse_iterations, double* relres, double* guess_relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_device_pair(c, x_dev_lex, b_dev_lex, "ddamg_hip_solve_guess_device");
  solve_guess_core(c, system, tol, load_lex(c, x_dev_lex), load_lex(c, b_dev_lex), store_lex(c, x_dev_lex), false, iterations, coarse_iterations, relres,
                   guess_relres);
  DDAMG_API_END
}

int ddamg_hip_solve_guess_vec(ddamg_hip_ctx* c, int system, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol, int* iterations,
                              int* coarse_iterations, double* relres, double* guess_relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_solve_vecs(x, b, "solve_guess_vec needs fine-level fp64 vectors");
  DDAMG_REQUIRE(x != b, "solve_guess_vec: the guess and the right-hand side must be two vectors");
  solve_guess_core(c, system, tol, load_dev(c, vec_data<double>(x)), load_dev(c, vec_data<double>(b)), store_dev(c, vec_data<double>(x)), false,
                   iterations, coarse_iterations, relres, guess_relres);
  DDAMG_API_END
}

int ddamg_hip_chrono_create(ddamg_hip_ctx* c, int depth, ddamg_hip_chrono** h) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(h, "null argument");
  DDAMG_REQUIRE(depth >= 1 && depth <= CHRONO_MAX, "chrono_create: 1 <= depth <= 8");
  std::unique_ptr<ddamg_hip_chrono> s(new ddamg_hip_chrono);
  s->owner = c; s->depth = depth;
  s->n = (size_t)24 * c->levels[0]->geom.V;
  s->V.alloc((size_t)depth * s->n);
  *h = s.release();
  DDAMG_API_END
}

int ddamg_hip_chrono_destroy(ddamg_hip_ctx* c, ddamg_hip_chrono* h) {
  DDAMG_API_BEGIN
  enter(c);
  if (!h) return 0;
  require_store(c, h);
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  delete h;
  DDAMG_API_END
}

int ddamg_hip_chrono_reset(ddamg_hip_ctx* c, ddamg_hip_chrono* h) {
  DDAMG_API_BEGIN
  enter(c);
  require_store(c, h);
  h->count = h->next = 0;
  DDAMG_API_END
}

int ddamg_hip_chrono_count(ddamg_hip_ctx* c, ddamg_hip_chrono* h, int* n) {
  DDAMG_API_BEGIN
  enter(c);
  require_store(c, h);
  DDAMG_REQUIRE(n, "null argument");
  *n = h->count;
  DDAMG_API_END
}

int ddamg_hip_chrono_push_vec(ddamg_hip_ctx* c, ddamg_hip_chrono* h, const ddamg_hip_vec* x) {
  DDAMG_API_BEGIN
  enter(c);
  require_store(c, h);
  DDAMG_REQUIRE(x, "null argument");
  DDAMG_REQUIRE(x->level == 0 && x->precision == 64, "chrono_push_vec needs a fine-level fp64 vector");
  chrono_push(c, h, vec_data<double>(x));
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  DDAMG_API_END
}

int ddamg_hip_chrono_guess_vec(ddamg_hip_ctx* c, ddamg_hip_chrono* h, int system, ddamg_hip_vec* x0, const ddamg_hip_vec* b, int* kept,
                               double* predicted_relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_store(c, h);
  require_system(system);
  require_solve_vecs(x0, b, "chrono_guess_vec needs fine-level fp64 vectors");
  DDAMG_REQUIRE(x0 != b, "chrono_guess_vec: the guess and the right-hand side must be two vectors");
  chrono_guess(c, h, system, vec_data<double>(x0), vec_data<double>(b), kept, predicted_relres);
  DDAMG_API_END
}

int ddamg_hip_solve_chrono_vec(ddamg_hip_ctx* c, ddamg_hip_chrono* h, int system, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol, int* iterations,
                               int* coarse_iterations, double* relres, double* guess_relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_store(c, h);
  require_solve_vecs(x, b, "solve_chrono_vec needs fine-level fp64 vectors");
  DDAMG_REQUIRE(x != b, "solve_chrono_vec: the solution and the right-hand side must be two vectors");
  solve_chrono_core(c, h, system, tol, load_dev(c, vec_data<double>(b)), store_dev(c, vec_data<double>(x)), iterations, coarse_iterations, relres,
                    guess_relres);
  DDAMG_API_END
}

int ddamg_hip_solve_chrono_device(ddamg_hip_ctx* c, ddamg_hip_chrono* h, int system, double* x_dev_lex, const double* b_dev_lex, double tol,
                                  int* iterations, int* coarse_iterations, double* relres, double* guess_relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_store(c, h);
  require_device_pair(c, x_dev_lex, b_dev_lex, "ddamg_hip_solve_chrono_device");
  solve_chrono_core(c, h, system, tol, load_lex(c, b_dev_lex), store_lex(c, x_dev_lex), iterations, coarse_iterations, relres, guess_relres);
  DDAMG_API_END
}

int ddamg_hip_solve_squared_chrono_vec(ddamg_hip_ctx* c, ddamg_hip_chrono* hy, ddamg_hip_chrono* hx, ddamg_hip_vec* x, const ddamg_hip_vec* b,
                                       double tol, int iterations[2], int coarse_iterations[2], double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_solve_vecs(x, b, "solve_squared_chrono_vec needs fine-level fp64 vectors");
  DDAMG_REQUIRE(x != b, "solve_squared_chrono_vec: the solution and the right-hand side must be two vectors");
  solve_squared_chrono_core(c, hy, hx, tol, load_dev(c, vec_data<double>(b)), store_dev(c, vec_data<double>(x)), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

int ddamg_hip_solve_squared_chrono_device(ddamg_hip_ctx* c, ddamg_hip_chrono* hy, ddamg_hip_chrono* hx, double* x_dev_lex, const double* b_dev_lex,
                                          double tol, int iterations[2], int coarse_iterations[2], double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_device_pair(c, x_dev_lex, b_dev_lex, "ddamg_hip_solve_squared_chrono_device");
  solve_squared_chrono_core(c, hy, hx, tol, load_lex(c, b_dev_lex), store_lex(c, x_dev_lex), iterations, coarse_iterations, relres);
  DDAMG_API_END
}


int ddamg_hip_solve(ddamg_hip_ctx* c, double* x_lex, const double* b_lex, double tol, int* iterations, int* coarse_iterations, double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(x_lex && b_lex, "null argument");
  double* st = c->stage(sizeof(double) * 24 * c->levels[0]->geom.V);
  solve_core(c, tol, load_lex(c, b_lex, st), store_lex(c, x_lex, st), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

int ddamg_hip_solve_device(ddamg_hip_ctx* c, double* x_dev_lex, const double* b_dev_lex, double tol, int* iterations, int* coarse_iterations, double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_device_pair(c, x_dev_lex, b_dev_lex, "ddamg_hip_solve_device");
  solve_core(c, tol, load_lex(c, b_dev_lex), store_lex(c, x_dev_lex), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

int ddamg_hip_solve_vec(ddamg_hip_ctx* c, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol, int* iterations, int* coarse_iterations, double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_solve_vecs(x, b, "solve_vec needs fine-level fp64 vectors");
  solve_core(c, tol, load_dev(c, vec_data<double>(b)), store_dev(c, vec_data<double>(x)), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

// ---- D^dagger x = b: x = gamma5 D^-1 gamma5 b, the signs in the load and store callbacks (no pass of their own) ----
int ddamg_hip_solve_dagger(ddamg_hip_ctx* c, double* x_lex, const double* b_lex, double tol, int* iterations, int* coarse_iterations, double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(x_lex && b_lex, "null argument");
  double* st = c->stage(sizeof(double) * 24 * c->levels[0]->geom.V);
  solve_core(c, tol, load_lex(c, b_lex, st, true), store_lex(c, x_lex, st, true), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

int ddamg_hip_solve_dagger_device(ddamg_hip_ctx* c, double* x_dev_lex, const double* b_dev_lex, double tol, int* iterations, int* coarse_iterations, double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_device_pair(c, x_dev_lex, b_dev_lex, "ddamg_hip_solve_dagger_device");
  solve_core(c, tol, load_lex(c, b_dev_lex, nullptr, true), store_lex(c, x_dev_lex, nullptr, true), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

int ddamg_hip_solve_dagger_vec(ddamg_hip_ctx* c, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol, int* iterations, int* coarse_iterations, double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_solve_vecs(x, b, "solve_dagger_vec needs fine-level fp64 vectors");
  solve_core(c, tol, load_dev(c, vec_data<double>(b), true), store_dev(c, vec_data<double>(x), true), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

// ---- D^dagger D x = b (solve_squared_core) ----
int ddamg_hip_solve_squared(ddamg_hip_ctx* c, double* x_lex, const double* b_lex, double tol, int iterations[2], int coarse_iterations[2], double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(x_lex && b_lex, "null argument");
  double* st = c->stage(sizeof(double) * 24 * c->levels[0]->geom.V);
  solve_squared_core(c, tol, load_lex(c, b_lex, st, true), load_lex(c, b_lex, st), store_lex(c, x_lex, st), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

int ddamg_hip_solve_squared_device(ddamg_hip_ctx* c, double* x_dev_lex, const double* b_dev_lex, double tol, int iterations[2], int coarse_iterations[2],
                                   double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_device_pair(c, x_dev_lex, b_dev_lex, "ddamg_hip_solve_squared_device");
  solve_squared_core(c, tol, load_lex(c, b_dev_lex, nullptr, true), load_lex(c, b_dev_lex), store_lex(c, x_dev_lex), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

int ddamg_hip_solve_squared_vec(ddamg_hip_ctx* c, ddamg_hip_vec* x, const ddamg_hip_vec* b, double tol, int iterations[2], int coarse_iterations[2],
                                double* relres) {
  DDAMG_API_BEGIN
  enter(c);
  require_solve_vecs(x, b, "solve_squared_vec needs fine-level fp64 vectors");
  const double* bd = vec_data<double>(b);
  solve_squared_core(c, tol, load_dev(c, bd, true), load_dev(c, bd), store_dev(c, vec_data<double>(x)), iterations, coarse_iterations, relres);
  DDAMG_API_END
}

// ---- BLAS-1 on device vectors (src/linalg_generic.c:29-353) ---------------------------------------
static void same_shape(const ddamg_hip_vec* a, const ddamg_hip_vec* b) {
  DDAMG_REQUIRE(a && b && a->level == b->level && a->precision == b->precision, "vectors differ in level or precision");
}

int ddamg_hip_vec_copy(ddamg_hip_ctx* c, ddamg_hip_vec* dst, const ddamg_hip_vec* src) {
  DDAMG_API_BEGIN
  enter(c);
  same_shape(dst, src);
  with_vec(dst, [&](auto* d) { using T = pointee<decltype(d)>; vec_copy<T>(d, vec_data<T>(src), whole(vec_len(dst)), c->stream); });
  DDAMG_API_END
}
int ddamg_hip_vec_axpy(ddamg_hip_ctx* c, ddamg_hip_vec* z, const ddamg_hip_vec* x, const ddamg_hip_vec* y, double alpha_re, double alpha_im) {
  DDAMG_API_BEGIN
  enter(c);
  same_shape(z, x); same_shape(z, y);
  with_vec(z, [&](auto* d) { using T = pointee<decltype(d)>; vec_axpy<T>(d, vec_data<T>(x), vec_data<T>(y), alpha_re, alpha_im, whole(vec_len(z)), c->stream); });
  DDAMG_API_END
}
int ddamg_hip_vec_dot(ddamg_hip_ctx* c, const ddamg_hip_vec* x, const ddamg_hip_vec* y, double* re, double* im, double* norm_x) {
  DDAMG_API_BEGIN
  enter(c);
  same_shape(x, y);
  ReduceWork& rw = blas_rw(c);
  with_vec(x, [&](auto* p) { using T = pointee<decltype(p)>; vec_dot_and_norm2<T>(p, vec_data<T>(y), whole(vec_len(x)), rw, rw.d_result, c->stream); });
  DDAMG_HIP_CHECK(hipMemcpyAsync(rw.h_result, rw.d_result, sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
  DDAMG_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (re) *re = rw.h_result[0];
  if (im) *im = rw.h_result[1];
  if (norm_x) *norm_x = sqrt(rw.h_result[2]);
  DDAMG_API_END
}

int ddamg_hip_preconditioner(ddamg_hip_ctx* c, double* out_lex, const double* in_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(out_lex && in_lex, "null argument");
  DDAMG_REQUIRE(c->setup_done && c->par.method > 0, "setup has not been run");
  double* st = c->stage(sizeof(double) * 24 * c->levels[0]->geom.V);
  precondition_core(c, load_lex(c, in_lex, st), store_lex(c, out_lex, st));
  DDAMG_API_END
}

int ddamg_hip_preconditioner_device(ddamg_hip_ctx* c, double* out_dev_lex, const double* in_dev_lex) {
  DDAMG_API_BEGIN
  enter(c);
  DDAMG_REQUIRE(c->setup_done && c->par.method > 0, "setup has not been run");
  require_device_pair(c, out_dev_lex, in_dev_lex, "ddamg_hip_preconditioner_device");
  precondition_core(c, load_lex(c, in_dev_lex), store_lex(c, out_dev_lex));
  DDAMG_API_END
}

int ddamg_hip_residual_history(ddamg_hip_ctx* c, double* history, int max_len, int* len) {
  DDAMG_API_BEGIN
  DDAMG_REQUIRE(c, "null context");   // host numbers only: no device is selected
  DDAMG_REQUIRE(len && (history || max_len <= 0), "null argument");
  const int n = (int)c->last_history.size();
  *len = n;
  for (int i = 0; i < n && i < max_len; i++) history[i] = c->last_history[i];
  DDAMG_API_END
}

}  // extern "C"
