// mg.cpp -- see mg.h
#include "mg.h"
#include "coarse_batch.h"
#include <cstdio>
#include <chrono>
#include <cstdlib>
#include "setup_kernels.h"
#include <cmath>
#include <cstdlib>
#include <vector>
#include <algorithm>

namespace ddamg {

template <typename T>
Multigrid<T>::Multigrid(const ddamg_hip_params& par, const Knobs& knobs, const std::vector<const Geometry*>& geoms, const FineOp<T>* fop, hipStream_t st)
    : par_(par), knobs_(knobs), st_(st) {
  const int L = par.num_levels;
  DDAMG_REQUIRE(L >= 2 && L <= DDAMG_HIP_MAX_LEVELS && (int)geoms.size() == L, "multigrid needs 2..4 levels");
  size_t max_coarse = 0;
  for (int d = 0; d < L; d++) {
    std::unique_ptr<MGLevel<T>> lv(new MGLevel<T>);
    lv->depth = d; lv->g = geoms[d];
    lv->n = d == 0 ? 12 : 2 * par.num_vect[d - 1];
    lv->coarsest = d == L - 1;
    lv->nvec = lv->coarsest ? 0 : par.num_vect[d];
    lv->nel = (size_t)lv->g->V * lv->n * 2;
    if (d > 0) max_coarse = std::max(max_coarse, lv->nel);
    lv_.push_back(std::move(lv));
  }
  for (int d = 0; d < L; d++) {
    MGLevel<T>& lv = *lv_[d];
    const Geometry& g = *lv.g;
    for (int i = 0; i < 4; i++) { lv.buf[i].alloc(lv.nel); DDAMG_HIP_CHECK(device_zero(lv.buf[i], sizeof(T) * lv.nel)); }
    if (d == 0) lv.fop = fop;
    else lv.cop.alloc(g, lv.n, knobs_);
    if (!lv.coarsest) {
      if (par.method == 4) {
        // smoother = GMRES on the odd-even Schur complement of this level (schwarz_PRECISION_alloc, src/schwarz_generic.c:78-83:
        // restart length block_iter, tolerance EPS_PRECISION, no preconditioner; the V-cycle sets the number of restarts)
        for (int i = 0; i < 3; i++) { lv.sbuf[i].alloc(lv.nel); DDAMG_HIP_CHECK(device_zero(lv.sbuf[i], sizeof(T) * lv.nel)); }
        lv.srw.init(par.block_iter[d] + 8);
        lv.sgm.single_allreduce = knobs_.single_allreduce_arnoldi;
        lv.sgm.alloc(lv.nel, par.block_iter[d], false);
        lv.sgm.tol = sizeof(T) == 4 ? 1e-6 : 1e-14;
        // fine level: the Krylov vectors live on the even sites, which the site order keeps as the first half of every
        // Schwarz block -- a strided view (one row per 16-byte chunk row and block), so that no BLAS-1 pass touches the odd half
        lv.sgm.view = (par.odd_even && d == 0 && g.block_even_sites * 2 == g.block_sites)
                          ? View{(24 / Chunk<T>::CH) * g.num_blocks, (size_t)g.block_sites * Chunk<T>::CH, 0, (size_t)g.block_even_sites * Chunk<T>::CH}
                          : whole(lv.nel);
        lv.sgm.st = st_; lv.sgm.rw = &lv.srw;
        if (par.odd_even) lv.sgm.op = [this, d](T* out, const T* in) { this->smoother_schur(d, out, in); };
        else lv.sgm.op = [this, d](T* out, const T* in) { this->apply_op(d, out, in); };   // GMRES on the operator itself (src/schwarz_generic.c:81-82)
        if (d > 0 && par.odd_even) {
          std::vector<int> ps[2];
          for (int s = 0; s < g.V; s++) ps[g.parity[s]].push_back(s);
          for (int q = 0; q < 2; q++) {
            lv.n_parity_sites[q] = (int)ps[q].size();
            lv.d_parity_sites[q].upload(ps[q]);
          }
        }
      }
      if (d == 0) { if (par.method != 4) lv.fsap.setup(g, fop, par.block_iter[0], par.method, knobs_, st_, par.odd_even != 0); lv.fip.alloc(g, *geoms[1], lv.nvec, knobs_); }
      else { if (par.method != 4) lv.csap.setup(g, &lv.cop, par.block_iter[d], par.method, st_); lv.cip.alloc(g, *geoms[d + 1], lv.n, lv.nvec, knobs_); }
      lv.d_agg_face.alloc(g.V);
      DDAMG_HIP_CHECK(hipMemcpy(lv.d_agg_face, g.agg_face.data(), g.V, hipMemcpyHostToDevice));
      if (d == 0) {
        // the forward faces of an aggregate in compact form (AggFaces, transfer.h) -- where every aggregate has the same shape
        // and site order (it has, with the aggregate -> block -> parity ordering, unless blocks of odd extent alternate)
        std::vector<unsigned short> tab;
        AggFaces& af = lv.agg_faces;
        if (agg_face_tables(g, af, tab)) {
          lv.d_agg_tables.upload(tab);
          af.rank = lv.d_agg_tables;
          af.list = lv.d_agg_tables + (size_t)4 * af.agg_sites;
        }
      }
      for (int mu = 0; mu < 4; mu++) {
        std::vector<unsigned char> m(g.V);
        for (int s = 0; s < g.V; s++) m[s] = g.agg_face[s] & (unsigned char)(1u << mu);
        lv.d_dir_mask[mu].upload(m);
      }
    }
    if (d > 0 && !lv.coarsest) {
      // K-cycle FGMRES of this level (src/init_generic.c:155-160): restart kcycle_restart, kcycle_max_restart cycles
      lv.rw.init(std::max(par.kcycle_restart, PANEL_COLUMNS * lv.nvec) + 8);    // the Gram-Schmidt panels project on up to nvec vectors
      lv.gm.single_allreduce = knobs_.single_allreduce_arnoldi;
      lv.gm.alloc(lv.nel, par.kcycle_restart, true);
      lv.gm.num_restart = par.kcycle_max_restart;
      lv.gm.tol = par.kcycle_tol;
      lv.gm.view = whole(lv.nel);
      lv.gm.st = st_; lv.gm.rw = &lv.rw;
      lv.gm.op = [this, d](T* out, const T* in) { this->apply_op(d, out, in); };
      lv.gm.prec = [this, d](T* phi, T* Dphi, const T* eta, int res) { this->vcycle(d, phi, par_.method <= 2 ? Dphi : nullptr, eta, res); };
      lv.gm.prec_gives_Dphi = par.mixed_precision == 2 && par.method <= 2;   // src/linsolve_generic.c:757,828-835
      // the reference's vector loops visit this level aggregate -> block -> lexicographic inside the block
      // (src/gathering_generic.c:126-157); ours orders block sites by parity first
      lv.ref_order.reserve(g.V);
      int bpa[4], a[4], b[4], r[4], c[4];
      for (int mu = 0; mu < 4; mu++) bpa[mu] = g.A[mu] / g.B[mu];
      for (a[0] = 0; a[0] < g.nagg[0]; a[0]++) for (a[1] = 0; a[1] < g.nagg[1]; a[1]++)
      for (a[2] = 0; a[2] < g.nagg[2]; a[2]++) for (a[3] = 0; a[3] < g.nagg[3]; a[3]++)
        for (b[0] = 0; b[0] < bpa[0]; b[0]++) for (b[1] = 0; b[1] < bpa[1]; b[1]++)
        for (b[2] = 0; b[2] < bpa[2]; b[2]++) for (b[3] = 0; b[3] < bpa[3]; b[3]++)
          for (r[0] = 0; r[0] < g.B[0]; r[0]++) for (r[1] = 0; r[1] < g.B[1]; r[1]++)
          for (r[2] = 0; r[2] < g.B[2]; r[2]++) for (r[3] = 0; r[3] < g.B[3]; r[3]++) {
            for (int mu = 0; mu < 4; mu++) c[mu] = (a[mu] * bpa[mu] + b[mu]) * g.B[mu] + r[mu];
            lv.ref_order.push_back(g.site_of_lex[g.lex(c)]);
          }
    } else if (d == 0) {
      lv.rw.init(PANEL_COLUMNS * lv.nvec + 8);
    }
    if (lv.coarsest) {
      // coarsest-level GMRES on the even-site Schur complement (src/init_generic.c:148-154)
      lv.rw.init(std::max(par.coarse_iter, 8) + 4);
      lv.gm.pipelined = knobs_.pipelined_arnoldi;
      lv.gm.single_allreduce = knobs_.single_allreduce_arnoldi;
      lv.gm.alloc(lv.nel, par.coarse_iter, lv.gm.pipelined);
      lv.gm.num_restart = par.coarse_restart;
      lv.gm.tol = par.coarse_tol;
      lv.gm.st = st_; lv.gm.rw = &lv.rw;
      if (!par.odd_even) {
        // GMRES on the whole coarsest operator (fgmres_PRECISION on apply_coarse_operator, src/init_generic.c:148-154)
        lv.gm.view = whole(lv.nel);
        lv.gm.op = [this, d](T* out, const T* in) { this->apply_op(d, out, in); };
        continue;
      }
      // odd-even preconditioning needs a bipartite lattice: even global extents (the reference's check, src/init.c:1012)
      for (int mu = 0; mu < 4; mu++)
        DDAMG_REQUIRE((g.L[mu] * g.P[mu]) % 2 == 0, "the coarsest lattice must have even global extents (odd-even preconditioning)");
      int n_even = 0;
      for (int s = 0; s < g.V; s++) if (g.parity[s] == 0) n_even++;
      DDAMG_REQUIRE(n_even * 2 == g.V, "coarsest lattice needs as many even as odd sites");
      for (int s = 0; s < n_even; s++) DDAMG_REQUIRE(g.parity[s] == 0, "coarsest level must be parity ordered");
      lv.gm.view = View{1, 0, 0, (size_t)n_even * lv.n * 2};
      lv.gm.op = [this](T* out, const T* in) { this->schur(out, in); };
    }
  }
  const Geometry& g0 = *geoms[0];
  std::vector<int> id(g0.V);
  for (int i = 0; i < g0.V; i++) id[i] = i;
  d_identity0_.upload(id);
  d_lex0_.alloc(g0.V);
  DDAMG_HIP_CHECK(hipMemcpy(d_lex0_, g0.lex_of_site.data(), sizeof(int) * g0.V, hipMemcpyHostToDevice));
  d_stage_.alloc(std::max(lv_[0]->nel, max_coarse));
  // (W_, the five full fields of the column-by-column Galerkin construction, is allocated when that path first runs: 8 GB at
  // 64^4 that the batched construction never touches)
  cwork_.alloc(max_coarse * 5);
  if (par.gather_coarsest && lv_.back()->g->distributed()) setup_gathered_coarsest();
}

// rows of `row` reals: dst[i] = src[perm[i]]
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_kernel(T* __restrict__ dst, const T* __restrict__ src, const int* __restrict__ perm, size_t row, size_t total) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t r = i / row;
    dst[i] = src[(size_t)perm[r] * row + (i - r * row)];
  }
}
template <typename T>
static void gather_rows(T* dst, const T* src, const int* perm, int nrows, size_t row, hipStream_t st) {
  const size_t total = (size_t)nrows * row;
  hipLaunchKernelGGL(gather_rows_kernel<T>, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, st, dst, src, perm, row, total);
  DDAMG_HIP_CHECK(hipGetLastError());
}

template <typename T>
void Multigrid<T>::setup_gathered_coarsest() {
  MGLevel<T>& lv = *lv_.back();
  const Geometry& gd = *lv.g;
  DDAMG_REQUIRE(par_.odd_even == 1, "the gathered coarsest level runs the odd-even Schur complement solve (odd_even = 1)");
  GatheredCoarsest<T>& G = gath_;
  int Lg[4];
  for (int mu = 0; mu < 4; mu++) Lg[mu] = gd.L[mu] * gd.P[mu];
  G.g.build(Lg, Lg, Lg);
  G.V_local = gd.V;
  const int V = G.g.V, n = lv.n, np = gd.nranks;
  DDAMG_REQUIRE((long long)gd.V * np == V, "gathered coarsest lattice: process grid does not tile the lattice");
  for (int mu = 0; mu < 4; mu++) DDAMG_REQUIRE(Lg[mu] % 2 == 0, "the coarsest lattice must have even global extents (odd-even preconditioning)");
  // where every site of the whole lattice lives: each process orders its part by the parity of the GLOBAL lattice, which
  // depends on the parity of its origin
  std::vector<int> g2d(V, -1), d2g(gd.V, -1);
  for (int r = 0; r < np; r++) {
    int pc[4], rr = r;
    for (int mu = 3; mu >= 0; mu--) { pc[mu] = rr % gd.P[mu]; rr /= gd.P[mu]; }
    Geometry gr;
    gr.build(gd.L, gd.B, gd.A, gd.P, pc);
    for (int s = 0; s < gr.V; s++) {
      int c[4];
      for (int mu = 0; mu < 4; mu++) c[mu] = pc[mu] * gd.L[mu] + gr.coord[(size_t)s * 4 + mu];
      const int sg = G.g.site_of_lex[G.g.lex(c)];
      g2d[sg] = r * gd.V + s;
      if (r == gd.rank) d2g[s] = sg;
    }
  }
  for (int s = 0; s < V; s++) DDAMG_REQUIRE(g2d[s] >= 0, "gathered coarsest lattice: a site has no owner");
  G.d_g2d.alloc(V);
  G.d_d2g.alloc(gd.V);
  DDAMG_HIP_CHECK(hipMemcpy(G.d_g2d, g2d.data(), sizeof(int) * V, hipMemcpyHostToDevice));
  DDAMG_HIP_CHECK(hipMemcpy(G.d_d2g, d2g.data(), sizeof(int) * gd.V, hipMemcpyHostToDevice));
  G.cop.alloc(G.g, n, knobs_);
  const size_t nel = (size_t)V * n * 2;
  for (int i = 0; i < 2; i++) { G.buf[i].alloc(nel); DDAMG_HIP_CHECK(device_zero(G.buf[i], sizeof(T) * nel)); }
  // landing zone of the all-gathers: the operator is the larger payload (5 matrices per site)
  const size_t raw_elems = std::max((size_t)V * 5 * lv.cop.msize() * 2, nel);
  G.raw.alloc(raw_elems);
  G.rw.init(std::max(par_.coarse_iter, 8) + 4);
  G.gm.pipelined = false;     // nothing to hide: the reductions are local
  G.gm.single_allreduce = knobs_.single_allreduce_arnoldi;
  G.gm.alloc(nel, par_.coarse_iter, false);
  G.gm.num_restart = par_.coarse_restart;
  G.gm.tol = par_.coarse_tol;
  G.gm.st = st_; G.gm.rw = &G.rw;
  int n_even = 0;
  for (int s = 0; s < V; s++) if (G.g.parity[s] == 0) n_even++;
  DDAMG_REQUIRE(n_even * 2 == V, "coarsest lattice needs as many even as odd sites");
  G.gm.view = View{1, 0, 0, (size_t)n_even * n * 2};
  G.gm.op = [this](T* out, const T* in) { this->schur_on(true, gath_.g.V, gath_.buf[0], gath_.buf[1], out, in); };
  G.on = true;
}

template <typename T>
void Multigrid<T>::regather_coarsest_operator() {
  if (!gath_.on) return;
  MGLevel<T>& lv = *lv_.back();
  const size_t row = 5 * lv.cop.msize() * 2;      // reals per site: five matrices
  comm_allgather(comm_, lv.cop.matrices(), gath_.raw, sizeof(T) * row * (size_t)gath_.V_local, st_);
  gather_rows<T>(gath_.cop.matrices(), gath_.raw, gath_.d_g2d, gath_.g.V, row, st_);
  gath_.cop.compute_self_inverse(st_);
}

template <typename T>
Multigrid<T>::~Multigrid() {
  (void)hipStreamSynchronize(st_);
}

// ---- level-generic pieces ---------------------------------------------------------------------------
template <typename T> void Multigrid<T>::apply_op(int l, T* out, const T* in) {
  if (l == 0) lv_[0]->fop->apply(out, in, st_);
  else if (CoarseHalf* h = half_of(l)) {
    if (lv_[l]->coarsest) {   // self coupling, then the hopping terms on top of it
      DDAMG_REQUIRE(out != in, "coarse apply cannot run in place");
      const int V = lv_[l]->cop.V();
      coarsest_self_mul(false, out, in, 0, V, false);
      coarsest_hop(false, out, in, 0, V, -1.0, true);
    } else if constexpr (sizeof(T) == 4) h->apply(lv_[l]->cop, out, in, st_);
  }
  else lv_[l]->cop.apply(out, in, st_);
}

// ---- 16-bit storage for the solve (half_storage.h) -------------------------------------------------------
template <typename T>
void Multigrid<T>::set_storage(StorageKind kind, int bits) {
  DDAMG_REQUIRE(bits == 32 || (bits == 16 && sizeof(T) == 4), "storage: 32 bits, or 16 with the fp32 V-cycle");
  storage_.bits[kind] = bits;
  if (bits != 32) return;
  // free this kind's copies; one wait for the stream if any of them is in use
  bool waited = false;
  const auto release = [&](auto& copy) {
    if (!copy.allocated()) return;
    if (!waited) { DDAMG_HIP_CHECK(hipStreamSynchronize(st_)); waited = true; }
    copy.release();
  };
  if (kind == Transfer) release(thalf_);
  if (kind == Coarse) { release(lv_.back()->half); release(gath_.half); }
  if (kind == Intermediate) for (int l = 1; l + 1 < num_levels(); l++) release(lv_[l]->half);
}
template <typename T>
void Multigrid<T>::coarsest_hop(bool gathered, T* out, const T* in, int s0, int s1, double sign, bool accumulate) {
  const CoarseOp<T>& cop = gathered ? gath_.cop : lv_.back()->cop;
  if constexpr (sizeof(T) == 4) { if (CoarseHalf* h = half_of(num_levels() - 1, gathered)) { h->hop(cop, out, in, s0, s1, sign, accumulate, st_); return; } }
  cop.hop(out, in, s0, s1, sign, accumulate, st_);
}
template <typename T>
void Multigrid<T>::coarsest_self_mul(bool gathered, T* out, const T* in, int s0, int s1, bool inverse) {
  const CoarseOp<T>& cop = gathered ? gath_.cop : lv_.back()->cop;
  if constexpr (sizeof(T) == 4) { if (CoarseHalf* h = half_of(num_levels() - 1, gathered)) { h->self_mul(cop, out, in, s0, s1, inverse, st_); return; } }
  cop.self_mul(out, in, s0, s1, inverse, st_);
}
template <typename T> void Multigrid<T>::smoother(int l, T* phi, T* Dphi, const T* eta, int cycles, int res) {
  if (par_.method == 4) {
    DDAMG_REQUIRE(Dphi == nullptr, "the GMRES smoother does not return D*phi");   // ASSERT( Dphi == NULL ), src/vcycle_generic.c:82
    gmres_smoother(l, phi, eta, cycles, res);
    return;
  }
  if (l == 0) lv_[0]->fsap.smooth(phi, Dphi, eta, cycles, res, st_);
  else lv_[l]->csap.smooth(phi, Dphi, eta, cycles, res, st_, half_of(l));
}
template <typename T> void Multigrid<T>::restrict_to(int l, T* phi_c, const T* phi) {
  if constexpr (sizeof(T) == 4) { if (l == 0 && storage_.bits[Transfer] == 16) { thalf_.restrict_to(lv_[0]->fip, phi_c, phi, st_); return; } }
  if (l == 0) lv_[0]->fip.restrict_to(phi_c, phi, st_);
  else lv_[l]->cip.restrict_to(phi_c, phi, st_);
}
template <typename T> void Multigrid<T>::interpolate(int l, T* phi, const T* phi_c, bool add) {
  if constexpr (sizeof(T) == 4) { if (l == 0 && storage_.bits[Transfer] == 16) { thalf_.interpolate(lv_[0]->fip, phi, phi_c, add, st_); return; } }
  if (l == 0) lv_[0]->fip.interpolate(phi, phi_c, add, st_);
  else lv_[l]->cip.interpolate(phi, phi_c, add, st_);
}
template <typename T> void Multigrid<T>::set_kcycle_tol(double tol) {
  for (auto& p : lv_) if (p->depth > 0 && !p->coarsest) p->gm.tol = tol;
}

// ---- GMRES smoother on the odd-even Schur complement of a smoothing level (method 4) ----------------------------
// S = D_ee - D_eo D_oo^-1 D_oe on the even sites (apply_schur_complement_PRECISION src/oddeven_generic.c:704-740,
// coarse_apply_schur_complement_PRECISION src/coarse_oddeven_generic.c).  Vectors keep the level's full length and
// site order; only their even sites carry the Krylov vectors (fine level: BLAS-1 through a strided even-site view;
// coarse levels: listed kernels, the odd sites stay zero).
template <typename T>
void Multigrid<T>::smoother_schur(int l, T* out, const T* in) {
  MGLevel<T>& lv = *lv_[l];
  T *t = lv.sbuf[0], *u = lv.sbuf[1];
  if (l == 0) {
    const FineOp<T>& D = *lv.fop;
    D.hop(u, in, 1, st_, 1);                // odd: D_oo^-1 H_oe in_e
    D.hop(out, u, 0, st_, 2, in);           // even: D_ee in_e - H_eo D_oo^-1 H_oe in_e
  } else {
    const int *Le = lv.d_parity_sites[0], *Lo = lv.d_parity_sites[1];
    const int ne = lv.n_parity_sites[0], no = lv.n_parity_sites[1];
    lv.cop.self_mul_list(out, in, Le, ne, false, st_);                               // out_e = D_ee in_e
    lv.cop.apply_masked(t, in, Lo, no, nullptr, false, 0.0, -1.0, false, st_);       // t_o = D_oe in_e
    lv.cop.self_mul_list(u, t, Lo, no, true, st_);                                   // u_o = D_oo^-1 t_o
    lv.cop.apply_masked(out, u, Le, ne, nullptr, false, 0.0, +1.0, true, st_);       // out_e -= D_eo u_o
  }
}

// smoother_PRECISION, g.method == 4 with odd-even (src/vcycle_generic.c:48-71) around solve_oddeven_PRECISION
// (src/oddeven_generic.c:740-777) / coarse_solve_odd_even_PRECISION: the system for the correction is reduced to the even
// sites, GMRES(block_iter) runs `cycles` restarts on it from a zero start, the odd sites follow by back substitution.
template <typename T>
void Multigrid<T>::gmres_smoother(int l, T* phi, const T* eta, int cycles, int res) {
  MGLevel<T>& lv = *lv_[l];
  const View all = whole(lv.nel);
  Gmres<T>& gm = lv.sgm;
  if (!par_.odd_even) {
    // l->sp.x = phi; l->sp.b = eta; fgmres( &(l->sp) ) with initial_guess_zero = res, num_restart = n (src/vcycle_generic.c:70-75)
    vec_copy<T>(gm.b, eta, all, st_);
    if (res == RES) vec_copy<T>(gm.x, phi, all, st_);
    gm.num_restart = cycles; gm.initial_guess_zero = res == NO_RES;
    gm.solve();
    vec_copy<T>(phi, gm.x, all, st_);
    return;
  }
  T *t = lv.sbuf[0], *u = lv.sbuf[1], *rhs = lv.sbuf[2];
  // right-hand side: eta, or the residual eta - D phi when phi carries an iterate
  const T* b = eta;
  if (res == RES) {
    apply_op(l, t, phi);
    vec_minus<T>(rhs, eta, t, all, st_);
    b = rhs;
  }
  if (l == 0) {
    const FineOp<T>& D = *lv.fop;
    D.oo_inv(u, b, st_);                          // u_o = D_oo^-1 b_o
    D.hop(t, u, 0, st_);                          // t_e = H_eo D_oo^-1 b_o
    D.parity_select(gm.b, b, t, 0, st_);          // b_e - D_eo D_oo^-1 b_o
    gm.num_restart = cycles; gm.initial_guess_zero = true;
    gm.solve();                                   // S x_e = b_e
    D.hop(t, gm.x, 1, st_);                       // t_o = H_oe x_e
    D.parity_select(u, b, t, 1, st_);             // b_o - D_oe x_e on the odd sites
    D.oo_inv(t, u, st_);                          // x_o
    if (res == NO_RES) vec_plus<T>(phi, gm.x, t, all, st_);
    else { vec_plus<T>(u, gm.x, t, all, st_); vec_plus<T>(phi, phi, u, all, st_); }
  } else {
    const int *Le = lv.d_parity_sites[0], *Lo = lv.d_parity_sites[1];
    const int ne = lv.n_parity_sites[0], no = lv.n_parity_sites[1];
    T* x = u;                                                                        // assembled correction
    lv.cop.self_mul_list(x, b, Lo, no, true, st_);                                   // x_o = D_oo^-1 b_o
    vec_zero<T>(gm.b, all, st_);
    lv.cop.apply_masked(gm.b, x, Le, ne, nullptr, false, 0.0, +1.0, false, st_);     // -D_eo x_o on the even sites
    aos_list_copy<T>(gm.b, b, Le, ne, lv.n, true, st_);                                     // + b_e
    gm.num_restart = cycles; gm.initial_guess_zero = true;
    gm.solve();
    vec_copy<T>(t, b, all, st_);
    lv.cop.apply_masked(t, gm.x, Lo, no, nullptr, false, 0.0, +1.0, true, st_);      // t_o = b_o - D_oe x_e
    lv.cop.self_mul_list(x, t, Lo, no, true, st_);                                   // x_o = D_oo^-1 t_o
    aos_list_copy<T>(x, gm.x, Le, ne, lv.n, false, st_);                                    // x_e
    if (res == NO_RES) vec_copy<T>(phi, x, all, st_);
    else vec_plus<T>(phi, phi, x, all, st_);
  }
}

template <typename T>
void Multigrid<T>::coarsest_hop_parity(T* out, const T* in, int parity, double sign, bool accumulate) {
  DDAMG_REQUIRE(par_.odd_even && (parity == 0 || parity == 1), "coarsest hopping term by parity: odd_even = 1, parity 0 or 1");
  const int V = lv_.back()->cop.V(), Ve = V / 2;
  coarsest_hop(false, out, in, parity ? Ve : 0, parity ? V : Ve, sign, accumulate);
}
template <typename T>
void Multigrid<T>::coarsest_self_mul_parity(T* out, const T* in, int parity, bool inverse) {
  DDAMG_REQUIRE(par_.odd_even && (parity == 0 || parity == 1), "coarsest self coupling by parity: odd_even = 1, parity 0 or 1");
  const int V = lv_.back()->cop.V(), Ve = V / 2;
  coarsest_self_mul(false, out, in, parity ? Ve : 0, parity ? V : Ve, inverse);
}

// ---- coarsest level: odd-even Schur complement solve ----------------------------------------------
// S = D_ee - D_eo D_oo^-1 D_oe  on the even sites (coarse_apply_schur_complement_PRECISION)
template <typename T>
void Multigrid<T>::schur_on(bool gathered, int V, T* t0, T* t1, T* out, const T* in) {
  const int Ve = V / 2;
  coarsest_self_mul(gathered, out, in, 0, Ve, false);        // out_e = D_ee in_e
  coarsest_hop(gathered, t0, in, Ve, V, -1.0, false);        // tmp0_o = -H_oe in_e   (= D_oe in_e)
  coarsest_self_mul(gathered, t1, t0, Ve, V, true);          // tmp1_o = D_oo^-1 tmp0_o
  coarsest_hop(gathered, out, t1, 0, Ve, +1.0, true);        // out_e += H_eo tmp1_o  (= -D_eo tmp1_o)
}
template <typename T>
void Multigrid<T>::schur(T* out, const T* in) {
  MGLevel<T>& lv = *lv_.back();
  schur_on(false, lv.g->V, lv.buf[0], lv.buf[1], out, in);
}

template <typename T>
int Multigrid<T>::coarse_solve() {
  MGLevel<T>& lv = *lv_.back();
  const int V = lv.g->V, Ve = V / 2;
  T *x = lv.gm.x, *b = lv.gm.b;
  if (!par_.odd_even) {
    const int it = lv.gm.solve();
    coarse_iter_count += it;
    return it;
  }
  if (gath_.on) {
    // one all-gather of the right-hand side, the solve on the whole lattice (every process the same, bit for bit: the
    // kernels are deterministic), my part of the solution
    GatheredCoarsest<T>& G = gath_;
    const size_t row = (size_t)lv.n * 2;
    const int Vg = G.g.V, Vge = Vg / 2;
    comm_allgather(comm_, b, G.raw, sizeof(T) * row * (size_t)G.V_local, st_);
    T *gx = G.gm.x, *gb = G.gm.b;
    gather_rows<T>(gb, G.raw, G.d_g2d, Vg, row, st_);
    coarsest_self_mul(true, gx, gb, Vge, Vg, true);
    coarsest_hop(true, gb, gx, 0, Vge, +1.0, true);
    const int it = G.gm.solve();
    coarsest_hop(true, gb, gx, Vge, Vg, +1.0, true);
    coarsest_self_mul(true, gx, gb, Vge, Vg, true);
    gather_rows<T>(x, gx, G.d_d2g, G.V_local, row, st_);
    coarse_iter_count += it;
    return it;
  }
  coarsest_self_mul(false, x, b, Ve, V, true);     // x_o = D_oo^-1 b_o
  coarsest_hop(false, b, x, 0, Ve, +1.0, true);    // b_e <- b_e - D_eo x_o
  int it = lv.gm.solve();                           // S x_e = b_e  to coarse_tol
  coarsest_hop(false, b, x, Ve, V, +1.0, true);    // b_o <- b_o - D_oe x_e
  coarsest_self_mul(false, x, b, Ve, V, true);     // x_o = D_oo^-1 b_o
  coarse_iter_count += it;
  return it;
}

template <typename T>
bool Multigrid<T>::coarse_solve_many(T* X, size_t xstride, const T* B, size_t bstride, int ncols, int* iters) {
  if constexpr (sizeof(T) == 4) {
    MGLevel<T>& lv = *lv_.back();
    if (gath_.on || !LockstepCoarseSolver::available(lv.cop, ncols, par_.odd_even != 0)) return false;
    if (!lockstep_.ready()) lockstep_.init(&lv.cop, std::min(lv.gm.restart_length, 24), lv.gm.tol, st_);
    coarse_iter_count += lockstep_.solve(X, xstride, B, bstride, ncols, iters);
    return true;
  }
  return false;
}

template <typename T>
bool Multigrid<T>::coarsest_apply_many(T* out, size_t ostride, const T* in, size_t istride, int ncols) {
  if constexpr (sizeof(T) == 4) {
    MGLevel<T>& lv = *lv_.back();
    if (gath_.on || !LockstepCoarseSolver::available(lv.cop, ncols, par_.odd_even != 0)) return false;
    ensure_lockstep();
    lockstep_.gather(lockstep_.batch(2), in, istride, ncols);
    lockstep_.apply(lockstep_.batch(3), lockstep_.batch(2));
    lockstep_.scatter(out, ostride, lockstep_.batch(3), ncols);
    return true;
  }
  return false;
}

// ---- the intermediate levels for many right-hand sides (coarse_multi.h): level 1 of three levels, levels 1 and 2 of four -------
template <typename T>
void Multigrid<T>::ensure_lockstep() {
  if constexpr (sizeof(T) == 4) {
    MGLevel<T>& lc = *lv_.back();
    if (!lockstep_.ready()) lockstep_.init(&lc.cop, std::min(lc.gm.restart_length, 24), lc.gm.tol, st_);
  }
}
template <typename T>
bool Multigrid<T>::multi_refuse(int l, const char* why) {
  if (knobs_.setup_timing && !multi_noticed_[l]) fprintf(stderr, "[ddamg setup] level %d one vector at a time: %s\n", l, why);
  multi_noticed_[l] = true;
  return false;
}
template <typename T>
bool Multigrid<T>::multi_ready(int l, int ncols) {
  if constexpr (sizeof(T) == 4) {
    const int L = num_levels();
    if (l < 1 || l > L - 2 || ncols < 2 || ncols > LOCKSTEP_COLS) return false;
    // mixed precision 2: the K-cycle takes D*phi out of the smoother's residual (src/linsolve_generic.c:757,828-835), which the
    // batched smoother does not return -- one vector at a time there
    if (comm_ != nullptr) return multi_refuse(l, "process grid");
    if (gath_.on) return multi_refuse(l, "gathered coarsest level");
    if (par_.mixed_precision == 2) return multi_refuse(l, "mixed_precision = 2");
    if (!par_.odd_even) return multi_refuse(l, "odd_even = 0");
    // every intermediate level from this one down, or none: a V-cycle of level l goes through all of them
    size_t need = 0;
    for (int d = l; d <= L - 2; d++) {
      MGLevel<T>& ld = *lv_[d];
      if (ld.nvec > 32) return multi_refuse(d, "more than 32 test vectors");
      if (!CoarseMulti::available(*ld.g, ld.cop, par_.method)) return multi_refuse(d, "method, dof count, block size or block colouring not covered");
      if (!multi_[d].ready()) need += CoarseMulti::workspace_bytes(*ld.g, ld.n, ld.gm.restart_length);
    }
    if (!LockstepCoarseSolver::available(lv_[L - 1]->cop, ncols, true)) return multi_refuse(L - 1, "coarsest level not covered by the lockstep solver");
    if (need > 0) {
      // the batches are tens of GB at 64^4: next to a context that already holds its solver workspace they may not fit, and a
      // failed allocation in the middle of a setup is worse than the one-vector-at-a-time path.  All levels involved together,
      // before any of them allocates.
      size_t free_b = 0, total_b = 0;
      DDAMG_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
      if (need + need / 8 > free_b) {
        if (knobs_.setup_timing) fprintf(stderr, "[ddamg setup] level %d one vector at a time: %zu bytes free, %zu needed from this level down\n", l, free_b, need);
        return false;
      }
      for (int d = l; d <= L - 2; d++) {
        if (multi_[d].ready()) continue;
        MGLevel<T>& ld = *lv_[d];
        multi_[d].init(*ld.g, &ld.cop, &ld.cip, par_.block_iter[d], st_);
        if (knobs_.setup_timing) fprintf(stderr, "[ddamg setup] level %d all vectors at once: %d dof per site, %d sites\n", d, ld.n, ld.g->V);
      }
    }
    ensure_lockstep();
    return true;
  }
  return false;
}
template <typename T>
const CoarseMulti::Nested* Multigrid<T>::multi_nested(int l, CoarseMulti::Nested* chain) {
  if constexpr (sizeof(T) == 4) {
    const int L = num_levels();
    const CoarseMulti::Nested* below = nullptr;
    for (int d = L - 2; d > l; d--) {       // from the deepest intermediate level up to l + 1
      MGLevel<T>& ld = *lv_[d];
      chain[d].level = &multi_[d];
      chain[d].m = ld.gm.restart_length; chain[d].cycles = ld.gm.num_restart; chain[d].tol = ld.gm.tol;
      chain[d].post_smooth = par_.post_smooth_iter[d];
      chain[d].nested = below;
      below = &chain[d];
    }
    return below;
  }
  return nullptr;
}
template <typename T>
int Multigrid<T>::multi_vcycle(int l, float2* phi, const float2* eta, int ncols) {
  if constexpr (sizeof(T) == 4) {
    MGLevel<T>& lc = *lv_.back();
    CoarseMulti::Nested chain[DDAMG_HIP_MAX_LEVELS];
    const int it = multi_[l].vcycle(phi, eta, ncols, par_.post_smooth_iter[l], lockstep_, [this] { this->coarse_solve(); }, lc.gm.x, lc.gm.b, nullptr, multi_nested(l, chain));
    coarse_iter_count += it;
    return it;
  }
  return 0;
}
template <typename T>
int Multigrid<T>::multi_kcycle(int l, float2* X, const float2* B, int ncols, int* iters) {
  if constexpr (sizeof(T) == 4) {
    MGLevel<T>& ll = *lv_[l];
    MGLevel<T>& lc = *lv_.back();
    CoarseMulti::Nested chain[DDAMG_HIP_MAX_LEVELS];
    const int it = multi_[l].kcycle(X, B, ncols, ll.gm.restart_length, ll.gm.num_restart, ll.gm.tol, par_.post_smooth_iter[l], lockstep_,
                                    [this] { this->coarse_solve(); }, lc.gm.x, lc.gm.b, iters, nullptr, multi_nested(l, chain));
    coarse_iter_count += it;
    return it;
  }
  return 0;
}
template <typename T>
void Multigrid<T>::multi_update_deeper(int l, int ncols) {
  if constexpr (sizeof(T) == 4) {
    // the one-vector code takes gm.x of the LAST level-d K-cycle that ran for vector i (bootstrap()); in lockstep that is the
    // level-d iterate batch as the last V-cycle in which column i took part left it (CoarseMulti::next_iterate)
    for (int d = num_levels() - 2; d > l; d--) {
      float2* Xd = multi_[d - 1].next_iterate();
      const int nup = std::min(ncols, lv_[d]->nvec);
      multi_[d].normalize_columns(Xd);
      multi_[d].scatter(tv_base(d), tv_stride(d), Xd, nup);
    }
  }
}
template <typename T>
bool Multigrid<T>::multi_apply_many(int l, T* out, size_t ostride, const T* in, size_t istride, int ncols) {
  if constexpr (sizeof(T) == 4) {
    if (!multi_ready(l, ncols)) return false;
    CoarseMulti& m = multi_[l];
    m.gather(m.work(0), in, istride, ncols);
    m.apply(m.work(1), m.work(0));
    m.scatter(out, ostride, m.work(1), ncols);
    return true;
  }
  return false;
}
template <typename T>
bool Multigrid<T>::multi_smooth_many(int l, T* phi, size_t pstride, const T* eta, size_t estride, int ncols, int cycles, int res) {
  if constexpr (sizeof(T) == 4) {
    if (!multi_ready(l, ncols)) return false;
    CoarseMulti& m = multi_[l];
    m.gather(m.work(0), eta, estride, ncols);
    if (res == RES) m.gather(m.work(1), phi, pstride, ncols);
    m.smooth(m.work(1), m.work(0), cycles, res);
    m.scatter(phi, pstride, m.work(1), ncols);
    return true;
  }
  return false;
}
template <typename T>
bool Multigrid<T>::multi_vcycle_many(int l, T* phi, size_t pstride, const T* eta, size_t estride, int ncols) {
  if constexpr (sizeof(T) == 4) {
    // above another intermediate level the V-cycle runs that level's K-cycle in lockstep: without K-cycles one vector at a time
    if (!multi_ready(l, ncols) || (l < num_levels() - 2 && !par_.kcycle)) return false;
    CoarseMulti& m = multi_[l];
    m.gather(m.work(0), eta, estride, ncols);
    multi_vcycle(l, m.work(1), m.work(0), ncols);
    m.scatter(phi, pstride, m.work(1), ncols);
    return true;
  }
  return false;
}
template <typename T>
bool Multigrid<T>::multi_kcycle_many(int l, T* x, size_t xstride, const T* b, size_t bstride, int ncols, int* iters) {
  if constexpr (sizeof(T) == 4) {
    if (!multi_ready(l, ncols) || !par_.kcycle) return false;
    CoarseMulti& m = multi_[l];
    m.gather(m.work(0), b, bstride, ncols);
    multi_kcycle(l, m.work(1), m.work(0), ncols, iters);
    m.scatter(x, xstride, m.work(1), ncols);
    return true;
  }
  return false;
}
template <typename T>
int Multigrid<T>::kcycle_solve(int l) {
  MGLevel<T>& lv = *lv_[l];
  DDAMG_REQUIRE(l > 0 && !lv.coarsest && par_.kcycle, "kcycle_solve: an intermediate level with the K-cycle switched on");
  lv.gm.initial_guess_zero = true;
  return lv.gm.solve();
}

// ---- V-cycle / K-cycle (post-smoothing only) --------------------------------------------------------
template <typename T>
void Multigrid<T>::vcycle(int l, T* phi, T* Dphi, const T* eta, int res) {
  MGLevel<T>& lv = *lv_[l];
  MGLevel<T>& nx = *lv_[l + 1];
  if (res == NO_RES) {
    restrict_to(l, nx.gm.b, eta);
  } else {
    apply_op(l, lv.buf[0], phi);
    vec_minus<T>(lv.buf[1], eta, lv.buf[0], whole(lv.nel), st_);
    restrict_to(l, nx.gm.b, lv.buf[1]);
  }
  if (nx.coarsest) {
    coarse_solve();
  } else if (par_.kcycle) {
    nx.gm.initial_guess_zero = true;
    nx.gm.solve();     // FGMRES on level l+1, preconditioned by vcycle(l+1)
  } else {
    vcycle(l + 1, nx.gm.x, nullptr, nx.gm.b, NO_RES);
  }
  interpolate(l, phi, nx.gm.x, res != NO_RES);
  smoother(l, phi, Dphi, eta, par_.post_smooth_iter[l], RES);
}

// ---- setup ------------------------------------------------------------------------------------------
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
template <typename T>
double Multigrid<T>::tick(const char* phase, double t0) {
  if (!knobs_.setup_timing) return 0;
  DDAMG_HIP_CHECK(hipStreamSynchronize(st_));
  const double t = now_s();
  if (phase) {
    bool found = false;
    for (auto& e : setup_times) if (e.first == phase) { e.second += t - t0; found = true; }
    if (!found) setup_times.emplace_back(phase, t - t0);
  }
  return t;
}

template <typename T>
double Multigrid<T>::norm_of(int l, const T* v) {
  return host_norm<T>(v, whole(lv_[l]->nel), lv_[l]->rw, st_);
}

// vector_PRECISION_define_random (src/data_generic.c:42-56): libc rand(), in the order of the reference's
// vector loop on this level; gcc evaluates the imaginary operand's rand() first (fixture rng_probe)
template <typename T>
void Multigrid<T>::random_vector(int l, T* dst) {
  MGLevel<T>& lv = *lv_[l];
  const int n = lv.n, V = lv.g->V;
  if (par_.test_vector_rng == 1) {
    // device generator: the layout of the vector does not matter for independent uniform numbers
    vec_random<T>(dst, lv.nel, par_.rng_seed + 7919ull * (unsigned long long)lv.g->rank, rng_stream_++, st_);
    return;
  }
  if (l == 0 && !par_.odd_even && ref_order0_.empty()) {
    // without odd-even the reference's Schwarz layout of the fine level is lexicographic inside a block
    // (src/schwarz_generic.c:449-486); ours keeps the parity split
    const Geometry& g = *lv.g;
    ref_order0_.resize(V);
    for (int b = 0; b < g.num_blocks; b++) {
      std::vector<std::pair<int, int>> o;
      for (int i = 0; i < g.block_sites; i++) { const int s = b * g.block_sites + i; o.emplace_back(g.lex_of_site[s], s); }
      std::sort(o.begin(), o.end());
      for (int i = 0; i < g.block_sites; i++) ref_order0_[(size_t)b * g.block_sites + i] = o[i].second;
    }
  }
  std::vector<double> h((size_t)V * n * 2);
  for (int pos = 0; pos < V; pos++) {
    const size_t site = l == 0 ? (ref_order0_.empty() ? (size_t)pos : (size_t)ref_order0_[pos]) : (size_t)lv.ref_order[pos];
    for (int d = 0; d < n; d++) {
      const double im = (double)(T)(((double)rand() / (double)RAND_MAX)) - 0.5;
      const double re = (double)(T)(((double)rand() / (double)RAND_MAX)) - 0.5;
      h[(site * n + d) * 2] = re; h[(site * n + d) * 2 + 1] = im;
    }
  }
  DDAMG_HIP_CHECK(hipMemcpyAsync(d_stage_, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, st_));
  if (l == 0) vec_from_lex<T>(dst, d_stage_, d_identity0_, V, 12, st_);
  else aos_from_lex<T>(dst, d_stage_, d_identity0_, V, n, st_);   // identity order: the host array is already site-major
  DDAMG_HIP_CHECK(hipStreamSynchronize(st_));
}

template <typename T>
void Multigrid<T>::define_interpolation(int l) {
  MGLevel<T>& lv = *lv_[l];
  const View all = whole(lv.nel);
  bool batched = false;
  if constexpr (sizeof(T) == 4) {
    if (l >= 1 && par_.method == 2 && multi_ready(l, lv.nvec)) {
      // the three smoother passes of all test vectors of the level at once (coarse_multi.h); the random numbers in the
      // reference's order first
      double t0 = tick(nullptr, 0);
      for (int k = 0; k < lv.nvec; k++) random_vector(l, test_vector(l, k));
      t0 = tick("random test vectors", t0);
      CoarseMulti& m = multi_[l];
      float2 *A = m.work(0), *Bt = m.work(1);
      m.gather(A, tv_base(l), tv_stride(l), lv.nvec);
      m.smooth(Bt, A, 1, NO_RES);
      m.smooth(A, Bt, 2, NO_RES);
      m.smooth(Bt, A, 3, NO_RES);
      m.scatter(tv_base(l), tv_stride(l), Bt, lv.nvec);
      tick("initial smoothing", t0);
      batched = true;
    }
  }
  for (int k = 0; k < lv.nvec && !batched; k++) {
    T* tv = test_vector(l, k);
    double t0 = tick(nullptr, 0);
    random_vector(l, tv);
    t0 = tick("random test vectors", t0);
    // three smoother passes with 1, 2, 3 cycles -- one cycle each with the GMRES smoother (src/setup_generic.c:215-231)
    // (the three passes alternate between the test vector and a work vector: one copy at the end instead of one per pass)
    smoother(l, lv.buf[2], nullptr, tv, 1, NO_RES);
    smoother(l, tv, nullptr, lv.buf[2], par_.method >= 4 ? 1 : 2, NO_RES);
    smoother(l, lv.buf[2], nullptr, tv, par_.method >= 4 ? 1 : 3, NO_RES);
    vec_copy<T>(tv, lv.buf[2], all, st_);
    tick("initial smoothing", t0);
  }
  for (int k = 0; k < lv.nvec; k++) {
    T* tv = test_vector(l, k);
    vec_scale<T>(tv, tv, 1.0 / norm_of(l, tv), 0.0, all, st_);
  }
}

template <typename T>
void Multigrid<T>::orthonormalize(int l) {
  // interpolation <- test vectors, Gram-Schmidt on aggregates; done twice on depth > 0 in re_setup (src/setup_generic.c:291-292)
  if (l == 0) lv_[0]->fip.orthonormalize(st_);
  else lv_[l]->cip.orthonormalize(2, st_);
}

template <typename T>
void Multigrid<T>::build_coarse_operator(int l) {
  MGLevel<T>& lv = *lv_[l];
  MGLevel<T>& nx = *lv_[l + 1];
  const int N = lv.nvec;
  const double t_start = tick(nullptr, 0);
  const bool no_batch = knobs_.galerkin_unbatched;
  if (l == 0 && !no_batch && Interpolation<T>::restrict_batch_available(lv.fip.agg_sites, N)) {
    // batched form: D P for a whole batch of columns (5 fields each), then ONE restriction on the matrix cores
    const size_t ws = (size_t)24 * lv.g->V;             // one fine vector
    const size_t cs = (size_t)nx.g->V * nx.n * 2;       // one coarse vector
    // the four forward parts of a column on the aggregate faces only (AggFaces, transfer.h): 2 instead of 5 fields per column
    // to write and to restrict with 4^4 aggregates
    const bool no_compact = knobs_.galerkin_full_fields;
    const AggFaces& af = lv.agg_faces;
    const bool compact = !no_compact && 2 * N <= 64 && Interpolation<T>::restrict_compact_available(lv.fip.agg_sites, N, af);
    // ... and their restriction written straight into the next level's matrices (DDAMG_GALERKIN_STORE_COLUMNS: through coarse
    // column vectors and one store launch per column, as the full-field path does)
    const bool direct = compact && !knobs_.galerkin_store_columns;
    const int nagg = lv.fip.num_aggs, as = lv.fip.agg_sites;
    const size_t wcol = compact ? (size_t)24 * af.column_sites(nagg) : 5 * ws;          // one column of W, whole lattice
    const size_t wcol_agg = compact ? (size_t)24 * af.column_sites(1) : (size_t)5 * 24 * as;   // ... one aggregate of it
    const int max_batch = compact ? 64 : 256 / 5;
    // the batch workspace is allocated once per setup and kept until release_setup_workspace(): allocating and
    // freeing tens of GB for every build costs more than the build itself
    if (!gal_W_) {
      size_t free_b = 0, total_b = 0;
      DDAMG_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
      gal_batch_ = 2 * N;
      while (gal_batch_ > 1 && (gal_batch_ > max_batch || sizeof(T) * gal_batch_ * (wcol + 5 * cs) > free_b / 2)) gal_batch_ = (gal_batch_ + 1) / 2;
      gal_slab_aggs_ = 0;
      if (2 * N <= max_batch && !lv.fop->distributed()) {
        // keep ALL columns and walk the lattice in slabs of whole aggregates -- D P and its restriction are local to an
        // aggregate.  Fewer columns per pass would starve the N dimension of the restriction GEMM (64^4: 6 of 48 columns, 30 of
        // 240 fields, 4x the time).
        // The slab is no larger than what the bootstrap borrows (Nvec fine vectors) or 512 aggregates: the time of a build does
        // not depend on the slab size from 512 aggregates on, and memory that is never allocated need not be mapped -- the first
        // process on a freshly started box pays ~20-40 ms per GB of never-used device memory (docs/design/09_rounds_2_3.md)
        const size_t per_agg = sizeof(T) * 2 * N * wcol_agg;
        const size_t coarse_b = sizeof(T) * 5 * 2 * N * cs;           // gal_C_: all columns on the coarse lattice
        DDAMG_REQUIRE(coarse_b + per_agg < free_b, "Galerkin construction: not enough device memory for the coarse columns and one aggregate of fields");
        // half of the free memory for the two buffers where that leaves room for at least one aggregate, else what is left
        // after the coarse columns (unsigned arithmetic: never subtract past zero)
        const size_t budget = free_b / 2 > coarse_b + per_agg ? free_b / 2 - coarse_b : free_b - coarse_b - (free_b - coarse_b) / 8;
        gal_slab_aggs_ = (int)std::min<size_t>((size_t)nagg, std::max<size_t>(1, budget / per_agg));
        const size_t borrow = (sizeof(T) * (size_t)N * ws + per_agg - 1) / per_agg;      // aggregates whose slab holds Nvec fine vectors
        gal_slab_aggs_ = (int)std::min<size_t>((size_t)gal_slab_aggs_, std::max<size_t>(borrow, 512));
        if (knobs_.galerkin_slab_aggs.set) gal_slab_aggs_ = std::max(1, std::min(knobs_.galerkin_slab_aggs.value, nagg));   // tests
        DDAMG_REQUIRE(per_agg * (size_t)gal_slab_aggs_ + coarse_b < free_b, "Galerkin construction: slab workspace does not fit the free device memory");
        gal_batch_ = 2 * N;
        gal_W_.alloc(per_agg / sizeof(T) * (size_t)gal_slab_aggs_);
      } else {
        gal_W_.alloc((size_t)gal_batch_ * wcol);
      }
      // coarse column vectors: five per column, or -- with the restriction writing straight into the matrices -- only what the
      // bootstrap borrows (Nvec right-hand sides and Nvec solutions)
      const size_t c_cols = direct ? (size_t)2 * N : (size_t)5 * gal_batch_;
      gal_C_.alloc(c_cols * cs);
    }
    const int batch = gal_batch_;
    DDAMG_REQUIRE(direct || gal_C_.size() >= (size_t)5 * gal_batch_ * cs, "Galerkin construction: the workspace of this context was sized for the direct store of the restriction");
    T *Wb = gal_W_, *Cb = gal_C_;
    if (gal_slab_aggs_ > 0) {
      for (int a0 = 0; a0 < nagg; a0 += gal_slab_aggs_) {
        const int na = std::min(gal_slab_aggs_, nagg - a0);
        const size_t wss = (size_t)24 * na * as;        // one field of this slab
        if (compact) {
          for (int c = 0; c < 2 * N; c++)
            aggregate_dirac_compact<T>(Wb + (size_t)c * na * wcol_agg, interpolation_column(lv.fip, c % N), c / N, *lv.fop, lv.d_agg_face, af, a0, na, knobs_, st_);
          lv.fip.restrict_batch_compact(Cb, cs, Wb, 2 * N, af, a0, na, st_, direct ? nx.cop.matrices() : nullptr, nx.cop.nt(), nx.cop.msize(), 0);
        } else {
          for (int c = 0; c < 2 * N; c++)
            aggregate_dirac_slab<T>(Wb + (size_t)5 * c * wss, interpolation_column(lv.fip, c % N), c / N, *lv.fop, lv.d_agg_face, (size_t)a0 * as, (size_t)na * as, st_);
          lv.fip.restrict_batch_slab(Cb, cs, Wb, wss, 5 * 2 * N, a0, na, st_);
        }
      }
      if (!direct) for (int c = 0; c < 2 * N; c++) galerkin_store_column<T>(nx.cop, Cb + (size_t)5 * c * cs, c, st_);
    } else
    for (int c0 = 0; c0 < 2 * N; c0 += batch) {
      const int nb = std::min(batch, 2 * N - c0);
      if (compact) {
        for (int c = 0; c < nb; c++)
          aggregate_dirac_compact<T>(Wb + (size_t)c * wcol, interpolation_column(lv.fip, (c0 + c) % N), (c0 + c) / N, *lv.fop, lv.d_agg_face, af, 0, nagg, knobs_, st_);
        lv.fip.restrict_batch_compact(Cb, cs, Wb, nb, af, 0, nagg, st_, direct ? nx.cop.matrices() : nullptr, nx.cop.nt(), nx.cop.msize(), c0);
      } else {
        for (int c = 0; c < nb; c++)
          aggregate_dirac<T>(Wb + (size_t)5 * c * ws, interpolation_column(lv.fip, (c0 + c) % N), (c0 + c) / N, *lv.fop, lv.d_agg_face, st_);
        lv.fip.restrict_batch(Cb, cs, Wb, ws, 5 * nb, st_);
      }
      if (!direct) for (int c = 0; c < nb; c++) galerkin_store_column<T>(nx.cop, Cb + (size_t)5 * c * cs, c0 + c, st_);
    }
  } else if (l == 0) {
    for (int chir = 0; chir < 2; chir++)
      for (int j = 0; j < N; j++) {
        if (!W_) W_.alloc(lv_[0]->nel * 5);
        aggregate_dirac<T>(W_, interpolation_column(lv.fip, j), chir, *lv.fop, lv.d_agg_face, st_);
        galerkin_column<T>(nx.cop, lv.fip, W_, chir * N + j, cwork_, st_);
      }
  } else if constexpr (sizeof(T) == 4) {
    if (!no_batch && coarse_galerkin_batch_available(lv.n, 2 * N, sizeof(T))) {
      // all 2*Nvec columns at once on the matrix cores (coarse_batch.hip)
      if (!gal_cwork_) gal_cwork_.alloc(coarse_galerkin_batch_work(lv_[1]->g->V, lv_[1]->n));
      coarse_galerkin_batched(nx.cop, lv.cop, lv.cip, lv.d_agg_face, gal_cwork_, knobs_, st_);
      if (nx.coarsest || par_.method == 4) nx.cop.compute_self_inverse(st_);   // D_oo^-1 of the Schur complements
      if (nx.coarsest) regather_coarsest_operator();
      DDAMG_HIP_CHECK(hipStreamSynchronize(st_));
      tick("Galerkin coarse operator", t_start);
      return;
    }
  }
  if (l > 0) {
    // coarse_aggregate_self_couplings / coarse_aggregate_neighbor_couplings (src/coarse_operator_generic.c:238-285):
    // the same masked gather kernel as the operator itself, restricted with this level's P
    const int V = lv.g->V;
    for (int chir = 0; chir < 2; chir++)
      for (int j = 0; j < N; j++) {
        aos_chirality_copy<T>(lv.buf[2], lv.cip.interp_vector(j), V, lv.n, chir, st_);
        lv.cop.apply_masked(lv.buf[3], lv.buf[2], nullptr, V, lv.d_agg_face, true, 1.0, -1.0, false, st_);
        lv.cip.restrict_to(cwork_, lv.buf[3], st_);
        store_matrix_column<T>(nx.cop, cwork_, 0, chir * N + j, st_);
        for (int mu = 0; mu < 4; mu++) {
          lv.cop.apply_masked(lv.buf[3], lv.buf[2], nullptr, V, lv.d_dir_mask[mu], false, 0.0, +1.0, false, st_);
          lv.cip.restrict_to(cwork_, lv.buf[3], st_);
          store_matrix_column<T>(nx.cop, cwork_, 1 + mu, chir * N + j, st_);
        }
      }
  }
  if (nx.coarsest || par_.method == 4) nx.cop.compute_self_inverse(st_);
  if (nx.coarsest) regather_coarsest_operator();
  DDAMG_HIP_CHECK(hipStreamSynchronize(st_));
  tick("Galerkin coarse operator", t_start);
}

template <typename T>
void Multigrid<T>::release_setup_workspace() {
  DDAMG_HIP_CHECK(hipStreamSynchronize(st_));
  gal_W_.reset(); gal_C_.reset(); gal_cwork_.reset();
  lockstep_.release();
  for (auto& m : multi_) m.release();
}

template <typename T>
void Multigrid<T>::re_setup(int l) {
  if (l == 0) p_orthonormal_ = true;    // every level's interpolation operator is orthonormalised again below
  if (lv_[l]->coarsest) return;
  const double t0 = tick(nullptr, 0);
  orthonormalize(l);
  tick("aggregate Gram-Schmidt", t0);
  build_coarse_operator(l);
  re_setup(l + 1);
}

template <typename T>
void Multigrid<T>::initial_setup() { setup_times.clear(); initial_setup_from(0); }   // the phase times of one setup, not of all so far

template <typename T>
void Multigrid<T>::initial_setup_from(int l0) {
  // method_setup -> next_level_setup -> interpolation_PRECISION_define -> coarse_grid_correction_PRECISION_setup
  const SetupStorage fp32_storage(*this);
  const int L = num_levels();
  if (l0 == 0) p_orthonormal_ = true;
  for (int l = l0; l + 1 < L; l++) {
    MGLevel<T>& lv = *lv_[l];
    if (l > 0) {
      // the reference first fills the extra test vectors of this level with random numbers
      // (src/setup_generic.c:96-101) and then redefines ALL of them at random (:212-214): same rand() stream
      const int nprev = lv_[l - 1]->nvec;
      for (int i = std::min(lv.nvec, nprev); i < lv.nvec; i++) random_vector(l, test_vector(l, i));
    }
    define_interpolation(l);
    if (l == 0) lv.fip.orthonormalize(st_); else lv.cip.orthonormalize(1, st_);
    build_coarse_operator(l);
  }
}

// The Nvec V-cycles of one bootstrap iteration on the fine level do not depend on each other (the interpolation operator
// is a copy of the previous iteration's test vectors), so the two passes over the interpolation operator that every one of
// them makes -- restriction of its right-hand side, interpolation of its coarse correction -- are done for all of them at
// once: P is read twice per iteration instead of 2 Nvec times (32^4, Nvec 24: 2 x 2.4 GB instead of 115 GB), the
// restriction on the matrix cores (restrict_mfma_kernel, the Galerkin construction's kernel).  The coarse solves and the
// smoother calls stay one vector at a time.  Borrows the Galerkin workspace between two builds; fp32.
template <typename T>
bool Multigrid<T>::bootstrap_vcycles_batched() {
  const bool off = knobs_.bootstrap_unbatched;
  MGLevel<T>& lv = *lv_[0];
  MGLevel<T>& nx = *lv_[1];
  const int N = lv.nvec;
  const size_t ws = (size_t)24 * lv.g->V, cs = (size_t)nx.g->V * nx.n * 2;
  // (on a process grid as well: restriction and interpolation are local to the aggregates, which never straddle a process
  // boundary; the coarse solves and smoother calls in between communicate as they do one vector at a time.)
  if (off || sizeof(T) != 4 || !gal_W_ || !gal_C_) return false;
  if (!Interpolation<T>::restrict_batch_available(lv.fip.agg_sites, N) || !Interpolation<T>::interpolate_batch_available(lv.fip.agg_sites, N, N)) return false;
  // the borrowed workspace holds `cap` fine vectors: all Nvec in a first setup; fewer next to a context that already holds its
  // solver workspace (64^4: 17 of 24), and then the interpolation + smoothing at the end goes through it in groups
  int cap = (int)std::min<size_t>((size_t)N, gal_W_.size() / ws);
  if (knobs_.bootstrap_group.set) cap = std::max(1, std::min(cap, knobs_.bootstrap_group.value));   // tests: groups at any volume
  if (cap < 1 || gal_C_.size() < (size_t)2 * N * cs) {
    if (knobs_.setup_timing)
      fprintf(stderr, "[ddamg setup] bootstrap one vector at a time: workspace %zu / %zu elements, needed %zu / %zu\n", gal_W_.size(), gal_C_.size(), (size_t)N * ws, (size_t)2 * N * cs);
    return false;
  }
  T* F = gal_W_;                 // N fine vectors: the iterates of the V-cycles
  T* Cb = gal_C_;                // N coarse right-hand sides
  T* Cx = gal_C_ + (size_t)N * cs;   // N coarse solutions
  const View all = whole(lv.nel), call = whole(nx.nel);
  lv.fip.restrict_batch(Cb, cs, tv_base(0), tv_stride(0), N, st_);
  // two levels: the N coarsest-level solves as N GMRES recurrences in lockstep, the coarse operator on the matrix cores
  // (coarse_lockstep.h); a column that needs more steps than the lockstep basis holds falls back to the one-at-a-time solver
  bool in_lockstep = false;
  if constexpr (sizeof(T) == 4) {
    if (nx.coarsest && !gath_.on && LockstepCoarseSolver::available(nx.cop, N, par_.odd_even != 0)) {
      std::vector<int> its(N);
      coarse_solve_many(Cx, cs, Cb, cs, N, its.data());
      for (int i = 0; i < N; i++)
        if (its[i] < 0) {
          vec_copy<T>(nx.gm.b, Cb + (size_t)i * cs, call, st_);
          coarse_solve();
          vec_copy<T>(Cx + (size_t)i * cs, nx.gm.x, call, st_);
        }
      in_lockstep = true;
    }
  }
  if constexpr (sizeof(T) == 4) {
    if (!nx.coarsest && par_.kcycle && multi_ready(1, N)) {
      // three and four levels: the N K-cycles of level 1 in lockstep -- operator, Schwarz smoother, transfers and the coarsest
      // solves for all columns at once (coarse_multi.h), every column with its own FGMRES recurrence; on four levels the K-cycles
      // of level 2 inside every V-cycle of level 1 the same way
      CoarseMulti& m1 = multi_[1];
      float2 *B1 = m1.work(0), *X1 = m1.work(1);
      std::vector<int> its(N);
      m1.gather(B1, Cb, cs, N);
      multi_kcycle(1, X1, B1, N, its.data());
      m1.scatter(Cx, cs, X1, N);
      // test_vector_PRECISION_update of the intermediate levels from their K-cycle iterates: the deeper level first
      multi_update_deeper(1, N);
      const int nup = std::min(N, nx.nvec);
      m1.normalize_columns(X1);
      m1.scatter(tv_base(1), tv_stride(1), X1, nup);
      in_lockstep = true;
    }
  }
  for (int i = 0; i < N && !in_lockstep; i++) {
    vec_copy<T>(nx.gm.b, Cb + (size_t)i * cs, call, st_);
    if (nx.coarsest) {
      coarse_solve();
    } else if (par_.kcycle) {
      nx.gm.initial_guess_zero = true;
      nx.gm.solve();
    } else {
      vcycle(1, nx.gm.x, nullptr, nx.gm.b, NO_RES);
    }
    // test_vector_PRECISION_update of the deeper intermediate levels, from their K-cycle iterate of THIS V-cycle
    for (int d = num_levels() - 2; d > 0; d--) {
      MGLevel<T>& dl = *lv_[d];
      if (i < dl.nvec) vec_scale<T>(test_vector(d, i), dl.gm.x, 1.0 / norm_of(d, dl.gm.x), 0.0, whole(dl.nel), st_);
    }
    vec_copy<T>(Cx + (size_t)i * cs, nx.gm.x, call, st_);
  }
  for (int i0 = 0; i0 < N; i0 += cap) {
    const int ni = std::min(cap, N - i0);
    lv.fip.interpolate_batch(F, ws, Cx + (size_t)i0 * cs, cs, ni, st_);
    for (int i = 0; i < ni; i++) {
      T* out = F + (size_t)i * ws;
      smoother(0, out, nullptr, test_vector(0, i0 + i), par_.post_smooth_iter[0], RES);
      vec_scale<T>(test_vector(0, i0 + i), out, 1.0 / norm_of(0, out), 0.0, all, st_);
    }
  }
  return true;
}

template <typename T>
void Multigrid<T>::bootstrap(int l, int iters) {
  MGLevel<T>& lv = *lv_[l];
  const View all = whole(lv.nel);
  const size_t stride = tv_stride(l);
  for (int j = 0; j < iters; j++) {
    // gram_schmidt_PRECISION on the test vectors (classical, src/linalg_generic.c:483-528)
    double tb = tick(nullptr, 0);
    // By panels of PANEL_COLUMNS vectors: the projections of a panel on all earlier vectors in two passes over those (one for
    // the dots, one for the updates), then the panel's own vectors one by one.  Vector i still gets i projections, subtracted in
    // the order 0 .. i-1; the ones on the earlier vectors of its own panel are taken from the vector as the first pass left it
    // (classical Gram-Schmidt takes all of them from the original vector: the same in exact arithmetic, differences of the order
    // of the rounding of the dots).  A quarter of the vector reads of the column-by-column form (DDAMG_TV_GS_COLUMNWISE).
    const bool columnwise = knobs_.tv_gs_columnwise;
    const int CBp = columnwise ? 1 : PANEL_COLUMNS;
    for (int i0 = 0; i0 < lv.nvec; i0 += CBp) {
      const int nb = std::min(CBp, lv.nvec - i0);
      if (i0 > 0 && !columnwise) vec_panel_project<T>(test_vector(l, i0), stride, nb, tv_base(l), stride, i0, all, lv.rw, st_);
      for (int c = 0; c < nb; c++) {
        const int i = i0 + c, first = columnwise ? 0 : i0;
        T* vi = test_vector(l, i);
        if (i > first) {
          vec_multi_dot<T>(test_vector(l, first), stride, i - first, vi, all, lv.rw, lv.rw.d_result, st_);
          vec_multi_axpy_dev<T>(vi, test_vector(l, first), stride, i - first, lv.rw.d_result, -1.0, all, st_);
        }
        vec_scale<T>(vi, vi, 1.0 / norm_of(l, vi), 0.0, all, st_);
      }
    }
    tb = tick("test-vector Gram-Schmidt", tb);
    if (l == 0 && bootstrap_vcycles_batched()) {
      tick("bootstrap V-cycles", tb);
      re_setup(l);
      if (!lv_[1]->coarsest)
        bootstrap(1, std::max(1, (int)std::lround((double)((j + 1) * par_.setup_iter[1]) / (double)iters)));
      continue;
    }
    bool level_batched = false;
    if constexpr (sizeof(T) == 4) {
      if (l >= 1 && (par_.kcycle || lv_[l + 1]->coarsest) && multi_ready(l, lv.nvec)) {
        // the V-cycles of all test vectors of an intermediate level at once (coarse_multi.h); above another intermediate level
        // with that level's K-cycles inside (kcycle = 0: one vector at a time there), and its test vectors updated from their iterates
        CoarseMulti& m = multi_[l];
        float2 *E = m.work(0), *Phi = m.work(1);
        m.gather(E, tv_base(l), tv_stride(l), lv.nvec);
        multi_vcycle(l, Phi, E, lv.nvec);
        multi_update_deeper(l, lv.nvec);
        m.normalize_columns(Phi);
        m.scatter(tv_base(l), tv_stride(l), Phi, lv.nvec);
        level_batched = true;
      }
    }
    for (int i = 0; i < lv.nvec && !level_batched; i++) {
      T* out = l == 0 ? lv.buf[2] : lv.gm.x;   // the reference writes into l->p_PRECISION.x
      vcycle(l, out, nullptr, test_vector(l, i), NO_RES);
      // test_vector_PRECISION_update: deeper intermediate levels first, from their K-cycle iterate
      for (int d = num_levels() - 2; d > l; d--) {
        MGLevel<T>& dl = *lv_[d];
        if (i < dl.nvec) vec_scale<T>(test_vector(d, i), dl.gm.x, 1.0 / norm_of(d, dl.gm.x), 0.0, whole(dl.nel), st_);
      }
      vec_scale<T>(test_vector(l, i), out, 1.0 / norm_of(l, out), 0.0, all, st_);
    }
    tick(l == 0 ? "bootstrap V-cycles" : "bootstrap V-cycles, coarse levels", tb);
    re_setup(l);
    if (l == 0 && !lv_[1]->coarsest)
      bootstrap(1, std::max(1, (int)std::lround((double)((j + 1) * par_.setup_iter[1]) / (double)iters)));
  }
  if (l > 0 && !lv_[l + 1]->coarsest)
    bootstrap(l + 1, std::max(1, (int)std::lround((double)(par_.setup_iter[l + 1] * iters) / (double)par_.setup_iter[l])));
}

template <typename T>
void Multigrid<T>::iterative_setup(int iters) {
  if (iters <= 0) return;
  const SetupStorage fp32_storage(*this);
  set_kcycle_tol(par_.coarse_tol);   // src/setup_generic.c:447-449
  bootstrap(0, iters);
  set_kcycle_tol(par_.kcycle_tol);
}

template <typename T>
void Multigrid<T>::operator_changed() {
  for (int l = 0; l + 1 < num_levels(); l++) build_coarse_operator(l);
}

// shift_update (src/dirac.c:646-668) on the hierarchy.  The reference re-runs its Galerkin construction on every level
// (operator_updates_PRECISION, src/dirac_generic.c:465-501); with P^H P = 1 that is D_c + diff on every level, which is what
// is done here without touching P: diagonal kernels and the inverses of the self couplings where a solver reads them.
template <typename T>
void Multigrid<T>::mass_shifted(double diff) {
  if (!p_orthonormal_) {
    // interpolation vectors imported as they are: P^H (D + d) P is not D_c + d -- the reference's way, the Galerkin construction
    operator_changed();
    return;
  }
  for (int l = 1; l < num_levels(); l++) {
    MGLevel<T>& lv = *lv_[l];
    lv.cop.shift_diagonal(diff, st_);
    if (lv.coarsest || par_.method == 4) lv.cop.compute_self_inverse(st_);
    if (lv.coarsest && gath_.on) { gath_.cop.shift_diagonal(diff, st_); gath_.cop.compute_self_inverse(st_); }
  }
}

template <typename T>
void Multigrid<T>::import_test_vectors(const double* tv_lex_host) {
  MGLevel<T>& lv = *lv_[0];
  for (int k = 0; k < lv.nvec; k++) {
    DDAMG_HIP_CHECK(hipMemcpyAsync(d_stage_, tv_lex_host + (size_t)k * lv.nel, sizeof(double) * lv.nel, hipMemcpyHostToDevice, st_));
    vec_from_lex<T>(lv.fip.test_vector(k), d_stage_, d_lex0_, lv.g->V, 12, st_);
    DDAMG_HIP_CHECK(hipStreamSynchronize(st_));
  }
  re_setup(0);
}

template <typename T>
void Multigrid<T>::import_interpolation(const double* P_lex_host) {
  MGLevel<T>& lv = *lv_[0];
  for (int k = 0; k < lv.nvec; k++) {
    DDAMG_HIP_CHECK(hipMemcpyAsync(d_stage_, P_lex_host + (size_t)k * lv.nel, sizeof(double) * lv.nel, hipMemcpyHostToDevice, st_));
    vec_from_lex<T>(lv.buf[0], d_stage_, d_lex0_, lv.g->V, 12, st_);
    lv.fip.set_column(k, lv.buf[0], st_);       // P is stored aggregate by aggregate (transfer.hip)
    DDAMG_HIP_CHECK(hipStreamSynchronize(st_));
  }
  p_orthonormal_ = false;  // "as they are": the caller's vectors need not be orthonormal on the aggregates
  build_coarse_operator(0);
  initial_setup_from(1);   // deeper levels get their own initial setup on the new level-1 operator
}

template <typename T>
void Multigrid<T>::import_interpolation_level(int l, const double* P_lex_host) {
  if (l == 0) { import_interpolation(P_lex_host); return; }
  MGLevel<T>& lv = *lv_[l];
  DDAMG_REQUIRE(l > 0 && l + 1 < num_levels(), "import_interpolation_level: the level has no coarser level below it");
  {
    DeviceBuffer<int> d_lex;
    d_lex.upload(lv.g->lex_of_site);
    for (int k = 0; k < lv.nvec; k++) {
      DDAMG_HIP_CHECK(hipMemcpyAsync(d_stage_, P_lex_host + (size_t)k * lv.nel, sizeof(double) * lv.nel, hipMemcpyHostToDevice, st_));
      aos_from_lex<T>(lv.cip.interp_vector(k), d_stage_, d_lex, lv.g->V, lv.n, st_);
      aos_from_lex<T>(lv.cip.test_vector(k), d_stage_, d_lex, lv.g->V, lv.n, st_);
      DDAMG_HIP_CHECK(hipStreamSynchronize(st_));
    }
  }
  p_orthonormal_ = false;
  build_coarse_operator(l);
  initial_setup_from(l + 1);
}

template class Multigrid<float>;
template class Multigrid<double>;

}  // namespace ddamg
