// blas_driver.hip -- host program that runs ONE operation of blas.h / krylov.h / coarse_lockstep.h (the batch BLAS) on inputs a test wrote, and writes what came out.
//
//   blas_driver <dir>
//
// <dir>/case.txt holds "key value" lines (op, type, the view, counts, strides, scalars); the arrays are raw little-endian files
// <dir>/<name>.bin of the case's type (double where blas.h says double).  Results go to <dir>/out_<name>.bin.  The driver checks
// no result: tests/native_driver.py starts it and the tests compare.  It only refuses a case whose view or strides would address
// outside the arrays it was given (a malformed case must not turn into a stray access).  A std::runtime_error of the library
// ends it with status 2 and the exception text on stderr.
#include "blas.h"
#include "krylov.h"
#include "coarse_lockstep.h"
#include "driver_case.h"

using namespace ddamg;

static View view_of(const Case& c) { return View{(int)c.i("rows"), (size_t)c.i("stride"), (size_t)c.i("off"), (size_t)c.i("len")}; }

// one past the last real the view touches
static size_t view_end(const View& v) { return v.total() == 0 ? 0 : v.off + (size_t)(v.rows - 1) * v.stride + v.len; }
static void sync(hipStream_t st) { DDAMG_HIP_CHECK(hipStreamSynchronize(st)); }
static void fill_nan(double* d, size_t n) { DDAMG_HIP_CHECK(hipMemset(d, 0xFF, sizeof(double) * n)); DDAMG_HIP_CHECK(hipDeviceSynchronize()); }

// ---- elementwise operations -----------------------------------------------------------------------------------------------
template <typename T>
static void run_ew(const Case& c, hipStream_t st) {
  const std::string f = c.str("ew");
  View v;
  if (c.has("site_range")) {   // "site_range 1" with nreal, V, s0, s1: the view comes from site_range<T>, and is reported
    v = site_range<T>((int)c.i("nreal"), (size_t)c.i("V"), (size_t)c.i("s0"), (size_t)c.i("s1"));
    const long long vv[4] = {v.rows, (long long)v.stride, (long long)v.off, (long long)v.len};
    c.write("view", vv, 4);
  } else {
    v = view_of(c);
  }
  const bool inplace = c.i("inplace", 0) != 0;
  Dev<T> z, x, y;
  Dev<double> sc;
  z.load(c, "z");
  need(view_end(v) <= z.n, "view exceeds z");
  const bool needs_x = f != "zero", needs_y = f == "axpy" || f == "minus" || f == "plus";
  if (needs_x && !inplace) { x.load(c, "x"); need(view_end(v) <= x.n, "view exceeds x"); }
  if (needs_y) { y.load(c, "y"); need(view_end(v) <= y.n, "view exceeds y"); }
  const T* xp = inplace ? (const T*)z.p : (const T*)x.p;
  const double are = c.d("are", 0), aim = c.d("aim", 0);
  if (f == "zero") vec_zero<T>(z.p, v, st);
  else if (f == "copy") vec_copy<T>(z.p, xp, v, st);
  else if (f == "scale") vec_scale<T>(z.p, xp, are, aim, v, st);
  else if (f == "minus") vec_minus<T>(z.p, xp, y.p, v, st);
  else if (f == "plus") vec_plus<T>(z.p, xp, y.p, v, st);
  else if (f == "axpy") vec_axpy<T>(z.p, xp, y.p, are, aim, v, st);
  else if (f == "scale_inv") {
    sc.from(std::vector<double>{c.d("scalar")});
    vec_scale_inv_dev<T>(z.p, xp, sc.p, v, st);
  } else need(false, "unknown elementwise operation " + f);
  sync(st);
  z.store(c, "z");
}

// ---- reductions: each runs twice, both results are written ----------------------------------------------------------------
template <typename T>
static void run_reduce(const Case& c, hipStream_t st) {
  const std::string op = c.str("op");
  const View v = view_of(c);
  ReduceWork rw;
  rw.init((int)c.i("max_m", 12));
  Dev<T> x, y;
  x.load(c, "x");
  const int m = (int)c.i("m", 1);
  const size_t xstride = (size_t)c.i("xstride", 0);
  int nres = 1;
  if (op == "norm") need(view_end(v) <= x.n, "view exceeds x");
  else {
    y.load(c, "y");
    need(view_end(v) <= y.n, "view exceeds y");
    if (op == "dot_norm2") { need(view_end(v) <= x.n, "view exceeds x"); nres = 3; }
    else { need(m < 1 || (size_t)(m - 1) * xstride + view_end(v) <= x.n, "vectors exceed x"); nres = 2 * std::max(m, 1); }
  }
  std::vector<double> res(2 * (size_t)nres);
  for (int rep = 0; rep < 2; rep++) {
    fill_nan(rw.d_result, 2 * rw.max_m + 8);
    fill_nan(rw.d_partial, rw.d_partial.size());
    if (op == "norm") vec_norm<T>(x.p, v, rw, rw.d_result, st);
    else if (op == "dot_norm2") vec_dot_and_norm2<T>(x.p, y.p, v, rw, rw.d_result, st);
    else vec_multi_dot<T>(x.p, xstride, m, y.p, v, rw, rw.d_result, st);
    sync(st);
    DDAMG_HIP_CHECK(hipMemcpy(res.data() + (size_t)rep * nres, rw.d_result, sizeof(double) * nres, hipMemcpyDeviceToHost));
  }
  c.write("res", res.data(), res.size());
}

template <typename T>
static void run_multi_axpy(const Case& c, hipStream_t st) {
  const View v = view_of(c);
  const int m = (int)c.i("m");
  const size_t xstride = (size_t)c.i("xstride");
  Dev<T> w, X;
  Dev<double> coef;
  w.load(c, "w"); X.load(c, "X"); coef.load(c, "coef");
  need(view_end(v) <= w.n && (size_t)(m - 1) * xstride + view_end(v) <= X.n && coef.n >= (size_t)2 * m, "arrays too short");
  vec_multi_axpy_dev<T>(w.p, X.p, xstride, m, coef.p, c.d("sign"), v, st);
  sync(st);
  w.store(c, "w");
}

template <typename T>
static void run_panel(const Case& c, hipStream_t st) {
  const View v = view_of(c);
  const int m = (int)c.i("m"), nb = (int)c.i("nb");
  const size_t xstride = (size_t)c.i("xstride"), wstride = (size_t)c.i("wstride");
  ReduceWork rw;
  rw.init((int)c.i("max_m"));
  std::vector<T> hW = c.read<T>("W");
  Dev<T> W, X;
  X.load(c, "X");
  need(nb < 1 || (size_t)(nb - 1) * wstride + view_end(v) <= hW.size(), "panel exceeds W");
  need(m < 1 || (size_t)(m - 1) * xstride + view_end(v) <= X.n, "vectors exceed X");
  const bool second_w = c.i("second_w", 1) != 0;
  const int ncoef = 2 * std::max(m, 1) * PANEL_COLUMNS;
  std::vector<double> coef(2 * (size_t)ncoef);
  for (int rep = 0; rep < 2; rep++) {
    W.from(hW);
    fill_nan(rw.d_result, 2 * rw.max_m + 8);
    fill_nan(rw.d_partial, rw.d_partial.size());
    vec_panel_project<T>(W.p, wstride, nb, X.p, xstride, m, v, rw, st);
    sync(st);
    DDAMG_HIP_CHECK(hipMemcpy(coef.data() + (size_t)rep * ncoef, rw.d_result, sizeof(double) * ncoef, hipMemcpyDeviceToHost));
    if (rep == 0) W.store(c, "W");
    else if (second_w) W.store(c, "W2");
  }
  c.write("coef", coef.data(), coef.size());
}

// ---- operations that do not depend on the case's type -----------------------------------------------------------------------
static void run_arnoldi_norm(const Case& c, hipStream_t st) {
  Dev<double> h;
  h.load(c, "h");
  const int m = (int)c.i("m");
  need(h.n >= (size_t)2 * m + 2, "h too short");
  arnoldi_norm_from_dots(h.p, m, st);
  sync(st);
  h.store(c, "h");
}

static void run_convert(const Case& c, hipStream_t st) {
  const size_t V = (size_t)c.i("V");
  const int nreal = (int)c.i("nreal");
  const size_t n = V * (size_t)nreal;
  if (c.str("to") == "double") {
    Dev<float> x; Dev<double> y;
    x.load(c, "x"); y.load(c, "y");
    need(x.n >= n && y.n >= n, "arrays too short");
    vec_convert<double, float>(y.p, x.p, V, nreal, st);
    sync(st);
    y.store(c, "y");
  } else {
    Dev<double> x; Dev<float> y;
    x.load(c, "x"); y.load(c, "y");
    need(x.n >= n && y.n >= n, "arrays too short");
    vec_convert<float, double>(y.p, x.p, V, nreal, st);
    sync(st);
    y.store(c, "y");
  }
}

static void run_axpy_f32basis(const Case& c, hipStream_t st) {
  const size_t V = (size_t)c.i("V"), xstride = (size_t)c.i("xstride");
  const int nreal = (int)c.i("nreal"), m = (int)c.i("m");
  Dev<double> w, coef; Dev<float> X;
  w.load(c, "w"); X.load(c, "X"); coef.load(c, "coef");
  need(w.n >= V * nreal && (size_t)(m - 1) * xstride + V * nreal <= X.n && coef.n >= (size_t)2 * m, "arrays too short");
  vec_multi_axpy_f32basis(w.p, X.p, xstride, m, coef.p, c.d("sign"), V, nreal, st);
  sync(st);
  w.store(c, "w");
}

template <typename T>
static void run_random(const Case& c, hipStream_t st) {
  Dev<T> x;
  x.from(std::vector<T>((size_t)c.i("n"), (T)7));
  vec_random<T>(x.p, x.n, c.u("seed"), c.u("stream"), st);
  sync(st);
  x.store(c, "x");
}

// three rounds of publish_to_host / wait_published (values, the sequence number the host saw and the one it expected), then
// upload_coefficients
static void run_pinned(const Case& c, hipStream_t st) {
  ReduceWork rw;
  rw.init((int)c.i("max_m"));
  const int n = (int)c.i("n"), rounds = 3;
  need(n <= 2 * rw.max_m + 8, "n exceeds the result slots");
  const std::vector<double> src = c.read<double>("src");
  need(src.size() >= (size_t)rounds * n, "src too short");
  Dev<double> d;
  d.from(src);
  std::vector<double> got((size_t)rounds * n);
  std::vector<unsigned long long> seq(2 * rounds);
  for (int r = 0; r < rounds; r++) {
    publish_to_host(d.p + (size_t)r * n, n, rw, st);
    wait_published(rw, st);
    for (int k = 0; k < n; k++) got[(size_t)r * n + k] = rw.h_result[k];
    seq[2 * r] = *rw.h_seq; seq[2 * r + 1] = rw.seq;
  }
  c.write("pub", got.data(), got.size());
  c.write("seq", seq.data(), seq.size());
  const std::vector<double> hc = c.read<double>("hcoef");
  need(hc.size() <= (size_t)2 * rw.max_m + 8, "hcoef exceeds the coefficient slots");
  fill_nan(rw.d_coef, 2 * rw.max_m + 8);
  for (size_t k = 0; k < hc.size(); k++) rw.h_coef[k] = hc[k];
  upload_coefficients(rw, (int)hc.size(), st);
  sync(st);
  std::vector<double> dc(2 * rw.max_m + 8);
  DDAMG_HIP_CHECK(hipMemcpy(dc.data(), rw.d_coef, sizeof(double) * dc.size(), hipMemcpyDeviceToHost));
  c.write("dcoef", dc.data(), dc.size());
}

// ---- GMRES on  (A z)_k = d_k z_k + a z_{k+1} + b z_{k-1}  (cyclic) ----------------------------------------------------------
//   d_k = 3 + ((7k) mod 11)/11 + i (((5k) mod 13)/13 - 0.5),  a = 0.4 - 0.3i,  b = -0.2 + 0.5i   (a = b = 0 with diag_only)
// The vector is n complex numbers, (re, im) interleaved.  `perm`: the input lives in the float chunk layout of a field with 4
// reals per site and n/2 sites while k counts in the double layout (vec_convert's permutation): complex k = e*V + s of the
// double layout is complex 2s + e of the float layout.
struct Stencil { double are, aim, bre, bim; };
__device__ __forceinline__ void diag_of(size_t k, double& dre, double& dim) {
  dre = 3.0 + (double)((7 * k) % 11) / 11.0;
  dim = (double)((5 * k) % 13) / 13.0 - 0.5;
}
__device__ __forceinline__ size_t float_slot(size_t k, size_t n, bool perm) {
  if (!perm) return k;
  const size_t V = n / 2, e = k / V, s = k - e * V;
  return 2 * s + e;
}
template <typename TO, typename TI>
__global__ __launch_bounds__(256) void stencil_kernel(TO* __restrict__ out, const TI* __restrict__ in, size_t n, Stencil s, bool perm) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const size_t kp = float_slot(k + 1 == n ? 0 : k + 1, n, perm), km = float_slot(k == 0 ? n - 1 : k - 1, n, perm), k0 = float_slot(k, n, perm);
  double dre, dim;
  diag_of(k, dre, dim);
  const TO zr = in[2 * k0], zi = in[2 * k0 + 1], pr = in[2 * kp], pi = in[2 * kp + 1], mr = in[2 * km], mi = in[2 * km + 1];
  const TO dr = (TO)dre, di = (TO)dim, ar = (TO)s.are, ai = (TO)s.aim, br = (TO)s.bre, bi = (TO)s.bim;
  out[2 * k]     = dr * zr - di * zi + ar * pr - ai * pi + br * mr - bi * mi;
  out[2 * k + 1] = dr * zi + di * zr + ar * pi + ai * pr + br * mi + bi * mr;
}
// z = v / d * f, written to the float slot where `perm`
template <typename TO, typename TI>
__global__ __launch_bounds__(256) void jacobi_kernel(TO* __restrict__ z, const TI* __restrict__ v, size_t n, double f, bool perm) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  double dre, dim;
  diag_of(k, dre, dim);
  const double vr = v[2 * k], vi = v[2 * k + 1], den = dre * dre + dim * dim;
  const size_t o = float_slot(k, n, perm);
  z[2 * o]     = (TO)((vr * dre + vi * dim) / den * f);
  z[2 * o + 1] = (TO)((vi * dre - vr * dim) / den * f);
}

template <typename T>
static void run_gmres(const Case& c, hipStream_t st) {
  const size_t n = (size_t)c.i("n");
  need(n >= 2 && (2 * n) % 4 == 0, "n must be even");
  const std::string form = c.str("form"), prec = c.str("prec");
  const bool diag_only = c.i("diag_only", 0) != 0, z32 = c.i("z_fp32", 0) != 0;
  const Stencil sten = diag_only ? Stencil{0, 0, 0, 0} : Stencil{0.4, -0.3, -0.2, 0.5};
  const unsigned grid = (unsigned)((n + 255) / 256);
  ReduceWork rw;
  Gmres<T> g;
  g.restart_length = (int)c.i("restart");
  rw.init(g.restart_length + 2);
  g.num_restart = (int)c.i("num_restart");
  g.tol = c.d("tol");
  g.initial_guess_zero = c.i("guess", 0) == 0;
  g.view = whole(2 * n);
  g.st = st; g.rw = &rw;
  g.track_history = true;
  g.single_allreduce = form == "single";
  g.pipelined = form == "pipelined";
  need(g.single_allreduce || g.pipelined || form == "classical", "unknown Arnoldi form " + form);
  g.z_fp32 = z32;
  g.alloc(2 * n, g.restart_length, g.pipelined || prec != "none");
  size_t history_at_cycle_start = 0;   // a cycle that does not start from a zero guess begins with the residual b - A x
  g.op = [&](T* out, const T* in) {
    if (in == g.x) history_at_cycle_start = g.history.size();
    hipLaunchKernelGGL((stencil_kernel<T, T>), dim3(grid), dim3(256), 0, st, out, in, n, sten, false);
    DDAMG_HIP_CHECK(hipGetLastError());
  };
  int calls = 0;
  if (prec == "jacobi" && !z32) {
    g.prec = [&](T* phi, T*, const T* eta, int) {
      hipLaunchKernelGGL((jacobi_kernel<T, T>), dim3(grid), dim3(256), 0, st, phi, eta, n, 1.0 + 0.1 * (calls++ % 3), false);
      DDAMG_HIP_CHECK(hipGetLastError());
    };
  } else if (prec == "jacobi") {
    need(sizeof(T) == 8, "fp32 iterates belong to Gmres<double>");
    g.sites32 = n / 2; g.nreal32 = 4;
    g.prec32 = [&](float* z, const T* v, int) {
      hipLaunchKernelGGL((jacobi_kernel<float, T>), dim3(grid), dim3(256), 0, st, z, v, n, 1.0 + 0.1 * (calls++ % 3), true);
      DDAMG_HIP_CHECK(hipGetLastError());
    };
    g.op32 = [&](T* out, const float* z) {
      hipLaunchKernelGGL((stencil_kernel<T, float>), dim3(grid), dim3(256), 0, st, out, z, n, sten, true);
      DDAMG_HIP_CHECK(hipGetLastError());
    };
  } else need(prec == "none", "unknown preconditioner " + prec);

  const std::vector<T> b = c.read<T>("b");
  need(b.size() == 2 * n, "b has the wrong length");
  DDAMG_HIP_CHECK(hipMemcpy(g.b, b.data(), sizeof(T) * 2 * n, hipMemcpyHostToDevice));
  if (!g.initial_guess_zero) {
    const std::vector<T> x0 = c.read<T>("x0");
    need(x0.size() == 2 * n, "x0 has the wrong length");
    DDAMG_HIP_CHECK(hipMemcpy(g.x, x0.data(), sizeof(T) * 2 * n, hipMemcpyHostToDevice));
  }
  const int iter = g.solve();
  sync(st);
  // the basis before true_residual() overwrites w and r (it does not touch the basis, but keep the order plain)
  std::vector<T> x(2 * n), Vb(g.vstride * (size_t)(g.restart_length + 1));
  DDAMG_HIP_CHECK(hipMemcpy(x.data(), g.x, sizeof(T) * x.size(), hipMemcpyDeviceToHost));
  DDAMG_HIP_CHECK(hipMemcpy(Vb.data(), g.Vb, sizeof(T) * Vb.size(), hipMemcpyDeviceToHost));
  const double gamma = g.gamma_jp1, norm_r0 = g.norm_r0;
  const double last_cycle_steps = (double)(g.history.size() - history_at_cycle_start);   // completed steps of the last cycle
  const double tr = norm_r0 > 0 ? g.true_residual() : 0.0;
  const double sc[7] = {(double)iter, gamma, norm_r0, tr, (double)g.history.size(), (double)g.vstride, last_cycle_steps};
  c.write("scalars", sc, 7);
  c.write("history", g.history.data(), g.history.size());
  c.write("x", x.data(), x.size());
  c.write("Vb", Vb.data(), Vb.size());
}

// ---- BLAS-1 on batches [row][32 columns], every column with its own coefficient (coarse_lockstep.h); fp32 only -----------------
// Arrays are files of float (two per complex number) or double; strides and counts are in the units of the library's interface:
// sstride / dstride in floats, vstride, rows and elems in complex numbers.
template <typename U> static void fill_ff(U* d, size_t n) { DDAMG_HIP_CHECK(hipMemset(d, 0xFF, sizeof(U) * (n ? n : 1))); DDAMG_HIP_CHECK(hipDeviceSynchronize()); }
static const float2* c2(const Dev<float>& a) { return reinterpret_cast<const float2*>((const float*)a.p); }
static float2* c2(Dev<float>& a) { return reinterpret_cast<float2*>((float*)a.p); }

static void run_batch_gather(const Case& c, hipStream_t st) {
  const size_t rows = (size_t)c.i("rows"), sstride = (size_t)c.i("sstride");
  const int ncols = (int)c.i("ncols");
  Dev<float> Wb, src;
  Wb.load(c, "Wb"); src.load(c, "src");
  need(ncols >= 0 && ncols <= LOCKSTEP_COLS && rows >= 1, "0 <= ncols <= 32, rows >= 1");
  need(ncols == 0 || (size_t)(ncols - 1) * sstride + 2 * rows <= src.n, "columns exceed src");
  need(2 * rows * LOCKSTEP_COLS <= Wb.n, "batch exceeds Wb");
  batch_gather(c2(Wb), src.p, sstride, ncols, rows, st);
  sync(st);
  Wb.store(c, "Wb");
}

static void run_batch_scatter(const Case& c, hipStream_t st) {
  const size_t rows = (size_t)c.i("rows"), dstride = (size_t)c.i("dstride");
  const int ncols = (int)c.i("ncols");
  Dev<float> Wb, dst;
  Wb.load(c, "Wb"); dst.load(c, "dst");
  need(ncols >= 0 && ncols <= LOCKSTEP_COLS && rows >= 1, "0 <= ncols <= 32, rows >= 1");
  need(ncols == 0 || (size_t)(ncols - 1) * dstride + 2 * rows <= dst.n, "columns exceed dst");
  need(2 * rows * LOCKSTEP_COLS <= Wb.n, "batch exceeds Wb");
  batch_scatter(dst.p, dstride, c2(Wb), ncols, rows, st);
  sync(st);
  dst.store(c, "dst");
}

// runs twice; res holds both results, each (m + extra) * 32 complex numbers of which the call may write the first m * 32
static void run_batch_dots(const Case& c, hipStream_t st) {
  const size_t rows = (size_t)c.i("rows"), vstride = (size_t)c.i("vstride");
  const int m = (int)c.i("m"), extra = (int)c.i("extra", 1);
  Dev<float> basis, w;
  basis.load(c, "basis"); w.load(c, "w");
  need(m >= 1 && extra >= 0 && rows >= 1, "m >= 1, extra >= 0, rows >= 1");
  need(2 * ((size_t)(m - 1) * vstride + rows * LOCKSTEP_COLS) <= basis.n, "vectors exceed basis");
  need(2 * rows * LOCKSTEP_COLS <= w.n, "batch exceeds w");
  const size_t nres = (size_t)2 * (m + extra) * LOCKSTEP_COLS, nws = batch_dots_workspace();
  DeviceBuffer<double> d_out, d_partial;
  d_out.alloc(nres); d_partial.alloc(nws);
  std::vector<double> res(2 * nres);
  for (int rep = 0; rep < 2; rep++) {
    fill_ff<double>(d_out, nres);
    fill_ff<double>(d_partial, nws);
    batch_dots(c2(basis), vstride, m, c2(w), rows, d_partial, d_out, st);
    sync(st);
    DDAMG_HIP_CHECK(hipMemcpy(res.data() + (size_t)rep * nres, d_out, sizeof(double) * nres, hipMemcpyDeviceToHost));
  }
  c.write("res", res.data(), res.size());
}

static void run_batch_axpy(const Case& c, hipStream_t st) {
  const size_t elems = (size_t)c.i("elems"), vstride = (size_t)c.i("vstride");
  const int m = (int)c.i("m");
  Dev<float> w, basis;
  Dev<double> coef;
  w.load(c, "w"); basis.load(c, "basis"); coef.load(c, "coef");
  need(m >= 1 && elems >= 1, "m >= 1, elems >= 1");
  need(2 * elems <= w.n && 2 * ((size_t)(m - 1) * vstride + elems) <= basis.n && coef.n >= (size_t)2 * m * LOCKSTEP_COLS, "arrays too short");
  batch_axpy(c2(w), c2(basis), vstride, m, coef.p, c.d("sign"), elems, st);
  sync(st);
  w.store(c, "w");
}

static void run_batch_scale_inv(const Case& c, hipStream_t st) {
  const size_t elems = (size_t)c.i("elems");
  Dev<float> w, out;
  Dev<double> n2;
  w.load(c, "w"); n2.load(c, "n2");
  need(elems >= 1 && 2 * elems <= w.n && n2.n >= (size_t)2 * LOCKSTEP_COLS, "arrays too short");
  out.from(std::vector<float>(w.n, 0.f));
  fill_ff<float>(out.p, out.n);
  batch_scale_inv(c2(out), c2(w), n2.p, elems, st);
  sync(st);
  out.store(c, "out");
}

template <typename T>
static void run_typed(const Case& c, const std::string& op, hipStream_t st) {
  if (op == "ew") run_ew<T>(c, st);
  else if (op == "norm" || op == "dot_norm2" || op == "multi_dot") run_reduce<T>(c, st);
  else if (op == "multi_axpy") run_multi_axpy<T>(c, st);
  else if (op == "panel") run_panel<T>(c, st);
  else if (op == "random") run_random<T>(c, st);
  else if (op == "gmres") run_gmres<T>(c, st);
  else need(false, "unknown operation " + op);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: blas_driver <case directory>\n"); return 64; }
  driver_name = "blas_driver";
  try {
    const Case c(argv[1]);
    const std::string op = c.str("op");
    hipStream_t st;
    DDAMG_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (op == "arnoldi_norm") run_arnoldi_norm(c, st);
    else if (op == "convert") run_convert(c, st);
    else if (op == "axpy_f32basis") run_axpy_f32basis(c, st);
    else if (op == "pinned") run_pinned(c, st);
    else if (op == "batch_gather") run_batch_gather(c, st);
    else if (op == "batch_scatter") run_batch_scatter(c, st);
    else if (op == "batch_dots") run_batch_dots(c, st);
    else if (op == "batch_axpy") run_batch_axpy(c, st);
    else if (op == "batch_scale_inv") run_batch_scale_inv(c, st);
    else if (c.str("type") == "float") run_typed<float>(c, op, st);
    else if (c.str("type") == "double") run_typed<double>(c, op, st);
    else need(false, "type must be float or double");
    DDAMG_HIP_CHECK(hipStreamSynchronize(st));
    DDAMG_HIP_CHECK(hipStreamDestroy(st));
  } catch (const std::runtime_error& e) {
    fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  return 0;
}
