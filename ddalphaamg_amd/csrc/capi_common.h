// capi_common.h -- what the two files of the C-ABI (capi.cpp, solver.cpp) share: the error boundary, the way into an entry
// point, and the dispatch on the precision of the hierarchy and of a vector (docs/design/05_host.md, 5c).
#pragma once
#include "context.h"
#include <string>
#include <type_traits>

extern thread_local std::string g_ddamg_last_error;   // what ddamg_hip_last_error hands out (capi.cpp)

// every entry point is  DDAMG_API_BEGIN  body  DDAMG_API_END : 0, or 1 with the message of what the body threw
#define DDAMG_API_BEGIN try {
#define DDAMG_API_END                                  \
  }                                                    \
  catch (const std::exception& e) {                    \
    g_ddamg_last_error = e.what();                     \
    return 1;                                          \
  }                                                    \
  catch (...) {                                        \
    g_ddamg_last_error = "unknown error";              \
    return 1;                                          \
  }                                                    \
  return 0;

namespace ddamg {

// the first statement of every entry point that touches the device
inline void enter(const ddamg_hip_ctx* c) {
  DDAMG_REQUIRE(c, "null context");
  DDAMG_HIP_CHECK(hipSetDevice(c->device));
}

// f(hierarchy) on the one the context has (fp32 V-cycle where mixed_precision >= 1, fp64 otherwise), and its result;
// `missing` is what the caller says where there is none yet
template <typename F>
auto with_mg(ddamg_hip_ctx* c, F f, const char* missing = "setup has not been run") {
  DDAMG_REQUIRE(c->mg32 || c->mg64, missing);
  if (c->mg32) return f(*c->mg32);
  return f(*c->mg64);
}
// f(hierarchy) on every hierarchy that exists: none is not an error
template <typename F>
void for_each_mg(ddamg_hip_ctx* c, F f) {
  if (c->mg32) f(*c->mg32);
  if (c->mg64) f(*c->mg64);
}
// float or double, inside a generic lambda:  using T = real_of<decltype(mg)>;  using T = pointee<decltype(p)>;
template <typename MG> using real_of = typename std::remove_reference_t<MG>::real;
template <typename P> using pointee = std::remove_pointer_t<P>;

// the reduction workspace of the entry points that reduce outside a Krylov solver
inline ReduceWork& blas_rw(ddamg_hip_ctx* c) {
  if (!c->rw_blas_ready) { c->rw_blas.init(8); c->rw_blas_ready = true; }
  return c->rw_blas;
}

// the even-odd entry points: local and global parity agree, and every pair x = 2k, 2k+1 holds one site of each parity, only where
// every local extent is even
inline void require_even_extents(const ddamg_hip_ctx* c, const char* name) {
  const Geometry& g = c->levels[0]->geom;
  for (int mu = 0; mu < 4; mu++)
    DDAMG_REQUIRE(g.L[mu] % 2 == 0, (std::string(name) + ": the even-odd entry points need even local lattice extents").c_str());
}

template <typename T> T* vec_data(const ddamg_hip_vec* v) { return reinterpret_cast<T*>(v->data.get()); }
inline size_t vec_len(const ddamg_hip_vec* v) { return (size_t)v->V * v->ndof * 2; }   // in reals
// f(float*) or f(double*) on the vector's numbers, by its precision
template <typename F>
auto with_vec(const ddamg_hip_vec* v, F f) {
  if (v->precision == 32) return f(vec_data<float>(v));
  return f(vec_data<double>(v));
}

}  // namespace ddamg
