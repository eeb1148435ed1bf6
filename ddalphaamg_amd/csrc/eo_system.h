// eo_system.h -- the even-odd preconditioned system of the fine operator for its users outside the smoothers:
//   Dhat = D_ee - D_eo D_oo^-1 D_oe  on the even sites (the asymmetric form; apply_schur_complement_PRECISION,
//   src/oddeven_generic.c:704-740), Dhat^dagger = gamma5 Dhat gamma5, and  sum_s log|det D_ss|  over the sites of one parity.
// Parity is the global one of FineOpDev::parity (0 even, 1 odd).  Vectors keep their full length (chunked SoA, fine_op.h); a
// half field is [V/2][12] complex fp64 in device memory: the sites of one parity of the process's own lattice in lexicographic
// order, half index = lexicographic index >> 1 (every local extent even: the pair x = 2k, 2k+1 holds one site of each parity).
#pragma once
#include "fine_op.h"
#include "blas.h"

namespace ddamg {

// half field -> the sites of parity `par` of the vector dst (T = float: rounded); zero_other: the sites of the other parity
// become zero, else they are left alone.  gamma5: the signs of vec_from_lex in the same pass.  16-byte accesses on both sides.
template <typename T>
void vec_from_half(T* dst, const double* half_dev, const int* lex_of_site, const unsigned char* parity, int par, bool zero_other, bool gamma5,
                   int V, hipStream_t st);
// the sites of parity `par` of src -> half field; the other parity is not read
template <typename T>
void vec_to_half(double* half_dev, const T* src, const int* lex_of_site, const unsigned char* parity, int par, bool gamma5, int V, hipStream_t st);

// what parity_update does on the sites of parity `par` of x (the others are left alone); gamma5: e times gamma5
enum class ParityOp { Zero /* x = 0 */, Add /* x += e */, MinusAssign /* x = -e */ };
template <typename T>
void parity_update(T* x, const T* e, const unsigned char* parity, int par, ParityOp op, bool gamma5, int V, hipStream_t st);

// workspace of schur_apply: two vectors per precision that was used, owned by the context
struct EoWork {
  DeviceBuffer<float> t32, g32;
  DeviceBuffer<double> t64, g64;
  template <typename T> DeviceBuffer<T>& t();
  template <typename T> DeviceBuffer<T>& g();
};
template <> inline DeviceBuffer<float>& EoWork::t<float>() { return t32; }
template <> inline DeviceBuffer<double>& EoWork::t<double>() { return t64; }
template <> inline DeviceBuffer<float>& EoWork::g<float>() { return g32; }
template <> inline DeviceBuffer<double>& EoWork::g<double>() { return g64; }

// out = Dhat in (dagger: Dhat^dagger in) on the even sites, zero on the odd ones; the odd sites of `in` are not read.  Two
// launches of FineOp::hop with its fused epilogues: t_o = D_oo^-1 H_oe in_e, out_e = D_ee in_e - H_eo t_o.  The dagger form is
// gamma5, that, gamma5 in three more passes (applications are not the hot path of this system, the solves are).  out != in.
template <typename T>
void schur_apply(const FineOp<T>& op, T* out, const T* in, bool dagger, EoWork& w, hipStream_t st);
// t = D_oo^-1 H_oe v_e on the odd sites (dagger: gamma5 v in place of v; the caller puts the outer gamma5 into parity_update):
// the odd part of the full-lattice solution is minus that.  Returns t, which lives in w.
template <typename T>
const T* schur_odd_part(const FineOp<T>& op, const T* v, bool dagger, EoWork& w, hipStream_t st);

// d_out[0] = sum over the sites of parity `par` of log|det D_ss| (both 6x6 blocks), d_out[1] = the number of negative pivots
// (the sign of the product is (-1)^that), d_out[2] = the number of zero or non-finite pivots (an error for the caller), from the
// fp64 clover field (72 reals per site, fine_op.h): 576 bytes per site, read once.  Two-stage deterministic fp64 reduction
// through rw (blas.h), summed over the processes of a grid in one all-reduce of the three numbers.
void clover_logdet(const double* clover64, const unsigned char* parity, int par, int V, ReduceWork& rw, double* d_out, hipStream_t st);

}  // namespace ddamg
