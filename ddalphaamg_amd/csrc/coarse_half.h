// coarse_half.h -- the couplings of the coarsest operator in 16-bit storage for the odd-even solve (opt-in:
// ddamg_hip_set_coarse_storage / DDAMG_COARSE_HALF; fp32 V-cycle, coarsest level on one process).
//
// The coarsest-level GMRES is a chain of dense matrix-vector products bound by the read of the couplings (coarse_op.hip), and
// it is solved to coarse_tol inside a preconditioner whose outer iteration measures its residual in fp64: the couplings can
// carry fewer bits.  CoarseHalf is a second copy of CoarseOp<float>'s M[0..4] and Minv that follows the operator through
// version() / inverse_version(), as the A-operand copies of coarse_multi.h do: mass shift, scale_clover, setup_update and
// set_coarse_operator* need no hook.  Vectors stay fp32 and site-major; products accumulate in fp32.
//
// Element format: one __half2 (re, im) / s, s the largest |re| or |im| of the matrix (fp32, one per matrix; a matrix of zeros
// has s = 0 and zero entries), so every matrix uses the full fp16 range whatever its size; s multiplies the finished product.
//
// Layout of a matrix (nt x nt tiles of 8 x 8, padding rows and columns zero, as coarse_op.h): element (i, j), i = a + 8p,
// j = b + 8q, belongs to tile t = p * nt + q and lane l = 8a + b.  Four consecutive tiles form a group in which a lane's four
// elements are adjacent: offset (t / 4) * 256 + 4 l + t % 4 (in __half2), so a wavefront reads a group as ONE 16-byte load
// per lane, 1 KiB contiguous.  nt odd leaves one last tile, stored as coarse_op.h stores it (offset (nt * nt - 1) * 64 + l)
// and read with a 4-byte load: no padding tile, the copy is exactly half the fp32 bytes plus the scales.
#pragma once
#include "common.h"
#include "coarse_op.h"
#include <hip/hip_fp16.h>

namespace ddamg {

struct CoarseHalfDev {
  const __half2* M;      // [V][5][msize]
  const __half2* Minv;   // [V][msize]
  const float* scale;    // [V][6]: M[0..4], Minv
  const int* nb;         // [8][V], the operator's neighbour table
  int V, n;
  size_t msize;          // __half2 per matrix = nt * nt * 64
};

// the copy's build kernel (coarse_half.hip), shared with the intermediate levels (coarse_half_level.h): matrices m0 .. m0 + count - 1
// of every site (0-4 the couplings, 5 the inverted self coupling) from `op` into Mh / Minvh in the layout above, their scales to
// scale[site * 6 + m].  Minvh is read only for m = 5.
void coarse_half_build(__half2* Mh, __half2* Minvh, float* scale, const CoarseOpDev<float>& op, int m0, int count, hipStream_t st);

class CoarseHalf {
 public:
  // the two products of the coarsest Schur complement, with the signature and semantics of CoarseOp::hop / self_mul; `op` is
  // the fp32 operator the copy follows (not decomposed over processes, n <= 64).  The copy is made at the first call and
  // refreshed when the operator has moved since the last one.
  void hop(const CoarseOp<float>& op, float* out, const float* in, int s0, int s1, double sign, bool accumulate, hipStream_t st);
  void self_mul(const CoarseOp<float>& op, float* out, const float* in, int s0, int s1, bool inverse, hipStream_t st);
  void release();   // frees the copy (the caller has waited for the stream)
  bool allocated() const { return M_ != nullptr; }

 private:
  DeviceBuffer<__half2> M_, Minv_;
  DeviceBuffer<float> scale_;
  const CoarseOp<float>* src_ = nullptr;   // the operator the copy belongs to
  unsigned version_ = 0, inverse_version_ = 0;
  bool valid_ = false;
  unsigned hop_count_ = 0;   // every second hopping term walks the level backwards (coarse_op.hip, launch_site)
  CoarseHalfDev refresh(const CoarseOp<float>& op, hipStream_t st);
};

}  // namespace ddamg
