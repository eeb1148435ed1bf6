// coarse_half.h -- the couplings of a coarse level in 16-bit storage for the solve (opt-in, fp32 V-cycle, level on one process):
// the coarsest level's for the odd-even solve (ddamg_hip_set_coarse_storage / DDAMG_COARSE_HALF), an intermediate level's
// (depth > 0, not the coarsest; methods 1-3) for the K-cycle and the Schwarz smoother (ddamg_hip_set_intermediate_storage /
// DDAMG_INTERMEDIATE_HALF).
//
// The coarsest-level GMRES is a chain of dense matrix-vector products bound by the read of the couplings (coarse_op.hip), and
// it is solved to coarse_tol inside a preconditioner whose outer iteration measures its residual in fp64: the couplings can
// carry fewer bits.  The same holds for the three products of an intermediate level -- the operator of the K-cycle FGMRES, the
// residual updates of the Schwarz smoother and its fused block solver.  CoarseHalf is a second copy of CoarseOp<float>'s
// M[0..4], and of Minv where a product reads it, one object per level, that follows the operator through version() /
// inverse_version(), as the A-operand copies of coarse_multi.h do: mass shift, scale_clover, setup_update and
// set_coarse_operator* need no hook.  Vectors stay fp32 and site-major; products accumulate in fp32.
//
// Element format: one __half2 (re, im) / s, s the largest |re| or |im| of the matrix (fp32, one per matrix; a matrix of zeros
// has s = 0 and zero entries), so every matrix uses the full fp16 range whatever its size; s multiplies the finished product.
// Six scales per site (M[0..4], Minv), the sixth unused while the copy holds no inverse.
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
  const __half2* Minv;   // [V][msize], or nullptr
  const float* scale;    // [V][6]: M[0..4], Minv
  const int* nb;         // [8][V], the operator's neighbour table
  int V, n;
  size_t msize;          // __half2 per matrix = nt * nt * 64
};

// `op` in every product: the fp32 operator of the object's level (always the same one, not decomposed over processes,
// n <= 64).  The copy is made at the first call and refreshed when the operator has moved since the last one.
class CoarseHalf {
 public:
  // the two products of the coarsest Schur complement, with the signature and semantics of CoarseOp::hop / self_mul
  // (coarse_half.hip).  They keep the inverted self coupling as well: six matrices per site.
  void hop(const CoarseOp<float>& op, float* out, const float* in, int s0, int s1, double sign, bool accumulate, hipStream_t st);
  void self_mul(const CoarseOp<float>& op, float* out, const float* in, int s0, int s1, bool inverse, hipStream_t st);
  // the three products of an intermediate level, with the signatures and semantics of CoarseOp::apply / apply_masked /
  // block_minres (coarse_half_level.hip).  No inverse (depth > 0 has no odd-even solve): five matrices per site.
  void apply(const CoarseOp<float>& op, float* out, const float* in, hipStream_t st);
  void apply_masked(const CoarseOp<float>& op, float* out, const float* in, const int* site_list, int nsites, const unsigned char* dir_mask,
                    bool mask_invert, double sign_self, double sign_hop, bool accumulate, hipStream_t st);
  bool block_minres(const CoarseOp<float>& op, float* x, float* r, float* latest, const int* blocks, int nblocks,
                    const CoarseOp<float>::BlockPlan& plan, int iters, double eps, hipStream_t st);
  void release();   // frees the copy (the caller has waited for the stream)
  bool allocated() const { return M_ != nullptr; }

 private:
  DeviceBuffer<__half2> M_, Minv_;
  DeviceBuffer<float> scale_;
  unsigned version_ = 0, inverse_version_ = 0;
  bool valid_ = false;       // M_ holds the operator of version_ (Minv_, where allocated, that of inverse_version_)
  unsigned hop_count_ = 0;   // every second hopping term walks the level backwards (coarse_op.hip, launch_site)
  CoarseHalfDev refresh(const CoarseOp<float>& op, hipStream_t st, bool with_inverse);
};

}  // namespace ddamg
