// coarse_half_level.h -- the couplings of an intermediate level (depth > 0, not the coarsest) in 16-bit storage for the solve
// (opt-in: ddamg_hip_set_intermediate_storage / DDAMG_INTERMEDIATE_HALF; fp32 V-cycle, methods 1-3, level on one process).
//
// The three products of an intermediate level -- the operator of the K-cycle FGMRES, the residual updates of the Schwarz
// smoother and its fused block solver -- stream the couplings and are bound by that read (coarse_op.hip).  CoarseHalfLevel is
// a second copy of CoarseOp<float>'s M[0..4] in the element format and tile-group layout of coarse_half.h, made by the same
// build kernel, with one object per level.  It holds no inverse (depth > 0 has no odd-even solve) and follows the operator
// through version().  Vectors stay fp32 and site-major; products accumulate in fp32; the scale multiplies the finished product.
// The scales keep the stride of coarse_half.h (six per site, the sixth unused) so that the build kernel is the same code.
#pragma once
#include "coarse_half.h"

namespace ddamg {

class CoarseHalfLevel {
 public:
  // the three products with the signatures and semantics of CoarseOp::apply / apply_masked / block_minres; `op` is the fp32
  // operator the copy follows (not decomposed over processes).  The copy is made at the first call and refreshed when the
  // operator has moved since the last one.
  void apply(const CoarseOp<float>& op, float* out, const float* in, hipStream_t st);
  void apply_masked(const CoarseOp<float>& op, float* out, const float* in, const int* site_list, int nsites, const unsigned char* dir_mask,
                    bool mask_invert, double sign_self, double sign_hop, bool accumulate, hipStream_t st);
  bool block_minres(const CoarseOp<float>& op, float* x, float* r, float* latest, const int* blocks, int nblocks,
                    const CoarseOp<float>::BlockPlan& plan, int iters, double eps, hipStream_t st);
  void release();   // frees the copy (the caller has waited for the stream)
  bool allocated() const { return M_ != nullptr; }

 private:
  DeviceBuffer<__half2> M_;      // [V][5][msize]
  DeviceBuffer<float> scale_;    // [V][6]
  const CoarseOp<float>* src_ = nullptr;
  unsigned version_ = 0;
  bool valid_ = false;
  CoarseHalfDev refresh(const CoarseOp<float>& op, hipStream_t st);
};

}  // namespace ddamg
