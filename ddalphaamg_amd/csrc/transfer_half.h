// transfer_half.h -- the fine level's interpolation operator in 16-bit storage for the solve (opt-in:
// ddamg_hip_set_transfer_storage / DDAMG_TRANSFER_HALF; fp32 V-cycle).
//
// Restriction and interpolation on the fine level stream P once per call (Nvec * 96 B per site in fp32 against 96 B of
// spinor) and are applied only inside the preconditioner of an outer iteration that measures its own residual in fp64; the
// columns of P are orthonormal per aggregate and chirality, so no entry exceeds 1 within a block of norm 1: P can carry fewer
// bits.  TransferHalf is a second copy of Interpolation<float>::P that follows the operator through Interpolation::version():
// setup, setup_update, set_test_vectors and set_interpolation need no hook.  Vectors stay fp32; products accumulate in fp32.
// The transfers of the intermediate levels (CoarseTransfer) and every many-vector path stay fp32.
//
// Element format: __half(value / s), s = s[a][j][h] (fp32) the largest |re| or |im| of the block (aggregate a, vector j,
// chirality h: 6 complex numbers on each site of the aggregate), so every block uses the full fp16 range.  A block of zeros
// has s = 0 and zero entries.  The restriction multiplies its finished sum (a, h, j) by s, the interpolation the coarse
// coefficient (a, h, j) when it is put into LDS: the scales cost nothing per element.
//
// Layout: aggregate by aggregate and contiguous per aggregate like the fp32 P (p_block in transfer.hip) --
// [aggregate][vector][row r of 3][site of the aggregate][8 halves] -- row r of a site vector holding its reals 8r .. 8r+7
// (complex dof 4r .. 4r+3; chirality 0 is rows 0 and the first half of row 1, chirality 1 the rest), so a lane reads a site
// vector of P as three 16-byte loads and a wavefront 1 KiB per load, where the fp32 P takes six.  Scales: [aggregate][vector][2].
// The copy is exactly half the fp32 bytes of P plus 8 bytes of scales per (aggregate, vector); no padding.
#pragma once
#include "common.h"
#include "transfer.h"
#include <hip/hip_fp16.h>

namespace ddamg {

class TransferHalf {
 public:
  // Interpolation<float>::restrict_to / interpolate on the 16-bit copy of ip.P.  The copy is made at the first call and
  // refreshed when ip.version() has moved since the last one.
  void restrict_to(const Interpolation<float>& ip, float* phi_c, const float* phi, hipStream_t st);
  void interpolate(const Interpolation<float>& ip, float* phi, const float* phi_c, bool add, hipStream_t st);
  void release();   // frees the copy (the caller has waited for the stream)
  bool allocated() const { return P_ != nullptr; }

 private:
  DeviceBuffer<__half> P_;       // [num_aggs][nvec][3][agg_sites][8]
  DeviceBuffer<float> scale_;    // [num_aggs][nvec][2]
  const Interpolation<float>* src_ = nullptr;   // the operator the copy belongs to
  unsigned version_ = 0;
  bool valid_ = false;
  void refresh(const Interpolation<float>& ip, hipStream_t st);
};

}  // namespace ddamg
