// half_storage.h -- what the solve may read from a 16-bit copy instead of the fp32 numbers, and the bits that are set for each.
// Plain C++: the context, the hierarchy and the entry points share it.
#pragma once

namespace ddamg {

// Coarse: the couplings of the coarsest level (coarse_half.h, ddamg_hip_set_coarse_storage, DDAMG_COARSE_HALF);
// Transfer: the fine level's interpolation operator (transfer_half.h, ddamg_hip_set_transfer_storage, DDAMG_TRANSFER_HALF);
// Intermediate: the couplings of every level with depth > 0 that is not the coarsest (coarse_half.h,
// ddamg_hip_set_intermediate_storage, DDAMG_INTERMEDIATE_HALF)
enum StorageKind { Coarse, Transfer, Intermediate };

struct StorageBits {
  int bits[3] = {32, 32, 32};   // per StorageKind: 32 or 16 bits per real
};

}  // namespace ddamg
