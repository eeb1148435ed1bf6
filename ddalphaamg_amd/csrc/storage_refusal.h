// storage_refusal.h -- why a context cannot keep one of its operators in 16 bits (ddamg_hip_set_coarse_storage,
// ddamg_hip_set_transfer_storage, ddamg_hip_set_intermediate_storage; half_storage.h).  nullptr: it can.
// Plain C++: the entry points and a host-only test share it.
#pragma once

namespace ddamg {

// the couplings of the coarsest level (coarse_half.h).  coarsest_decomposed: the coarsest level is divided over processes;
// gather_coarsest: every process then solves on the whole coarsest lattice (ddamg_hip_params::gather_coarsest)
inline const char* coarse_half_refusal(int num_levels, int method, int mixed_precision, int odd_even, bool coarsest_decomposed, bool gather_coarsest) {
  if (num_levels < 2 || method < 1 || method > 4) return "16-bit coarse storage needs a multigrid hierarchy (two levels or more, method 1 to 4)";
  if (mixed_precision == 0) return "16-bit coarse storage needs the fp32 V-cycle (mixed_precision 1 or 2)";
  if (odd_even == 0) return "16-bit coarse storage is implemented for the odd-even coarsest solve (odd_even = 1)";
  if (coarsest_decomposed && !gather_coarsest) return "16-bit coarse storage needs the coarsest level on one process (single process, or gather_coarsest)";
  return nullptr;
}

// the fine level's interpolation operator (transfer_half.h)
inline const char* transfer_half_refusal(int num_levels, int method, int mixed_precision) {
  if (num_levels < 2 || method < 1 || method > 4) return "16-bit transfer storage needs a multigrid hierarchy (two levels or more, method 1 to 4)";
  if (mixed_precision == 0) return "16-bit transfer storage needs the fp32 V-cycle (mixed_precision 1 or 2)";
  return nullptr;
}

// the couplings of the intermediate levels (coarse_half.h).  intermediate_level_decomposed: a level with depth > 0 that is not
// the coarsest is divided over processes (the halo forms of the operator are not covered)
inline const char* intermediate_half_refusal(int num_levels, int method, int mixed_precision, bool intermediate_level_decomposed) {
  if (num_levels < 3) return "16-bit intermediate storage needs a hierarchy with an intermediate level (three levels or more)";
  if (method < 1 || method > 3) return "16-bit intermediate storage is implemented for the Schwarz smoothers (method 1 to 3)";
  if (mixed_precision == 0) return "16-bit intermediate storage needs the fp32 V-cycle (mixed_precision 1 or 2)";
  if (intermediate_level_decomposed) return "16-bit intermediate storage needs every intermediate level on one process";
  return nullptr;
}

}  // namespace ddamg
