// intermediate_refusal.h -- why a context cannot keep the couplings of its intermediate levels in 16 bits
// (ddamg_hip_set_intermediate_storage, coarse_half_level.h).  Plain C++: the entry point and a host-only test share it.
#pragma once

namespace ddamg {

// nullptr: it can.  intermediate_level_decomposed: a level with depth > 0 that is not the coarsest is divided over processes
// (the halo forms of the operator are not covered)
inline const char* intermediate_half_refusal(int num_levels, int method, int mixed_precision, bool intermediate_level_decomposed) {
  if (num_levels < 3) return "16-bit intermediate storage needs a hierarchy with an intermediate level (three levels or more)";
  if (method < 1 || method > 3) return "16-bit intermediate storage is implemented for the Schwarz smoothers (method 1 to 3)";
  if (mixed_precision == 0) return "16-bit intermediate storage needs the fp32 V-cycle (mixed_precision 1 or 2)";
  if (intermediate_level_decomposed) return "16-bit intermediate storage needs every intermediate level on one process";
  return nullptr;
}

}  // namespace ddamg
