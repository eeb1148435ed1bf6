// chrono.h -- the streaming kernels of a solve that starts from a guess and of the chronological guess (minimal residual
// extrapolation from past solutions, Brower et al., Nucl. Phys. B 484 (1997) 353).  No counterpart in the reference, which
// starts every solve of its interface from zero.  fp64 vectors addressed by Views (blas.h); m <= CHRONO_MAX columns, column i
// of a family at  base + i * stride; complex coefficients (re, im) in device memory.  Reductions are two-stage and
// deterministic through the ReduceWork, global on a process grid.
#pragma once
#include "blas.h"

namespace ddamg {

constexpr int CHRONO_MAX = 8;   // columns a kernel takes: the width rw_blas is initialised with

// r = b - y,  d_out[0] = ||b||^2,  d_out[1] = ||r||^2 in one pass: both norms come out of one reduction, so equal vectors give
// equal bits.  r == b is allowed.  24 bytes per complex number.
void chrono_residual(double* r, const double* b, const double* y, View v, ReduceWork& rw, double* d_out, hipStream_t st);
// q -= sum_i h_i Q_i  and  w -= sum_i h_i W_i  in one launch (the Gram-Schmidt step on the images Q = A V and the same
// operations carried on V): (2 m + 4) * 16 bytes per complex number
void chrono_project_pair(double* q, const double* Q, double* w, const double* W, size_t stride, int m, const double* d_h, View v, hipStream_t st);
// x = sum_i c_i W_i  and  r = b - sum_i c_i Q_i  in one launch: (2 m + 3) * 16 bytes per complex number
void chrono_combine(double* x, const double* W, double* r, const double* b, const double* Q, size_t stride, int m, const double* d_c, View v,
                    hipStream_t st);

}  // namespace ddamg
