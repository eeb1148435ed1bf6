// gauge.h -- see gauge.cpp
#pragma once
#include <hip/hip_runtime.h>
namespace ddamg {
// gauge_in: [V][4][9] complex fp64 lexicographic (T,Z,Y,X; X fastest).  Writes D_out [V][36] complex
// (= U/2, after the optional anti-periodic sign) and clover_out [V][42] complex in the reference's
// storage; returns the average plaquette in [0,3].  Single process, computed on the device: links up, D / clover /
// plaquette down; gauge_device.hip
double gauge_to_operator_device(const int L[4], const double* gauge_in, int anti_pbc, double m0, double csw, double* D_out, double* clover_out,
                                hipStream_t st);
// clover term of the own sites and the sum of their plaquette traces from the links of the lattice extended by `halo`
// sites in every direction (U_ext_host: [prod(L+2 halo)][4][9] complex, lexicographic in the extended lattice), on the device
double clover_and_plaquette_extended_device(const int L[4], const int halo[4], const double* U_ext_host, double m0, double csw, double* clover_out, hipStream_t st);
// the same on a process grid: gauge_in is the process's own part; the links of the neighbouring processes that the
// clover leaves reach (one site deep, corners included) are fetched first (the reference exchanges the ghost shell of
// the gauge field in dirac_setup, src/dirac.c:88-120); the plaquette is the global average
// links that stay in device memory (ddamg_hip_set_gauge_device): dU_hopp / dU_clover [V][4][9] complex fp64 lexicographic on the
// device, read in place and never written (the anti-periodic sign is applied in the loads); writes the device arrays dD [V][36]
// complex = U_hopp / 2 with the sign and dC [V][42] complex, the clover term of U_clover; returns the average plaquette of
// U_clover, summed on the device.  Single process.  Waits for the stream.
double gauge_to_operator_resident(const int L[4], const double* dU_hopp, const double* dU_clover, int anti_pbc, double m0, double csw, double* dD,
                                  double* dC, hipStream_t st);
// measurement (ddamg_hip_clover_kernel_time): `reps` launches, after one untimed, of the field-strength kernel (which = 0), of the
// host path's clover_kernel (1) or of the field-strength, assembly and plaquette-sum kernels (2) on the links dU, between the
// events e0 and e1; *ms = milliseconds per launch; returns the average plaquette that the kernels give
double clover_kernels_timed(const int L[4], const double* dU, double m0, double csw, int which, int reps, hipEvent_t e0, hipEvent_t e1, hipStream_t st,
                            float* ms);
struct Geometry;
struct Comm;
// gauge_to_operator_resident on a process grid (ddamg_hip_set_gauge_device_grid): the process's own links in device memory, read
// in place and never written.  The clover field's links are copied into the local lattice extended by one site in every split
// direction, the neighbours' shell (corners included) is exchanged device to device over the transport, and the field-strength
// kernel runs on the extended array; D comes from the own hopping links alone.  Collective; returns the global average plaquette
// (one all-reduce).  Waits for the stream; the extended array and the slab buffers live for the call only.
double gauge_to_operator_resident_grid(const Geometry& g, Comm* comm, const double* dU_hopp, const double* dU_clover, int anti_pbc, double m0, double csw,
                                       double* dD, double* dC, hipStream_t st);
// measurement (ddamg_hip_clover_kernel_time, which = 3): the field-strength kernel on the extended array of the links dU, built
// once as above; *ms = milliseconds per launch; returns this process's average plaquette
double extended_field_strength_timed(const Geometry& g, Comm* comm, const double* dU, int reps, hipEvent_t e0, hipEvent_t e1, hipStream_t st, float* ms);
double gauge_to_operator_dist(const Geometry& g, Comm* comm, const double* gauge_in, int anti_pbc, double m0, double csw,
                              double* D_out, double* clover_out, hipStream_t st);
}
