// ildg_device.h -- see ildg_device.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
namespace ddamg {
// raw: the data of an "ildg-binary-data" record (include/ddamg_hip_io.h) for nsites sites in device memory, big-endian fp64
// (precision 64) or fp32 (32), directions X,Y,Z,T per site; links: [nsites][4][9] complex fp64, directions T,Z,Y,X.  One kernel
// launch on `st` each, no synchronisation; raw and links 16-byte aligned (fp32 raw: 8).
void ildg_to_links(const void* raw, int precision, size_t nsites, double* links, hipStream_t st);
void links_to_ildg(const double* links, int precision, size_t nsites, void* raw, hipStream_t st);
}
