// ildg_device.hip -- the data of an "ildg-binary-data" record <-> links, on the device (ildg_device.h).
//
// The reference turns a record into links on the host, one number at a time: byteswap8 / byteswap per real, a conversion per
// real for fp32 files, then swap_spin_in_conf per site (src/lime_io.c:50-72,273-314).  Here it is one streaming pass: one thread
// per complex number, a 16-byte load and a 16-byte store (8 bytes on the file side of an fp32 record), the byte order swapped in
// registers and the direction reversal X,Y,Z,T -> T,Z,Y,X folded into the index.  Consecutive threads read consecutive
// addresses; they write consecutive addresses within a link (9 complex = 144 bytes), the links of a site in reverse order.  No
// LDS, no atomics.  fp64 numbers are moved as integers, so every bit pattern arrives as it was.
#include "common.h"
#include "ildg_device.h"

namespace ddamg {

namespace {

constexpr int ILDG_THREADS = 256;

// complex number i of the record (site-major, 36 per site) sits at this index of the links, and the other way round: the
// map is its own inverse
__device__ __forceinline__ size_t reversed_direction(size_t i) {
  const size_t site = i / 36;
  const unsigned r = (unsigned)(i - site * 36), mu = r / 9, k = r - mu * 9;
  return site * 36 + (3 - mu) * 9 + k;
}

template <int P> struct FileComplex;
template <> struct FileComplex<64> { using type = ulonglong2; };
template <> struct FileComplex<32> { using type = uint2; };

template <int P>
__global__ void __launch_bounds__(ILDG_THREADS) ildg_to_links_kernel(const typename FileComplex<P>::type* __restrict__ raw, ulonglong2* __restrict__ links, size_t ncomplex) {
  const size_t i = (size_t)blockIdx.x * ILDG_THREADS + threadIdx.x;
  if (i >= ncomplex) return;
  const auto v = raw[i];
  ulonglong2 out;
  if constexpr (P == 64) {
    out.x = __builtin_bswap64(v.x); out.y = __builtin_bswap64(v.y);
  } else {
    out.x = (unsigned long long)__double_as_longlong((double)__uint_as_float(__builtin_bswap32(v.x)));   // fp32 -> fp64 is exact
    out.y = (unsigned long long)__double_as_longlong((double)__uint_as_float(__builtin_bswap32(v.y)));
  }
  links[reversed_direction(i)] = out;
}

template <int P>
__global__ void __launch_bounds__(ILDG_THREADS) links_to_ildg_kernel(const ulonglong2* __restrict__ links, typename FileComplex<P>::type* __restrict__ raw, size_t ncomplex) {
  const size_t i = (size_t)blockIdx.x * ILDG_THREADS + threadIdx.x;
  if (i >= ncomplex) return;
  const ulonglong2 v = links[reversed_direction(i)];
  typename FileComplex<P>::type out;
  if constexpr (P == 64) {
    out.x = __builtin_bswap64(v.x); out.y = __builtin_bswap64(v.y);
  } else {
    out.x = __builtin_bswap32(__float_as_uint((float)__longlong_as_double((long long)v.x)));   // round to nearest even
    out.y = __builtin_bswap32(__float_as_uint((float)__longlong_as_double((long long)v.y)));
  }
  raw[i] = out;
}

unsigned blocks_for(size_t ncomplex) {
  const size_t blocks = (ncomplex + ILDG_THREADS - 1) / ILDG_THREADS;
  DDAMG_REQUIRE(blocks <= 0x7fffffffu, "ildg conversion: more sites than one launch covers (convert the record in parts)");
  return (unsigned)blocks;
}

}  // namespace

void ildg_to_links(const void* raw, int precision, size_t nsites, double* links, hipStream_t st) {
  const size_t n = nsites * 36;
  if (n == 0) return;
  if (precision == 64) ildg_to_links_kernel<64><<<blocks_for(n), ILDG_THREADS, 0, st>>>((const ulonglong2*)raw, (ulonglong2*)links, n);
  else ildg_to_links_kernel<32><<<blocks_for(n), ILDG_THREADS, 0, st>>>((const uint2*)raw, (ulonglong2*)links, n);
  DDAMG_HIP_CHECK(hipGetLastError());
}

void links_to_ildg(const double* links, int precision, size_t nsites, void* raw, hipStream_t st) {
  const size_t n = nsites * 36;
  if (n == 0) return;
  if (precision == 64) links_to_ildg_kernel<64><<<blocks_for(n), ILDG_THREADS, 0, st>>>((const ulonglong2*)links, (ulonglong2*)raw, n);
  else links_to_ildg_kernel<32><<<blocks_for(n), ILDG_THREADS, 0, st>>>((const ulonglong2*)links, (uint2*)raw, n);
  DDAMG_HIP_CHECK(hipGetLastError());
}

}  // namespace ddamg
