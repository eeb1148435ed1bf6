// io_common.h -- what io.cpp and lime.cpp share: the error text behind ddamg_hip_io_last_error, a process's part of the
// lattice, whole-buffer pread / pwrite.  Host code only, standard library and POSIX.
#pragma once
#include "../../include/ddamg_hip_io.h"
#include <cstddef>
#include <cstdint>
#include <sys/types.h>
#include <unistd.h>

namespace ddamg_io {

// formats the text of ddamg_hip_io_last_error (per thread) and returns -1 (io.cpp)
int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

struct Part {
  int G[4], L[4], O[4];   // global extents, local extents, origin of this process
  size_t Vloc, Vglob;
};
inline bool make_part(const int G[4], const int P[4], const int C[4], Part& p) {
  p.Vloc = 1; p.Vglob = 1;
  for (int mu = 0; mu < 4; mu++) {
    const int np = P[mu] < 1 ? 1 : P[mu];
    if (G[mu] < 1 || G[mu] % np || C[mu] < 0 || C[mu] >= np) return false;
    p.G[mu] = G[mu]; p.L[mu] = G[mu] / np; p.O[mu] = C[mu] * p.L[mu];
    p.Vloc *= p.L[mu]; p.Vglob *= G[mu];
  }
  return true;
}
inline bool at_origin(const Part& p) { return p.O[0] == 0 && p.O[1] == 0 && p.O[2] == 0 && p.O[3] == 0; }

// rows of L[X] consecutive sites: the unit the reference moves as well (read_size = 4*18*ll[X], bar_size = 24*ll[X])
template <typename F>
int for_rows(const Part& p, F&& f) {
  size_t row = 0;
  for (int t = 0; t < p.L[0]; t++) for (int z = 0; z < p.L[1]; z++) for (int y = 0; y < p.L[2]; y++, row++) {
    const size_t gsite = (((size_t)(p.O[0] + t) * p.G[1] + (p.O[1] + z)) * p.G[2] + (p.O[2] + y)) * p.G[3] + p.O[3];
    if (int rc = f(row, gsite)) return rc;
  }
  return 0;
}

inline int pread_all(int fd, void* buf, size_t n, off_t off) {
  char* b = static_cast<char*>(buf);
  while (n) { ssize_t r = pread(fd, b, n, off); if (r <= 0) return -1; b += r; off += r; n -= (size_t)r; }
  return 0;
}
inline int pwrite_all(int fd, const void* buf, size_t n, off_t off) {
  const char* b = static_cast<const char*>(buf);
  while (n) { ssize_t r = pwrite(fd, b, n, off); if (r <= 0) return -1; b += r; off += r; n -= (size_t)r; }
  return 0;
}

// lime.cpp: the scan of ddamg_hip_lime_info and every check ddamg_hip_read_ildg_conf makes of the file against the global lattice G
// (a configuration, complete format record, G itself, record length, file long enough); ddamg_hip_load_ildg_conf reads the record
// described by *info itself.  Returns 0, or -1 with the error text set.
int ildg_checked_info(const char* path, const int G[4], struct ddamg_hip_lime_info* info);

}  // namespace ddamg_io
