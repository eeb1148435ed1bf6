// tools/chrono_kernel_bench.hip -- the pair projection of the chronological guess (chrono_project_pair, chrono.h) next to its
// yardstick, vec_multi_axpy_dev (blas.h), at `columns` columns on the same fp64 vectors of an L^4 lattice: milliseconds per launch
// (the median over `reps` repeats of `calls` back-to-back launches between HIP events, the two kernels in alternation inside every
// repeat, after two untimed repeats) and GB/s from the bytes the algorithm needs -- (columns + 2) vectors per family, one family
// for the multi-axpy, two for the pair projection.  One JSON line.  tools/chrono_bench.py builds and starts it.
//   chrono_kernel_bench [L = 32] [columns = 4] [calls = 20] [reps = 7]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "blas.h"
#include "chrono.h"

using namespace ddamg;

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char** argv) {
  const int L = argc > 1 ? atoi(argv[1]) : 32, m = argc > 2 ? atoi(argv[2]) : 4, calls = argc > 3 ? atoi(argv[3]) : 20, reps = argc > 4 ? atoi(argv[4]) : 7;
  if (L < 2 || L > 64 || m < 1 || m > CHRONO_MAX || calls < 1 || reps < 1) {
    fprintf(stderr, "usage: chrono_kernel_bench [L <= 64] [columns <= 8] [calls] [reps]\n");
    return 64;
  }
  try {
    const size_t n = (size_t)24 * L * L * L * L;
    const View all = whole(n);
    hipStream_t st;
    hipEvent_t e0, e1;
    DDAMG_HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    DDAMG_HIP_CHECK(hipEventCreate(&e0));
    DDAMG_HIP_CHECK(hipEventCreate(&e1));
    DeviceBuffer<double> Q, W, q, w, coef;
    Q.alloc((size_t)m * n); W.alloc((size_t)m * n); q.alloc(n); w.alloc(n); coef.alloc(2 * CHRONO_MAX);
    vec_random<double>(Q, (size_t)m * n, 1, 0, st);
    vec_random<double>(W, (size_t)m * n, 1, 1, st);
    vec_random<double>(q, n, 1, 2, st);
    vec_random<double>(w, n, 1, 3, st);
    vec_random<double>(coef, 2 * CHRONO_MAX, 1, 4, st);          // |h_i| < 1: nothing overflows in a few thousand launches
    auto timed = [&](auto launch) {
      DDAMG_HIP_CHECK(hipEventRecord(e0, st));
      for (int i = 0; i < calls; i++) launch();
      DDAMG_HIP_CHECK(hipEventRecord(e1, st));
      DDAMG_HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0;
      DDAMG_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      return (double)ms / calls;
    };
    std::vector<double> axpy, pair;
    for (int r = 0; r < reps + 2; r++) {
      const double a = timed([&] { vec_multi_axpy_dev<double>(q, Q, n, m, coef, -1.0, all, st); });
      const double p = timed([&] { chrono_project_pair(q, Q, w, W, n, m, coef, all, st); });
      if (r >= 2) { axpy.push_back(a); pair.push_back(p); }
    }
    const double family = (double)(m + 2) * n * sizeof(double);
    const double ms_axpy = median(axpy), ms_pair = median(pair);
    const double gbs_axpy = family / ms_axpy * 1e-6, gbs_pair = 2 * family / ms_pair * 1e-6;
    printf("{\"lattice\": %d, \"columns\": %d, \"calls\": %d, \"reps\": %d, \"multi_axpy_ms\": %.4f, \"multi_axpy_min_ms\": %.4f, \"multi_axpy_max_ms\": %.4f, "
           "\"multi_axpy_GBs\": %.1f, \"project_pair_ms\": %.4f, \"project_pair_min_ms\": %.4f, \"project_pair_max_ms\": %.4f, \"project_pair_GBs\": %.1f, "
           "\"ratio\": %.3f}\n",
           L, m, calls, reps, ms_axpy, *std::min_element(axpy.begin(), axpy.end()), *std::max_element(axpy.begin(), axpy.end()), gbs_axpy, ms_pair,
           *std::min_element(pair.begin(), pair.end()), *std::max_element(pair.begin(), pair.end()), gbs_pair, gbs_pair / gbs_axpy);
    DDAMG_HIP_CHECK(hipStreamSynchronize(st));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(st);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
