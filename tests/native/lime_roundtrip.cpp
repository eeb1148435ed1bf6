// lime_roundtrip.cpp -- a stand-alone host program over csrc/lime.cpp and csrc/io.cpp (no GPU, no HIP): writes and reads the 4^4
// cases of tests/test_lime_formats.py on process grids and walks the refusals.  tests/test_lime_formats.py builds it with the host
// compiler under -fsanitize=address,undefined and runs it; it prints LIME_ROUNDTRIP_OK and exits 0 when every comparison held.
#include "ddamg_hip_io.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s   [%s]\n", __LINE__, #cond, ddamg_hip_io_last_error()); failures++; } } while (0)

static const int G[4] = {4, 4, 4, 4};

// the part of the process at C of the grid P, cut out of a global lexicographic field with `reals` per site
static std::vector<double> local_part(const std::vector<double>& global, int reals, const int P[4], const int C[4]) {
  int L[4];
  for (int mu = 0; mu < 4; mu++) L[mu] = G[mu] / P[mu];
  std::vector<double> out;
  for (int t = 0; t < L[0]; t++) for (int z = 0; z < L[1]; z++) for (int y = 0; y < L[2]; y++) for (int x = 0; x < L[3]; x++) {
    const size_t s = (((size_t)(C[0] * L[0] + t) * G[1] + C[1] * L[1] + z) * G[2] + C[2] * L[2] + y) * G[3] + C[3] * L[3] + x;
    out.insert(out.end(), global.begin() + s * reals, global.begin() + (s + 1) * reals);
  }
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) { printf("usage: %s DIRECTORY\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  const size_t V = 256;
  std::vector<double> U(V * 72), phi(V * 24);
  unsigned long long state = 88172645463325252ull;
  auto next = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0 - 0.5; };
  for (double& u : U) u = next();
  for (double& v : phi) v = next();
  U[5] = -0.0; U[6] = 5e-320; U[7] = INFINITY;
  const double plaq = 1.786695870123;
  const int grids[3][4] = {{1, 1, 1, 1}, {1, 2, 1, 2}, {2, 2, 2, 2}};
  for (int precision : {64, 32})
    for (const auto& P : grids) {
      const std::string path = dir + "/conf" + std::to_string(precision) + "_" + std::to_string(P[0] * P[1] * P[2] * P[3]);
      for (int r = P[0] * P[1] * P[2] * P[3] - 1; r >= 0; r--) {
        const int C[4] = {r / (P[1] * P[2] * P[3]), r / (P[2] * P[3]) % P[1], r / P[3] % P[2], r % P[3]};
        CHECK(ddamg_hip_write_ildg_conf(path.c_str(), G, P, C, precision, local_part(U, 72, P, C).data(), plaq) == 0);
      }
      struct ddamg_hip_lime_info info;
      CHECK(ddamg_hip_lime_info(path.c_str(), &info) == 0);
      CHECK(info.kind == 1 && info.precision == precision && info.num_records == 3 && info.has_plaquette && info.plaquette == plaq / 3.0);
      CHECK(info.data_length == (long long)(V * 72 * precision / 8));
      for (int r = 0; r < P[0] * P[1] * P[2] * P[3]; r++) {
        const int C[4] = {r / (P[1] * P[2] * P[3]), r / (P[2] * P[3]) % P[1], r / P[3] % P[2], r % P[3]};
        std::vector<double> want = local_part(U, 72, P, C), got(want.size(), 7.5);
        if (precision == 32) for (double& w : want) w = (double)(float)w;
        double pl = 0; int has = 0;
        CHECK(ddamg_hip_read_ildg_conf(path.c_str(), G, P, C, got.data(), &pl, &has) == 0);
        CHECK(has == 1 && std::fabs(pl - plaq) <= 1e-14 * plaq);
        CHECK(memcmp(got.data(), want.data(), want.size() * sizeof(double)) == 0);
      }
    }
  for (const auto& P : grids) {
    const std::string path = dir + "/vec_" + std::to_string(P[0] * P[1] * P[2] * P[3]);
    const ddamg_hip_vector_header h = {"solution", -0.5, 1.0, 1.6, 1.6, "conf/a", nullptr, 0, nullptr};
    for (int r = P[0] * P[1] * P[2] * P[3] - 1; r >= 0; r--) {
      const int C[4] = {r / (P[1] * P[2] * P[3]), r / (P[2] * P[3]) % P[1], r / P[3] % P[2], r % P[3]};
      CHECK(ddamg_hip_write_lime_vector(path.c_str(), G, P, C, P[0] > 1 ? &h : nullptr, local_part(phi, 24, P, C).data()) == 0);
    }
    for (int r = 0; r < P[0] * P[1] * P[2] * P[3]; r++) {
      const int C[4] = {r / (P[1] * P[2] * P[3]), r / (P[2] * P[3]) % P[1], r / P[3] % P[2], r % P[3]};
      std::vector<double> want = local_part(phi, 24, P, C), got(want.size(), 7.5);
      CHECK(ddamg_hip_read_lime_vector(path.c_str(), G, P, C, got.data()) == 0);
      CHECK(memcmp(got.data(), want.data(), want.size() * sizeof(double)) == 0);
    }
  }
  // refusals: every one returns -1 with a text and writes nothing
  std::vector<double> out(V * 72, 7.5);
  const int one[4] = {1, 1, 1, 1}, zero[4] = {0, 0, 0, 0}, three[4] = {3, 1, 1, 1}, big[4] = {8, 4, 4, 4};
  const std::string good = dir + "/conf64_1", vec = dir + "/vec_1";
  CHECK(ddamg_hip_read_ildg_conf((dir + "/missing").c_str(), G, one, zero, out.data(), nullptr, nullptr) == -1 && strstr(ddamg_hip_io_last_error(), "cannot open"));
  CHECK(ddamg_hip_read_ildg_conf(good.c_str(), big, one, zero, out.data(), nullptr, nullptr) == -1 && strstr(ddamg_hip_io_last_error(), "expected 8x4x4x4"));
  CHECK(ddamg_hip_read_ildg_conf(good.c_str(), G, three, zero, out.data(), nullptr, nullptr) == -1 && strstr(ddamg_hip_io_last_error(), "does not divide"));
  CHECK(ddamg_hip_read_ildg_conf(vec.c_str(), G, one, zero, out.data(), nullptr, nullptr) == -1 && strstr(ddamg_hip_io_last_error(), "no binary record"));
  CHECK(ddamg_hip_read_lime_vector(good.c_str(), G, one, zero, out.data()) == -1 && strstr(ddamg_hip_io_last_error(), "no binary record"));
  {
    FILE* in = fopen(good.c_str(), "rb"); FILE* cut = fopen((dir + "/short").c_str(), "wb"); FILE* bad = fopen((dir + "/magic").c_str(), "wb");
    CHECK(in && cut && bad);
    if (in && cut && bad) {
      std::vector<char> bytes(100000);
      const size_t n = fread(bytes.data(), 1, bytes.size(), in);
      fwrite(bytes.data(), 1, n - 1000 < n ? n - 1000 : 0, cut);
      bytes[3] = 0; fwrite(bytes.data(), 1, n, bad);
    }
    if (in) fclose(in);
    if (cut) fclose(cut);
    if (bad) fclose(bad);
  }
  CHECK(ddamg_hip_read_ildg_conf((dir + "/short").c_str(), G, one, zero, out.data(), nullptr, nullptr) == -1 && strstr(ddamg_hip_io_last_error(), "ends early"));
  CHECK(ddamg_hip_read_ildg_conf((dir + "/magic").c_str(), G, one, zero, out.data(), nullptr, nullptr) == -1 && strstr(ddamg_hip_io_last_error(), "not a LIME file"));
  for (double v : out) if (v != 7.5) { failures++; break; }
  if (failures == 0) printf("LIME_ROUNDTRIP_OK\n");
  return failures != 0;
}
