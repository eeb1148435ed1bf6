// driver_case.h -- what the host programs of the direct kernel tests share (blas_driver.hip, transfer_driver.hip): the case
// directory a test wrote (case.txt with "key value" lines, raw little-endian arrays <name>.bin, results out_<name>.bin) and a
// device array with its length.  Each program sets driver_name before it reads a case.
#pragma once
#include "common.h"
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

static const char* driver_name = "driver";

static void need(bool ok, const std::string& what) { if (!ok) throw std::runtime_error(std::string(driver_name) + ": " + what); }

struct Case {
  std::string dir;
  std::map<std::string, std::string> kv;
  explicit Case(const std::string& d) : dir(d) {
    std::ifstream f(dir + "/case.txt");
    need((bool)f, "cannot read " + dir + "/case.txt");
    std::string k, v;
    while (f >> k >> v) kv[k] = v;
  }
  bool has(const std::string& k) const { return kv.count(k) != 0; }
  const std::string& str(const std::string& k) const {
    auto it = kv.find(k);
    need(it != kv.end(), "case lacks '" + k + "'");
    return it->second;
  }
  long long i(const std::string& k) const { return std::stoll(str(k)); }
  long long i(const std::string& k, long long dflt) const { return has(k) ? i(k) : dflt; }
  unsigned long long u(const std::string& k) const { return std::stoull(str(k)); }
  double d(const std::string& k) const { return std::stod(str(k)); }
  double d(const std::string& k, double dflt) const { return has(k) ? d(k) : dflt; }
  // "a,b,c" -> integers
  std::vector<long long> list(const std::string& k) const {
    std::vector<long long> v;
    std::stringstream ss(str(k));
    std::string tok;
    while (std::getline(ss, tok, ',')) if (!tok.empty()) v.push_back(std::stoll(tok));
    return v;
  }

  template <typename U> std::vector<U> read(const std::string& name) const {
    std::ifstream f(dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
    need((bool)f, "cannot read " + name + ".bin");
    const size_t bytes = (size_t)f.tellg();
    need(bytes % sizeof(U) == 0, name + ".bin: not a whole number of elements");
    std::vector<U> v(bytes / sizeof(U));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)bytes);
    return v;
  }
  template <typename U> void write(const std::string& name, const U* p, size_t n) const {
    std::ofstream f(dir + "/out_" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(p), (std::streamsize)(sizeof(U) * n));
    need((bool)f, "cannot write out_" + name + ".bin");
  }
};

// device array with its length
template <typename U>
struct Dev {
  ddamg::DeviceBuffer<U> p;
  size_t n = 0;
  void from(const std::vector<U>& h) { n = h.size(); p.alloc(n ? n : 1); if (n) DDAMG_HIP_CHECK(hipMemcpy(p, h.data(), sizeof(U) * n, hipMemcpyHostToDevice)); }
  void load(const Case& c, const std::string& name) { from(c.read<U>(name)); }
  std::vector<U> host() const { std::vector<U> h(n); if (n) DDAMG_HIP_CHECK(hipMemcpy(h.data(), p, sizeof(U) * n, hipMemcpyDeviceToHost)); return h; }
  void store(const Case& c, const std::string& name) const { auto h = host(); c.write(name, h.data(), h.size()); }
};
