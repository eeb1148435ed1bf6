// device_buffer.h -- the owners of device and pinned host memory.  hipMalloc / hipFree / hipHostMalloc / hipHostFree appear
// in the library in this header only; common.h includes it after the error macros it uses.
//
// A buffer is move-only, owns at most one allocation and gives it back in its destructor, so a throw anywhere (the library
// reports errors by throwing, DDAMG_HIP_CHECK / DDAMG_REQUIRE) unwinds to no leak.  It converts to T* implicitly: kernel
// launches, argument structs and pointer arithmetic take it as they took the raw pointer.  It does NOT zero-fill: whether a
// fill runs on the null stream with a device synchronisation (device_zero) or on the library's stream (hipMemsetAsync) is
// the caller's decision, see device_zero.
#pragma once
#include <atomic>
#include <utility>
#include <vector>

namespace ddamg {

// Every device allocation of the library goes through here.  DDAMG_POISON=1 fills fresh allocations with 0xFF bytes
// (NaN as float/double, -1 as int): a read of memory the library has not written itself then poisons the result
// instead of going unnoticed (device memory handed out by the driver is usually zero, sometimes recycled).
template <typename P>
inline hipError_t device_alloc(P** p, size_t bytes) {
  hipError_t e = hipMalloc(reinterpret_cast<void**>(p), bytes);
  if (e == hipSuccess && poison_allocations() && bytes) {
    e = hipMemset(*p, 0xFF, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();   // the library's streams do not synchronise with the null stream
    if (e != hipSuccess) { (void)hipFree(*p); *p = nullptr; }
  }
  return e;
}

// zero-fill at allocation time.  hipMemset runs on the null stream, which the library's non-blocking streams do NOT
// wait for: without the synchronisation a long fill (a Krylov slab of many GB) overlaps with the first kernels that
// write into the same memory and wipes their results.
inline hipError_t device_zero(void* p, size_t bytes) {
  hipError_t e = hipMemset(p, 0, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}

// bytes owned by live buffers of this process (ddamg_hip_memory_in_use).  What RCCL or the runtime allocate for themselves
// is not counted.
struct DeviceMemory {
  static inline std::atomic<size_t> in_use{0};
  static hipError_t allocate(void** p, size_t bytes) { return device_alloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};
struct PinnedMemory {
  static inline std::atomic<size_t> in_use{0};
  static hipError_t allocate(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void* p) { (void)hipHostFree(p); }
};

template <typename T, typename Memory>
class Buffer {
 public:
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
    return *this;
  }
  ~Buffer() { reset(); }

  // n elements plus `extra_bytes` (a few fields carry a trailing word); frees what the buffer held before
  void alloc(size_t n, size_t extra_bytes = 0) {
    reset();
    const size_t bytes = sizeof(T) * n + extra_bytes;
    void* p = nullptr;
    DDAMG_HIP_CHECK(Memory::allocate(&p, bytes));
    p_ = static_cast<T*>(p); bytes_ = bytes;
    Memory::in_use += bytes;
  }
  // alloc + the copy of a host vector: synchronous, or asynchronous on `st` (the caller synchronises before `v` dies)
  template <typename U> void upload(const std::vector<U>& v) {
    alloc_as(v);
    DDAMG_HIP_CHECK(hipMemcpy(p_, v.data(), sizeof(U) * v.size(), hipMemcpyHostToDevice));
  }
  template <typename U> void upload(const std::vector<U>& v, hipStream_t st) {
    alloc_as(v);
    DDAMG_HIP_CHECK(hipMemcpyAsync(p_, v.data(), sizeof(U) * v.size(), hipMemcpyHostToDevice, st));
  }
  void reset() {
    if (p_) { Memory::release(p_); Memory::in_use -= bytes_; }
    p_ = nullptr; bytes_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t bytes() const { return bytes_; }
  size_t size() const { return bytes_ / sizeof(T); }

 private:
  template <typename U> void alloc_as(const std::vector<U>& v) {
    static_assert(sizeof(U) % sizeof(T) == 0, "upload: the host element is a whole number of buffer elements");
    alloc(v.size() * (sizeof(U) / sizeof(T)));
  }
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

template <typename T> using DeviceBuffer = Buffer<T, DeviceMemory>;
template <typename T> using PinnedBuffer = Buffer<T, PinnedMemory>;

}  // namespace ddamg
