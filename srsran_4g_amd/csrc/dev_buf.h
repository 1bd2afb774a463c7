// Owning device / pinned-host buffers for the *_api.cpp objects (host code only).
//
// DevBuf<T> owns one hipMalloc allocation of T, PinBuf<T> one hipHostMalloc allocation.  Both are move-only,
// grow by free + allocate (contents are NOT preserved) and release in their destructor, so an object that
// holds them frees everything with `delete g`.  They know nothing about streams: a caller that may have
// work in flight on the old block synchronises BEFORE reserve() / reset().  Buffers that grow as a group: a
// failed reserve() empties only its own buffer, so the "must grow" test looks at EVERY member's cap() (or the
// group is reset() first), never at one member standing for the others.  Never put one in a static or
// otherwise process-lifetime holder that gets destroyed at exit (the HIP runtime is gone by then).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace srsran_amd {

namespace detail {
// Buf<T, Pinned>: the one implementation behind DevBuf / PinBuf
template <typename T, bool Pinned>
class Buf {
  T*       p_     = nullptr;
  size_t   cap_   = 0;        // elements of T
  unsigned flags_ = 0;        // hipHostMalloc flags (PinBuf only)

 public:
  Buf() = default;
  explicit Buf(unsigned host_flags) : flags_(host_flags) {}
  Buf(const Buf&)            = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_), flags_(o.flags_) { o.p_ = nullptr, o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, cap_ = o.cap_, flags_ = o.flags_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~Buf() { reset(); }

  // true and nothing done when n <= cap(); otherwise free, then allocate max(n, floor) elements.
  // After a failed allocation the buffer is empty (get() == nullptr, cap() == 0).
  bool reserve(size_t n, size_t floor = 0) {
    if (n <= cap_) return true;
    reset();
    if (n < floor) n = floor;
    void*      q = nullptr;
    hipError_t e = Pinned ? hipHostMalloc(&q, n * sizeof(T), flags_) : hipMalloc(&q, n * sizeof(T));
    if (e != hipSuccess || !q) return false;
    p_ = static_cast<T*>(q), cap_ = n;
    return true;
  }
  void reset() {
    if (p_) Pinned ? (void)hipHostFree(p_) : (void)hipFree(p_);
    p_ = nullptr, cap_ = 0;
  }
  T*     get() const { return p_; }
  size_t cap() const { return cap_; }
  // deliberate: a member reads as the pointer it replaced (arguments, arithmetic, null tests); a cast to
  // another pointer type does not go through it and takes get()
  operator T*() const { return p_; }
};
}  // namespace detail

template <typename T>
using DevBuf = detail::Buf<T, false>;
template <typename T>
using PinBuf = detail::Buf<T, true>;

}  // namespace srsran_amd
