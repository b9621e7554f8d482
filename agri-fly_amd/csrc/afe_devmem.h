// afe_devmem.h -- the one owner of a block of memory that somebody else hands out (device memory, pinned host memory).
// Internal to the library, host only, header only, and free of HIP: where the memory comes from is the policy's business
//   struct Policy { static void *get(size_t bytes);   // nullptr: refused, and nothing of the refusal is left pending (reserve may ask again)
//                   static void put(void *p); };
// (afe_consumer.h names the two policies the library uses), so the rules below are tested on the CPU against malloc
// (tests/test_devmem.py).
//
// THE RULE the handles rely on: the capacity is the buffer's, never a number kept beside it.  A refused growth leaves the
// buffer EMPTY -- get() == nullptr and capacity() == 0 -- so the next call that needs it asks again (and is granted or refused
// again) and no launch ever sees a pointer that an earlier failure has left behind.
#pragma once
#include <stddef.h>

namespace afe {

template <class Policy>
struct OwnedBuf {
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf &) = delete;
  OwnedBuf &operator=(const OwnedBuf &) = delete;
  OwnedBuf(OwnedBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  OwnedBuf &operator=(OwnedBuf &&o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~OwnedBuf() { reset(); }

  void reset() {
    if (p_) Policy::put(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // exactly `bytes` (one byte for none, so that a granted request always has an address), whatever was held given back first
  bool alloc(size_t bytes) {
    reset();
    return take(bytes ? bytes : 1);
  }
  // Room for `need` bytes.  Enough already: nothing happens.  Otherwise what is held goes back and `want` (>= need: the
  // caller's headroom) is asked for, then `need` alone if that is refused.  false: both refused, the buffer is empty.
  // *replaced (optional) is set when what was held went back, granted or not -- whatever was in it is gone -- and left alone otherwise.
  bool reserve(size_t need, size_t want, bool *replaced = nullptr) {
    if (cap_ >= need) return true;
    if (replaced) *replaced = true;
    reset();
    return take(want) || (want > need && take(need));
  }

  size_t capacity() const { return cap_; }
  void *get() const { return p_; }
  template <class T>
  T *as() const { return static_cast<T *>(p_); }

 private:
  void *p_ = nullptr;
  size_t cap_ = 0;
  bool take(size_t bytes) {
    p_ = Policy::get(bytes);
    cap_ = p_ ? bytes : 0;
    return p_ != nullptr;
  }
};

}  // namespace afe
