// Owner of one psh_malloc block that lives for one call: freed (stream-ordered, as psh_free is) when it goes out of
// scope, whichever return the function takes.  Declare it after the entry point's PSH_ENTER (entry.h), so that the
// free happens with the lock still held.  Host code only; no HIP header needed.
#pragma once

#include <cstddef>

#include "../../include/pysteps_hip.h"

namespace psh {

class Scratch {
 public:
  Scratch() = default;
  explicit Scratch(void *adopted) : p_(adopted) {}  // takes over a block that psh_malloc handed out earlier
  Scratch(Scratch &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  Scratch &operator=(Scratch &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      o.p_ = nullptr;
    }
    return *this;
  }
  Scratch(const Scratch &) = delete;
  Scratch &operator=(const Scratch &) = delete;
  ~Scratch() { reset(); }

  // psh_malloc's code; the pointer stays nullptr on failure.  A block held already is freed first
  int alloc(size_t bytes) {
    reset();
    const int rc = psh_malloc(&p_, bytes);
    if (rc) p_ = nullptr;
    return rc;
  }
  void reset() {  // frees now
    if (p_) (void)psh_free(p_);
    p_ = nullptr;
  }
  void *release() {  // gives the block up: the caller frees it
    void *p = p_;
    p_ = nullptr;
    return p;
  }
  template <class T> T *as() const { return static_cast<T *>(p_); }
  template <class T> T *at(size_t byte_offset) const { return reinterpret_cast<T *>(static_cast<char *>(p_) + byte_offset); }

 private:
  void *p_ = nullptr;
};

}  // namespace psh
