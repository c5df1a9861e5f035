// Stand-alone exercise of pysteps_amd/csrc/scratch.h with malloc underneath, meant to be built with
// -fsanitize=address,undefined (tests/test_ownership_rule.py does): psh_malloc / psh_free are defined HERE over
// malloc / free with a live-block counter.  A double free, a use after free or a leak ends the program with a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "../../pysteps_amd/csrc/scratch.h"

namespace {
int g_live = 0, g_frees = 0, g_fail_next = 0;
}  // namespace

extern "C" int psh_malloc(void **dev_ptr, size_t nbytes) {
  if (g_fail_next) {
    g_fail_next = 0;
    return PSH_ENOMEM;
  }
  *dev_ptr = std::malloc(nbytes ? nbytes : 1);
  ++g_live;
  return PSH_OK;
}
extern "C" int psh_free(void *dev_ptr) {
  if (!dev_ptr) return PSH_OK;
  std::free(dev_ptr);
  --g_live;
  ++g_frees;
  return PSH_OK;
}

namespace {

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

// an entry point's shape: two blocks, then a step that fails and returns early
int two_blocks_then(int fail_code) {
  psh::Scratch a, b;
  if (int rc = a.alloc(64)) return rc;
  if (int rc = b.alloc(32)) return rc;
  std::memset(a.as<char>(), 1, 64);
  std::memset(b.as<char>(), 2, 32);
  if (g_live != 2) return -1000;
  if (fail_code) return fail_code;
  return PSH_OK;
}

int run() {
  {  // alloc and scope exit; the carving accessors
    psh::Scratch s;
    CHECK(s.as<void>() == nullptr);
    CHECK(s.alloc(256) == PSH_OK && s.as<void>() != nullptr && g_live == 1);
    std::memset(s.as<char>(), 3, 256);
    CHECK(s.at<char>(0) == s.as<char>());
    CHECK(reinterpret_cast<char *>(s.at<double>(128)) == s.as<char>() + 128);
    s.at<int>(252)[0] = 7;
  }
  CHECK(g_live == 0 && g_frees == 1);
  {  // a failed alloc: pointer null, nothing freed
    psh::Scratch s;
    g_fail_next = 1;
    CHECK(s.alloc(16) == PSH_ENOMEM && s.as<void>() == nullptr && g_live == 0);
  }
  CHECK(g_live == 0 && g_frees == 1);
  // early return out of a function holding two blocks, and the plain return
  CHECK(two_blocks_then(PSH_EHIP) == PSH_EHIP && g_live == 0 && g_frees == 3);
  CHECK(two_blocks_then(0) == PSH_OK && g_live == 0 && g_frees == 5);
  g_fail_next = 0;
  {  // the second allocation fails: the first block still goes back
    struct FailSecond {
      static int call() {
        psh::Scratch a, b;
        if (int rc = a.alloc(8)) return rc;
        g_fail_next = 1;
        if (int rc = b.alloc(8)) return rc;
        return PSH_OK;
      }
    };
    CHECK(FailSecond::call() == PSH_ENOMEM && g_live == 0 && g_frees == 6);
  }
  {  // reset, then destruction: no double free; reset of an empty one is nothing
    psh::Scratch s;
    s.reset();
    CHECK(s.alloc(40) == PSH_OK && g_live == 1);
    s.reset();
    CHECK(s.as<void>() == nullptr && g_live == 0 && g_frees == 7);
    s.reset();
    CHECK(g_frees == 7);
  }
  CHECK(g_live == 0 && g_frees == 7);
  void *kept = nullptr;
  {  // release: the block stays the caller's
    psh::Scratch s;
    CHECK(s.alloc(24) == PSH_OK);
    kept = s.release();
    CHECK(kept != nullptr && s.as<void>() == nullptr && g_live == 1);
  }
  CHECK(g_live == 1 && g_frees == 7);
  {  // the adopting constructor takes it back
    const psh::Scratch s(kept);
    CHECK(s.as<void>() == kept && g_live == 1);
  }
  CHECK(g_live == 0 && g_frees == 8);
  {  // adopting nothing frees nothing
    const psh::Scratch s(nullptr);
  }
  CHECK(g_frees == 8);
  {  // move construction and move assignment: the moved-from object frees nothing
    psh::Scratch a;
    CHECK(a.alloc(48) == PSH_OK);
    void *p = a.as<void>();
    psh::Scratch b(std::move(a));
    CHECK(a.as<void>() == nullptr && b.as<void>() == p && g_live == 1);
    psh::Scratch c;
    CHECK(c.alloc(16) == PSH_OK && g_live == 2);
    c = std::move(b);  // c's own block is freed, b's moves in
    CHECK(b.as<void>() == nullptr && c.as<void>() == p && g_live == 1 && g_frees == 9);
    psh::Scratch &self = c;
    c = std::move(self);  // onto itself: nothing happens
    CHECK(c.as<void>() == p && g_live == 1 && g_frees == 9);
  }
  CHECK(g_live == 0 && g_frees == 10);
  return 0;
}

}  // namespace

int main() {
  const int rc = run();
  const bool ok = rc == 0 && g_live == 0;
  std::puts(ok ? "scratch selftest: ok" : "scratch selftest: FAILED");
  return ok ? 0 : 1;
}
