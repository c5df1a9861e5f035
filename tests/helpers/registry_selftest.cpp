// Stand-alone exercise of pysteps_amd/csrc/registry.h with malloc underneath, meant to be built with
// -fsanitize=address,undefined (tests/test_ownership_rule.py does): register, grow, drop, release, register again,
// release again.  A double free, a use after free or a leak in those paths ends the program with a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../pysteps_amd/csrc/registry.h"

namespace {

int g_live = 0, g_quiesced = 0, g_hooked = 0, g_fail_next = 0;

int test_alloc(psh::MemKind kind, void **out, size_t nbytes) {
  if (g_fail_next) {
    g_fail_next = 0;
    return -4;
  }
  char *p = static_cast<char *>(std::malloc(nbytes + 1));
  p[0] = static_cast<char>(kind);  // release() checks that a block comes back as the kind it was made as
  *out = p + 1;
  ++g_live;
  return 0;
}
void test_release(psh::MemKind kind, void *block) {
  char *p = static_cast<char *>(block) - 1;
  if (p[0] != static_cast<char>(kind)) std::abort();
  std::free(p);
  --g_live;
}
int test_quiesce() {
  ++g_quiesced;
  return 0;
}

#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                   \
    }                                                             \
  } while (0)

void *g_a = nullptr, *g_b = nullptr;

int run() {
  psh::Registry r{test_alloc, test_release, test_quiesce};
  r.hooks.push_back([] { ++g_hooked; });
  std::map<int, void *> tables;  // slots inside a node-based container, as the FFT tables are
  for (int cycle = 0; cycle < 3; ++cycle) {
    const unsigned long long gen0 = r.generation;
    CHECK(g_a == nullptr && g_b == nullptr && g_live == 0);
    CHECK(r.ensure(psh::kMemDevice, &g_a, 100) == 0 && g_a != nullptr);
    std::memset(g_a, 1, 100);
    CHECK(r.generation != gen0);
    const unsigned long long gen1 = r.generation;
    void *first = g_a;
    CHECK(r.ensure(psh::kMemDevice, &g_a, 40) == 0 && g_a == first);  // enough already: the same block, no wait
    CHECK(r.generation == gen1 && g_quiesced == 2 * cycle);
    CHECK(r.ensure(psh::kMemDevice, &g_a, 4000) == 0 && g_a != nullptr);  // grows: waits, frees, allocates
    std::memset(g_a, 2, 4000);
    CHECK(r.generation != gen1 && g_quiesced == 2 * cycle + 1 && g_live == 1);
    CHECK(r.ensure(psh::kMemPinned, &g_b, 64) == 0);
    std::memset(g_b, 3, 64);
    g_fail_next = 1;  // a failed regrow leaves NULL and nothing registered
    CHECK(r.ensure(psh::kMemPinned, &g_b, 128) != 0 && g_b == nullptr && g_live == 1);
    CHECK(r.blocks.count(&g_b) == 0 && g_quiesced == 2 * cycle + 2);
    CHECK(r.ensure(psh::kMemPinned, &g_b, 128) == 0 && g_b != nullptr);
    std::memset(g_b, 4, 128);
    for (int n = 0; n < 5; ++n) {
      CHECK(r.ensure(psh::kMemDevice, &tables[n], 16 << n) == 0);
      std::memset(tables[n], 5, 16 << n);
    }
    r.drop(&tables[2]);
    CHECK(tables[2] == nullptr && g_live == 6);
    r.drop(&tables[2]);  // not registered any more: nothing happens
    CHECK(g_live == 6);
    r.release_all();
    CHECK(g_live == 0 && g_a == nullptr && g_b == nullptr && r.blocks.empty());
    for (int n = 0; n < 5; ++n) CHECK(tables[n] == nullptr);
    CHECK(g_hooked == cycle + 1 && r.hooks.size() == 1);
    r.release_all();  // nothing registered: only the hooks run again
    CHECK(g_live == 0 && g_hooked == cycle + 2);
    g_hooked = cycle + 1;
  }
  return 0;
}

}  // namespace

int main() {
  const int rc = run();
  std::puts(rc == 0 ? "registry selftest: ok" : "registry selftest: FAILED");
  return rc;
}
