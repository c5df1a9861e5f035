// The library's one ownership rule, in plain host C++ (no HIP: tests/helpers/registry_selftest.cpp runs it under the
// sanitizers with malloc underneath).  Memory the library keeps for its own lifetime hangs on a SLOT - a pointer with
// static storage, or inside a container nothing is erased from - and comes from ensure().  Whatever else has a device
// lifetime (streams, events, pools, a communicator, ring positions) is put right by a hook its translation unit
// registers once.  release_all() is the only release path.
#pragma once

#include <cstddef>
#include <map>
#include <vector>

namespace psh {
enum MemKind { kMemDevice = 0, kMemPinned = 1 };

struct Registry {
  // the allocator underneath; alloc returns 0 and sets *out, or an error code and leaves *out alone
  int (*alloc)(MemKind kind, void **out, size_t nbytes);
  void (*release)(MemKind kind, void *block);
  int (*quiesce)();  // wait until nothing queued can still touch a block that is about to be freed; 0 = done
  struct Block { size_t bytes; MemKind kind; };
  std::map<void **, Block> blocks;  // by slot address: the size lives next to the pointer
  std::vector<void (*)()> hooks;    // kept across release_all()
  // moves with every allocation and release: guards remembered pointers INTO blocks (a new block can land on an old address)
  unsigned long long generation = 1;
  // *slot holds at least nbytes afterwards; a block that has to grow is replaced (contents are not kept) after
  // quiesce().  On failure *slot is NULL and nothing stays registered.
  int ensure(MemKind kind, void **slot, size_t nbytes) {
    auto it = blocks.find(slot);
    if (it != blocks.end() && it->second.bytes >= nbytes) return 0;
    if (it != blocks.end()) {
      if (int rc = quiesce()) return rc;
      drop(slot);
    }
    *slot = nullptr;
    if (int rc = alloc(kind, slot, nbytes)) return rc;
    blocks[slot] = Block{nbytes, kind};
    ++generation;
    return 0;
  }
  // free one block now (a table whose upload failed); the caller has made sure nothing queued uses it
  void drop(void **slot) {
    auto it = blocks.find(slot);
    if (it == blocks.end()) return;
    release(it->second.kind, *slot);
    *slot = nullptr;
    blocks.erase(it);
    ++generation;
  }
  // every block is freed and its slot set to NULL before the hooks run: a hook may clear a container slots live in
  void release_all() {
    for (auto &kv : blocks) {
      release(kv.second.kind, *kv.first);
      *kv.first = nullptr;
    }
    blocks.clear();
    ++generation;
    for (void (*hook)() : hooks) hook();
  }
};
}  // namespace psh
