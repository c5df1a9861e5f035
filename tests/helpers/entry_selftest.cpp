// Stand-alone exercise of pysteps_amd/csrc/entry.h with no HIP underneath, meant to be built once with
// -fsanitize=address,undefined and once with -fsanitize=thread (tests/test_entry_rule.py does both): the Context, ctx(),
// fail() and a bind_device() that counts its calls are defined HERE.  `stream` stands for everything psh_shutdown takes
// away under the lock.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <future>
#include <thread>

#include "../../pysteps_amd/csrc/entry.h"

namespace psh {
struct Context {
  bool ready = false;
  int device = -1;
  int stream = 0;
  std::recursive_mutex mu;
};
Context &ctx() {
  static Context c;
  return c;
}
}  // namespace psh

namespace {
int g_binds = 0, g_bound = -1, g_fails = 0, g_bind_result = PSH_OK;
bool g_bind_saw_lock = false, g_probe_lock = true;  // the probe starts a thread: not in the two-thread loop

// true if another thread cannot take the library lock now
bool held() {
  return !std::async(std::launch::async, [] {
            std::recursive_mutex &mu = psh::ctx().mu;
            const bool got = mu.try_lock();
            if (got) mu.unlock();
            return got;
          }).get();
}
}  // namespace

int psh::fail(int code, const char *, ...) {
  ++g_fails;
  return code;
}
int psh::bind_device(int device) {
  ++g_binds;
  g_bound = device;
  if (g_probe_lock) g_bind_saw_lock = held();
  return g_bind_result;
}

namespace {

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

// an entry point's shape; 1000 + ... : what it saw after the guard let it in
int entry_point() {
  PSH_ENTER(c);
  if (!c.ready || c.stream == 0) return 1001;  // let in, but the library is not up: the guard failed
  if (!held()) return 1002;
  return PSH_OK;
}

// an entry point that waits: releases the lock around the wait and takes it back
int waiting_entry_point() {
  PSH_ENTER(c);
  const int stream = c.stream;
  lock.unlock();
  if (held()) return 1003;
  if (stream == 0) return 1004;
  lock.lock();
  if (!held()) return 1005;
  return c.ready ? PSH_OK : 1006;
}

void init(int device) {
  psh::Context &c = psh::ctx();
  std::lock_guard<std::recursive_mutex> g(c.mu);
  c.device = device;
  c.stream = 7;
  c.ready = true;
}
void shutdown() {
  psh::Context &c = psh::ctx();
  std::lock_guard<std::recursive_mutex> g(c.mu);
  c.stream = 0;
  c.ready = false;
}

int run() {
  // not ready: PSH_ENOTINIT through fail(), the bind is never called, the lock is free afterwards
  CHECK(entry_point() == PSH_ENOTINIT && g_binds == 0 && g_fails == 1 && !held());
  // ready: one bind, with the context's device, under the lock; the lock is held until the entry point returns
  init(3);
  CHECK(entry_point() == PSH_OK && g_binds == 1 && g_bound == 3 && g_bind_saw_lock && g_fails == 1 && !held());
  // a bind that fails: its code comes back, the lock is free
  g_bind_result = PSH_EHIP;
  CHECK(entry_point() == PSH_EHIP && g_binds == 2 && !held());
  g_bind_result = PSH_OK;
  // release and retake
  CHECK(waiting_entry_point() == PSH_OK && g_binds == 3 && !held());
  {  // the mutex is recursive: an entry point called with the lock held (the registry's quiesce) comes through
    std::lock_guard<std::recursive_mutex> g(psh::ctx().mu);
    CHECK(entry_point() == PSH_OK && g_binds == 4);
  }
  CHECK(!held());
  shutdown();
  CHECK(entry_point() == PSH_ENOTINIT && g_binds == 4 && g_fails == 2);

  // psh_shutdown against a thread that keeps entering: every call is either a complete entry (ready and the stream
  // seen under the lock) or PSH_ENOTINIT, never an entry into a library that is gone
  g_probe_lock = false;
  for (int round = 0; round < 20; ++round) {
    init(round);
    std::atomic<int> calls{0};
    std::atomic<bool> stop{false};
    int entered = 0, refused = 0, other = 0;
    std::thread caller([&] {
      while (!stop.load()) {
        psh::Context &c = psh::ctx();
        psh::Lock lock;
        const int rc = psh::enter(c, lock);
        if (rc == PSH_OK && c.ready && c.stream == 7 && lock.owns_lock()) {
          ++entered;
        } else if (rc == PSH_ENOTINIT) {
          ++refused;
        } else {
          ++other;
        }
        lock = psh::Lock();
        ++calls;
      }
    });
    while (calls.load() < 1) std::this_thread::yield();
    shutdown();
    const int seen = calls.load();  // the call in flight may have entered before the shutdown, the one after it did not
    while (calls.load() < seen + 2) std::this_thread::yield();
    stop.store(true);
    caller.join();
    CHECK(other == 0 && entered >= 1 && refused >= 1);
  }
  return 0;
}

}  // namespace

int main() {
  const bool ok = run() == 0;
  std::puts(ok ? "entry selftest: ok" : "entry selftest: FAILED");
  return ok ? 0 : 1;
}
