// The one way into the library: every entry point that needs the device begins with PSH_ENTER(c).  The exceptions -
// entry points for which "not initialised" is no error, and the mechanism itself - are listed with their reasons in
// tests/test_entry_rule.py.  Host code only; no HIP header needed.
#pragma once

#include <mutex>

#include "../../include/pysteps_hip.h"

namespace psh {

struct Context;  // common.h
Context &ctx();
int fail(int code, const char *fmt, ...);
int bind_device(int device);  // runtime.hip: PSH_OK, or PSH_EHIP with the message set

// Owns the library lock for the call.  An entry point that waits for the device (a stream or an event) releases it
// around the wait with unlock() / lock(), so that a waiting thread does not hold the library.
using Lock = std::unique_lock<std::recursive_mutex>;

// (a template only so that this header needs no definition of Context)
template <class C> int enter(C &c, Lock &lock) {
  // 1. The lock first: c.ready, c.stream and every block of the registry are written by psh_init / psh_shutdown under
  //    it.  Checked before the lock, `ready` could be true for a thread that then waits while another thread's
  //    psh_shutdown destroys the stream, and goes on with what is gone.
  lock = Lock(c.mu);
  // 2. So a call that races with psh_shutdown either runs completely before it or returns this.
  if (!c.ready) return fail(PSH_ENOTINIT, "psh_init() has not been called");
  // 3. HIP's current device belongs to the calling thread, not to the process: a thread that has not made a call yet,
  //    or that has used another device since, would allocate and launch elsewhere.  So every call binds.
  return bind_device(c.device);
}

}  // namespace psh

// Declares `psh::Context &c` and the `psh::Lock lock` that holds c.mu until the function returns.
#define PSH_ENTER(c)                                      \
  [[maybe_unused]] ::psh::Context &c = ::psh::ctx();      \
  ::psh::Lock lock;                                       \
  if (int _rc = ::psh::enter(c, lock)) return _rc
