"""Every entry point of the C ABI called with all arguments zero / NULL (tests/test_entry_points_cpu.py).

call(lib, name) makes one such call.  Run as a program it loads the library WITHOUT psh_init, makes each call in a forked
child of its own - a crash is then a finding for that name, not the end of the run - and prints one JSON object
name -> return value, or "signal N" / "exit N" for a child that did not get to report.  No GPU is opened: the process
that forks has only dlopen'ed the library.
"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from pysteps_amd import _lib  # noqa: E402

# not status-code functions of a library state: the mechanism itself and the two string getters
NOT_CALLED = ("psh_init", "psh_shutdown", "psh_last_error", "psh_version")


def names():
    return [name for name in _lib.SIGNATURES if name not in NOT_CALLED]


def call(lib, name):
    """name(0, NULL, 0.0, ...): every ctypes type default-constructs to its zero."""
    return int(getattr(lib, name)(*[t() for t in _lib.SIGNATURES[name][1]]))


def call_forked(lib, name):
    rd, wr = os.pipe()
    pid = os.fork()
    if pid == 0:
        status = 1
        try:
            os.close(rd)
            os.write(wr, b"%d" % call(lib, name))
            status = 0
        finally:
            os._exit(status)
    os.close(wr)
    with os.fdopen(rd, "rb") as fh:
        text = fh.read()
    _, status = os.waitpid(pid, 0)
    if os.WIFSIGNALED(status):
        return "signal %d" % os.WTERMSIG(status)
    if os.WEXITSTATUS(status) != 0 or not text:
        return "exit %d" % os.WEXITSTATUS(status)
    return int(text)


def main():
    lib = _lib.load()
    print(json.dumps({name: call_forked(lib, name) for name in names()}, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
