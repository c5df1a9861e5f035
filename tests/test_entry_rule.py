"""The library's entry rule (pysteps_amd/csrc/entry.h), held from the source text (no GPU).

An entry point that needs the device begins with PSH_ENTER(c): the library lock, the psh_init check under it, the device
bind.  The parts of that sequence - the lock types, the context's mutex and `ready`, the bind - are written only at the
guard, in runtime.hip (psh_init / psh_shutdown are the mechanism, bind_device lives there), and where EXCEPTIONS says."""

import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest
from conftest import ROOT

from test_ownership_rule import CSRC, _enclosing_function

SPELLINGS = (
    r"PSH_REQUIRE_INIT",
    r"lock_guard<std::recursive_mutex>",
    r"unique_lock<std::recursive_mutex>",
    r"hipSetDevice",
    r"ctx\(\)\.ready",
    # what the guard is made of, taken directly
    r"\bc\.ready\b",
    r"\b[cp]\.mu\b",
    r"ctx\(\)\.mu\b",
    r"\bbind_device\(",
)
# Where they may still be written: file -> functions (None: anywhere in the file), with the reason.
EXCEPTIONS = {
    # the guard itself
    "entry.h": None,
    # psh_init / psh_shutdown are the mechanism and bind_device is defined here; psh_set_option("trim_cache") and
    # psh_free answer PSH_OK when the library is not up (they read `ready` under the lock)
    "runtime.hip": None,
    # a communicator is closed whether the library is up or not (psh_shutdown's hook calls it, too)
    "comm.hip": {"psh_comm_destroy"},
    # the pinned pool's own std::mutex (taken after the library lock, never the other way round) ...
    # ... and psh_host_free: PSH_OK after psh_shutdown, which took the pool's blocks; reads `ready` under the lock
    "hostpath.hip": {"pinned_alloc", "pinned_free", "pinned_release_cache", "psh_host_free"},
}
_SPELLING = re.compile("|".join(SPELLINGS))


def test_the_way_in_is_written_at_the_guard_and_in_the_listed_exceptions_only():
    sources = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(sources) > 30
    offenders, seen = [], set()
    for path in sources:
        name = os.path.basename(path)
        lines = open(path).read().split("\n")
        for i, line in enumerate(lines):
            code = line.split("//")[0]
            if not _SPELLING.search(code):
                continue
            allowed = EXCEPTIONS.get(name, set())
            if allowed is None:
                seen.add((name, None))
                continue
            where = _enclosing_function(lines, i)
            seen.add((name, where))
            if where not in allowed:
                offenders.append("%s:%d in %s: %s" % (name, i + 1, where, line.strip()))
    assert not offenders, offenders
    listed = {(name, fn) for name, fns in EXCEPTIONS.items() for fn in (fns if fns is not None else [None])}
    assert seen == listed, sorted(seen ^ listed, key=str)  # no stale row in the table


def test_psh_require_init_is_gone_and_the_guard_is_used():
    uses = 0
    for path in glob.glob(os.path.join(CSRC, "*")) + [os.path.join(ROOT, "include", "pysteps_hip.h")]:
        text = open(path).read()
        assert "PSH_REQUIRE_INIT" not in text, path
        uses += len(re.findall(r"^\s+PSH_ENTER\(\w+\);", text, flags=re.M))
    assert uses > 100, uses


def test_scratch_is_declared_after_the_guard():
    text = open(os.path.join(CSRC, "scratch.h")).read()
    assert "PSH_ENTER" in text and "lock_guard" not in text


def _fixed_address_space():
    """In the child, before the program starts: no address-space randomisation (what `setarch -R` does).  TSan's
    runtime maps its shadow memory at fixed places and gives up ("unexpected memory mapping") where the kernel
    randomises the program's addresses by more bits than that layout allows for."""
    ctypes.CDLL(None, use_errno=True).personality(0x0040000)  # ADDR_NO_RANDOMIZE


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_entry_selftest_under_the_sanitizers(tmp_path, sanitizer):
    """tests/helpers/entry_selftest.cpp: the guard over a Context of its own and a bind that counts its calls - not
    ready, ready, a failed bind, release and retake of the lock, a nested entry, and a thread that keeps entering while
    another clears `ready` under the lock as psh_shutdown does - as a program of its own, under ASan + UBSan and
    under TSan."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "entry_selftest")
    src = os.path.join(ROOT, "tests", "helpers", "entry_selftest.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", "-fsanitize=" + sanitizer,
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, preexec_fn=_fixed_address_space)
    assert run.returncode == 0 and "entry selftest: ok" in run.stdout, run.stdout + run.stderr[-3000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-3000:]
