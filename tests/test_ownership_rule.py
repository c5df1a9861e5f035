"""The library's ownership rule (pysteps_amd/csrc/registry.h, common.h), held from the source text (no GPU).

Everything the library allocates for its own lifetime goes through persistent_device / persistent_pinned and is
released by psh_shutdown through the registry; only the allocators themselves call the HIP allocation functions.  A block
from psh_malloc that lives for one call is owned by a psh::Scratch (scratch.h); psh_free is spelled out only where the
release does more than free, or where a handle keeps the block beyond the call."""

import glob
import os
import re
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "pysteps_amd", "csrc")
# runtime.hip: the registry's allocator and psh_malloc; hostpath.hip: the pinned pool; rng.hip: caller-owned handles
ALLOCATORS = {"runtime.hip", "hostpath.hip", "rng.hip"}
CALLS = ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(")


def test_only_the_allocators_call_the_hip_allocation_functions():
    sources = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(sources) > 20
    offenders = []
    for path in sources:
        if os.path.basename(path) in ALLOCATORS:
            continue
        text = open(path).read()
        offenders += ["%s: %s" % (os.path.basename(path), c) for c in CALLS if c in text]
    assert not offenders, offenders


def test_fft_release_is_gone():
    for path in glob.glob(os.path.join(CSRC, "*")):
        assert "fft_release" not in open(path).read(), path


def test_shutdown_has_no_subsystem_lines():
    """psh_shutdown: lock, wait for both streams, the registry's release, the main stream, the Context fields."""
    text = open(os.path.join(CSRC, "runtime.hip")).read()
    body = re.search(r"int psh_shutdown\(void\) \{\n(.*?)\n\}\n", text, flags=re.S).group(1)
    assert "release_all()" in body
    for word in ("fft", "mask_any", "pinned_release", "release_cache", "hipFree", "hipHostFree", "comm", "lk_"):
        assert word not in body, word


def test_registry_selftest_under_the_sanitizers(tmp_path):
    """tests/helpers/registry_selftest.cpp: the registry with malloc underneath - register, grow, a failed regrow,
    drop, release, register again, release again - as a program of its own under ASan + UBSan."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "registry_selftest")
    src = os.path.join(ROOT, "tests", "helpers", "registry_selftest.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "registry selftest: ok" in run.stdout, run.stdout + run.stderr[-3000:]


def test_scratch_selftest_under_the_sanitizers(tmp_path):
    """tests/helpers/scratch_selftest.cpp: psh::Scratch over malloc / free with a live-block counter - scope exit, a
    failed alloc, early returns, reset, release, adoption, moves - as a program of its own under ASan + UBSan."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "scratch_selftest")
    src = os.path.join(ROOT, "tests", "helpers", "scratch_selftest.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "scratch selftest: ok" in run.stdout, run.stdout + run.stderr[-3000:]


# Where psh_free( may still be written: file -> functions (None: anywhere in the file).
MANUAL_FREES = {
    # the allocator: psh_free is defined (and described) here
    "runtime.hip": None,
    # its cleanup waits for the download stream and destroys an event and a ring before it frees
    "hostpath.hip": None,
    # synchronises the stream before the frees: the blocks were filled from buffers on its stack
    "idw.hip": {"psh_idw_host"},
    # PyramidSet is a handle: it owns its block (raw pointer) from lk_pyramids_on until psh_lk_pyramids_free
    "lk.hip": {"lk_pyramids_on", "psh_lk_pyramids_free"},
    # PmPlan is a handle: it owns its block (raw pointer) from plan_create until plan_destroy
    "probmatch.hip": {"psh_probmatch_plan_create", "psh_probmatch_plan_destroy"},
}
_DEFINITION = re.compile(r"^(?!namespace|using|struct|class|template|typedef|#)[A-Za-z_][^;]*?\b(\w+)\($")


def _enclosing_function(lines, index):
    for i in range(index, -1, -1):
        head = lines[i]
        if head[:1].isspace() or not head.strip() or "(" not in head:
            continue
        m = _DEFINITION.match(head[:head.index("(") + 1])
        if m:
            return m.group(1)
    return None


def test_psh_free_is_written_only_where_the_release_does_more_than_free():
    sources = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(sources) > 20
    offenders, seen = [], set()
    for path in sources:
        name = os.path.basename(path)
        lines = open(path).read().split("\n")
        for i, line in enumerate(lines):
            if "psh_free(" not in line:
                continue
            seen.add(name)
            allowed = MANUAL_FREES.get(name, set())
            if allowed is None:
                continue
            where = _enclosing_function(lines, i)
            if where not in allowed:
                offenders.append("%s:%d in %s" % (name, i + 1, where))
    assert not offenders, offenders
    assert seen == set(MANUAL_FREES), sorted(seen ^ set(MANUAL_FREES))  # no stale entry in the list


def test_no_lambda_exists_only_to_reach_a_free():
    """`auto run = [&]() -> int { ... }; rc = run(); psh_free(...)`: the wrapper psh::Scratch made unnecessary."""
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        lines = open(path).read().split("\n")
        for i, line in enumerate(lines):
            m = re.search(r"auto (\w+) = \[&\]\(\) -> int \{", line)
            if not m:
                continue
            call = m.group(1) + "()"
            for j in range(i + 1, len(lines)):
                if call in lines[j]:
                    after = "\n".join(lines[j:j + 4])
                    assert "psh_free" not in after, "%s:%d" % (os.path.basename(path), j + 1)
    for name in ("DevBlock", "struct Release"):
        for path in glob.glob(os.path.join(CSRC, "*")):
            assert name not in open(path).read(), (name, path)
