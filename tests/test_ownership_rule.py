"""The library's ownership rule (pysteps_amd/csrc/registry.h, common.h), held from the source text (no GPU).

Everything the library allocates for its own lifetime goes through persistent_device / persistent_pinned and is
released by psh_shutdown through the registry; only the allocators themselves call the HIP allocation functions."""

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
