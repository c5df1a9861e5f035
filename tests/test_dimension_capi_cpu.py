"""The C ABI of csrc/dimension.hip (no GPU): include/pysteps_hip_dimension.h, the ctypes table
``pysteps_amd._lib.DIMENSION_SIGNATURES`` and the built library name the same entry points; every one of them begins
with the entry guard and answers PSH_ENOTINIT before psh_init.  What tests/test_capi_symbols.py and
tests/test_entry_points_cpu.py hold for pysteps_hip.h and ``_lib.SIGNATURES``, for the table these entry points live in."""

import ctypes
import json
import os
import re
import subprocess
import sys

from conftest import ROOT

from pysteps_amd import _lib

HEADER = os.path.join(ROOT, "include", "pysteps_hip_dimension.h")
NAMES = ["psh_accumulate_step_dev", "psh_aggregate_axis_dev", "psh_aggregate_space_dev", "psh_field_min_dev", "psh_window_copy_dev"]
# name -> what it answers with every argument zero / NULL on a library that is not initialised: the guard comes first
EXPECTED = {name: _lib.PSH_ENOTINIT for name in NAMES}


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(psh_[a-z0-9_]+)\s*\(", text)))


def test_header_table_and_library_name_the_same_entry_points():
    assert _declared(HEADER) == NAMES == sorted(_lib.DIMENSION_SIGNATURES)
    assert not set(NAMES) & set(_lib.SIGNATURES)  # one table each
    main = open(os.path.join(ROOT, "include", "pysteps_hip.h")).read()
    assert '#include "pysteps_hip_dimension.h"' in main  # a user of the library still includes one header
    from pysteps_amd import build

    lib = ctypes.CDLL(build.build())
    assert not [n for n in NAMES if not hasattr(lib, n)]
    loaded = _lib.load()
    for name, (restype, argtypes) in _lib.DIMENSION_SIGNATURES.items():
        fn = getattr(loaded, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_argument_counts_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (_, argtypes) in _lib.DIMENSION_SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(params.split(",")) == len(argtypes), name


def test_every_entry_point_begins_with_the_guard():
    text = open(os.path.join(ROOT, "pysteps_amd", "csrc", "dimension.hip")).read()
    for name in NAMES:
        body = text[text.index('extern "C" int %s(' % name):]
        first = body[body.index("{") + 1:].lstrip().split("\n")[0]
        assert first == "PSH_ENTER(c);", (name, first)


def test_what_the_entry_points_answer_before_psh_init():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "dimension_entry.py")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert json.loads(run.stdout.strip().split("\n")[-1]) == EXPECTED
