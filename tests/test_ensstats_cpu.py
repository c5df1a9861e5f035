"""The ensemble statistics' host side (no GPU): the goldens' coverage, the member-order restatement against the
reference's goldens, signatures, argument checks, registration, the C symbol.

Yardstick: tests/helpers/ensstats.py restates ``mean`` and ``excprob`` as loops over the members in member order; it
reproduces every output of the unmodified reference in tests/golden/ensstats_reference.npz
(tools/make_golden_ensstats.py) bit for bit.  That is the contract csrc/ensstats.hip is written to; the device is held
to the same goldens in tests/test_ensstats_gpu.py.
"""

import inspect
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import ensstats as restated

PATH = os.path.join(GOLDEN, "ensstats_reference.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def case_names():
    return [str(c) for c in np.load(PATH)["cases"]]


def ops_of(golden, name):
    return json.loads(str(golden[name + "__ops"]))


def test_golden_covers_the_required_cases(golden):
    members, odd, counts, scalar = set(), False, set(), False
    mean_modes, prob_modes = set(), set()
    for name in case_names():
        X = golden[name + "__X"]
        assert X.dtype == np.float32 and X.ndim == 3
        members.add(X.shape[0])
        odd |= (X.shape[1] * X.shape[2]) % 2 == 1
        assert 48 <= X.shape[1] <= 97 and 75 <= X.shape[2] <= 131
        # NaN border, scattered NaN, both infinities, a column that is NaN in every member, dry pixels
        assert np.isnan(X[:, 0]).all() and np.isnan(X[:, :, -1]).all()
        inner = X[:, 2:-2, 2:-2]
        assert 0 < np.isnan(inner).mean() < 0.1 and np.isnan(inner).all(axis=0).any()
        assert np.isposinf(X).any() and np.isneginf(X).any()
        assert (inner == 0).mean() > 0.2
        for dtype in ("float32", "float64"):
            for i, op in enumerate(ops_of(golden, name)):
                assert "%s__%s__%d" % (name, dtype, i) in golden.files
        for op in ops_of(golden, name):
            kw = op["kwargs"]
            if op["fn"] == "mean":
                mean_modes.add((bool(kw.get("ignore_nan")), kw.get("X_thr") is not None))
            else:
                prob_modes.add(bool(kw["ignore_nan"]))
                thr = kw["X_thr"]
                if np.isscalar(thr):
                    scalar = True
                else:
                    counts.add(len(thr))
                # values exactly equal to a threshold
                for t in [thr] if np.isscalar(thr) else thr:
                    if t in (0.7, 2.5):
                        assert (X == np.float32(t)).any()
    assert members == {1, 2, 7, 20, 48} and odd and scalar and counts == {1, 3, 17}
    assert mean_modes >= {(False, False), (True, False), (False, True)} and prob_modes == {False, True}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", case_names())
def test_restatement_reproduces_the_reference(golden, name, dtype):
    X = golden[name + "__X"].astype(dtype)
    for i, op in enumerate(ops_of(golden, name)):
        want = golden["%s__%s__%d" % (name, dtype, i)]
        got = getattr(restated, op["fn"])(X, **op["kwargs"])
        assert got.dtype == want.dtype and got.shape == want.shape, op
        assert np.array_equal(got, want, equal_nan=True), op
        ok = ~np.isnan(want)  # and as bit patterns: signed zeros too (NumPy sums members that are all -0.0 to +0.0)
        bits = np.uint64 if want.dtype == np.float64 else np.uint32
        assert np.array_equal(got[ok].view(bits), want[ok].view(bits)), op
        if op["fn"] == "mean":
            assert want.dtype == X.dtype
        else:
            assert want.dtype == np.float64


def test_float32_threshold_is_compared_as_numpy_compares_it():
    """float32(0.7) < 0.7 as float64 numbers, but a float32 stack meets the Python float 0.7 as float32(0.7)."""
    x = np.full((3, 2, 2), np.float32(0.7))
    assert restated.compared_as(0.7, np.float32) == float(np.float32(0.7)) != 0.7
    assert restated.compared_as(0.7, np.float64) == 0.7
    assert np.all(restated.excprob(x, [0.7]) == (x >= 0.7).mean(axis=0))
    assert np.all(restated.excprob(x.astype(np.float64), [0.7]) == 0.0)
    assert restated.compared_as(np.float64(0.7), np.float32) == float(np.result_type(np.float32, np.float64(0.7)).type(0.7))


def test_signatures_equal_the_reference(golden):
    from pysteps_amd.postprocessing import ensemblestats

    assert str(inspect.signature(ensemblestats.mean)) == str(golden["signature_mean"])
    assert str(inspect.signature(ensemblestats.excprob)) == str(golden["signature_excprob"])
    assert str(inspect.signature(ensemblestats.products)) == (
        "(X, thresholds, *, mean=True, ignore_nan=False, mean_ignore_nan=False, mean_thr=None)")
    assert ensemblestats.EnsembleProducts.accepts_device is True
    assert not hasattr(ensemblestats, "banddepth")


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the HIP library fails the test: the checks must come first."""
    from pysteps_amd import _lib

    def refuse():
        raise AssertionError("the device was used before the argument checks")

    monkeypatch.setattr(_lib, "lib", refuse)


def test_dimension_errors_as_recorded(golden, no_device):
    from pysteps_amd.postprocessing import ensemblestats

    errors = json.loads(str(golden["errors"]))
    assert sorted((e["fn"], len(e["shape"])) for e in errors) == [("excprob", 1), ("excprob", 2), ("mean", 1), ("mean", 4)]
    for e in errors:
        assert e["type"] == "Exception"
        args = [1.0] if e["fn"] == "excprob" else []
        with pytest.raises(Exception) as err:
            getattr(ensemblestats, e["fn"])(np.zeros(e["shape"]), *args)
        assert type(err.value) is Exception and str(err.value) == e["message"]
    with pytest.raises(Exception, match="should be 3 or more. It was: 2"):
        ensemblestats.products(np.zeros((4, 5)), [1.0])
    with pytest.raises(ValueError):
        ensemblestats.EnsembleProducts([1.0], keep="disk")


def test_other_dtypes_go_to_the_reference(ref_pysteps, no_device):
    from pysteps.postprocessing import ensemblestats as ref

    from pysteps_amd.postprocessing import ensemblestats

    X = np.arange(4 * 5 * 6).reshape(4, 5, 6) % 7
    with pytest.warns(UserWarning, match="dtype int64"):
        got = ensemblestats.mean(X)
    assert np.array_equal(got, ref.mean(X))
    with pytest.warns(UserWarning, match="dtype float16"):
        got = ensemblestats.excprob(X.astype(np.float16), [2.0, 3.0])
    assert np.array_equal(got, ref.excprob(X.astype(np.float16), [2.0, 3.0]))


def test_register_adds_the_hip_names(ref_pysteps):
    from pysteps import postprocessing
    from pysteps.postprocessing import ensemblestats as ref

    from pysteps_amd import register
    from pysteps_amd.postprocessing import ensemblestats

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        added = register.register()
    assert "ensemblestats:mean_hip" in added and "ensemblestats:excprob_hip" in added
    assert postprocessing.get_method("mean_hip", "ensemblestats") is ensemblestats.mean
    assert postprocessing.get_method("excprob_hip", "ensemblestats") is ensemblestats.excprob
    assert postprocessing.get_method("mean", "ensemblestats") is ref.mean
    assert postprocessing.get_method("excprob", "ensemblestats") is ref.excprob
    assert postprocessing.get_method("banddepth", "ensemblestats") is ref.banddepth


def test_package_table():
    from pysteps_amd import postprocessing
    from pysteps_amd.postprocessing import ensemblestats

    assert postprocessing.get_method("mean_hip") is ensemblestats.mean
    assert postprocessing.get_method("EXCPROB_HIP") is ensemblestats.excprob
    with pytest.raises(ValueError):
        postprocessing.get_method("banddepth_hip")


def test_symbol_in_header_library_and_signatures():
    import ctypes

    from pysteps_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "pysteps_hip.h")).read()
    assert "int psh_ens_products_dev(" in header
    restype, argtypes = _lib.SIGNATURES["psh_ens_products_dev"]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert hasattr(ctypes.CDLL(build.build()), "psh_ens_products_dev")


def test_imports_without_pysteps_and_without_gpu():
    code = (
        "import sys\n"
        "class Block:\n"
        "    def find_spec(self, name, path=None, target=None):\n"
        "        if name == 'pysteps' or name.startswith('pysteps.'):\n"
        "            raise ImportError('pysteps is blocked in this test')\n"
        "sys.meta_path.insert(0, Block())\n"
        "import numpy as np\n"
        "from pysteps_amd import postprocessing\n"
        "from pysteps_amd.postprocessing import ensemblestats as es\n"
        "assert postprocessing.get_method('mean_hip') is es.mean\n"
        "try:\n"
        "    es.mean(np.zeros((2, 3, 4), dtype=np.int32))\n"
        "except NotImplementedError as exc:\n"
        "    assert 'pysteps is not importable' in str(exc)\n"
        "else:\n"
        "    raise AssertionError('an integer stack must raise without pysteps')\n"
        "assert not any(k == 'pysteps' or k.startswith('pysteps.') for k in sys.modules)\n"
        "print('ok')\n"
    )
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr
