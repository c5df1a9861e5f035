"""RainFARM downscaling without a GPU: the golden file, the float64 restatement, the method tables, the error texts and
the host-built table of kernel-weight partial sums (pysteps_amd/downscaling/rainfarm.py)."""

import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import rainfarm as rf


@pytest.fixture(scope="module")
def golden():
    return rf.load_golden()


def test_golden_matches_generator(ref_pysteps, golden):
    """tools/make_golden_rainfarm.py run again gives the committed file: inputs, arguments, texts and the exception
    type exactly; the reference's outputs and slopes within 5 x its own recorded deviation (NumPy's exp, log and
    transforms differ in the last bits between CPU models); each bar - a maximum over few error samples - within a
    factor of two."""
    sys.path.insert(0, ROOT)
    from tools import make_golden_rainfarm

    state = np.random.get_state()
    fresh = make_golden_rainfarm.generate()
    assert np.random.get_state()[2] == state[2] and np.array_equal(np.random.get_state()[1], state[1])
    assert sorted(fresh) == sorted(golden.files)
    for key in golden.files:
        a, b = np.asarray(fresh[key]), golden[key]
        if key == "versions":
            continue
        if key.startswith("deviation_"):
            assert 0.5 * float(b) <= float(a) <= 2.0 * float(b), (key, float(a), float(b))
        elif key.endswith("__out"):
            assert a.shape == b.shape and rf.scaled_diff(a, b) <= rf.BAR_FACTOR * float(golden["deviation_field"]), key
        elif key.endswith("__alpha"):
            assert abs(float(a) - float(b)) <= rf.BAR_FACTOR * float(golden["deviation_alpha"]), key
        elif key.endswith("__g"):
            assert abs(float(a) - float(b)) <= 1e-12 * float(b), key
        else:
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), key
    assert os.path.getsize(rf.GOLDEN_FILE) < 1 << 20


def test_restatement_reproduces_goldens(golden):
    """The float64 restatement (the reference's NumPy / SciPy calls on redrawn uniforms) against every stored output,
    bar 5 x deviation_field of the case's largest value."""
    bar = rf.BAR_FACTOR * float(golden["deviation_field"])
    for name, shape, ds, kernel, _, seed in rf.CASES:
        u = rf.draw(seed, (shape[0] * ds, shape[1] * ds))
        got = rf.pipeline(golden[name + "__precip"], u, ds, float(golden[name + "__alpha"]), kernel)
        s = int(golden[name + "__stride"])
        want = golden[name + "__out"]
        diff = rf.scaled_diff(got[::s, ::s], want)
        print("%s: restatement vs golden %.3g (bar %.3g), bit-equal: %s" % (name, diff, bar, np.array_equal(got[::s, ::s], want)))
        assert diff <= bar, name


def test_get_method_names():
    from pysteps_amd import downscaling
    from pysteps_amd.downscaling.rainfarm import downscale

    assert downscaling.get_method("rainfarm") is downscale
    assert downscaling.get_method("rainfarm_hip") is downscale
    assert downscaling.get_method("RainFARM_HIP") is downscale
    with pytest.raises(ValueError):
        downscaling.get_method("nearest")


def test_register_adds_rainfarm_hip(ref_pysteps):
    import pysteps.downscaling.interface as ds_if
    from pysteps.downscaling import rainfarm as ref_rainfarm

    from pysteps_amd import register
    from pysteps_amd.downscaling.rainfarm import downscale

    stock = ds_if._downscale_methods["rainfarm"]
    try:
        added = register.register()
        assert "downscaling:rainfarm_hip" in added
        assert ds_if.get_method("rainfarm_hip") is downscale
        assert ds_if.get_method("rainfarm") is stock is ref_rainfarm.downscale
    finally:
        ds_if._downscale_methods.pop("rainfarm_hip", None)


def test_error_texts(golden):
    """The reference's three ValueErrors, raised before any device work (no GPU here)."""
    import json

    from pysteps_amd.downscaling.rainfarm import downscale

    messages = json.loads(str(golden["messages"]))
    with pytest.raises(ValueError) as e:
        downscale(np.array([[1.0, np.nan], [0.0, 2.0]]), 2)
    assert str(e.value) == messages["nonfinite"]
    with pytest.raises(ValueError) as e:
        downscale(np.ones((4, 4)), 0)
    assert str(e.value) == messages["ds_factor"]
    with pytest.raises(ValueError) as e:
        downscale(np.ones((4, 4)), 2.0)
    assert str(e.value) == messages["ds_factor"]
    with pytest.raises(ValueError) as e:
        downscale(rf.field((4, 4), 1) + 1.0, 2, alpha=1.0, kernel_type="box")
    assert str(e.value) == messages["kernel_type"]


@pytest.mark.parametrize("ds,radius", [(1, 1), (2, 1), (3, 2), (4, 2), (8, 5), (16, 9)])
def test_kernel_radii(ds, radius):
    from pysteps_amd.downscaling.rainfarm import kernel_radius, make_kernel

    assert kernel_radius(ds) == radius == rf.kernel_radius(ds)
    for kind in ("gaussian", "tophat", "uniform"):
        k = make_kernel(kind, ds)
        assert k.shape == (2 * radius + 1, 2 * radius + 1)
        assert np.array_equal(k, rf.make_kernel(kind, ds))


@pytest.mark.parametrize("kind", ["gaussian", "tophat"])
@pytest.mark.parametrize("ds,shape", [(1, (5, 4)), (2, (3, 4)), (3, (4, 3)), (8, (3, 4)), (16, (2, 3))])
def test_weight_table_against_tap_loop(kind, ds, shape):
    """The balanced average summed over coarse cells from the table equals the plain tap loop over the expanded plane
    (helpers/rainfarm.py ``convolve_same_direct``, float64) within ((2r+1)^2 - 1) 2^-53 of the plane's largest value:
    the same products summed in another order."""
    from pysteps_amd.downscaling.rainfarm import make_kernel, weight_table

    kernel = make_kernel(kind, ds)
    table, amin = weight_table(kernel, ds)
    na = table.shape[2]
    r = rf.kernel_radius(ds)
    assert table.shape == (ds, ds, na, na) and amin <= 0 <= amin + na - 1
    assert np.abs(table.sum(axis=(2, 3)) - 1.0).max() <= (2 * r + 1) ** 2 * 2.0 ** -53
    m, n = shape
    low = np.random.RandomState(7 + ds).rand(m, n) + 0.25
    fine = np.kron(low, np.ones((ds, ds)))
    want = rf.balanced_average(fine, kernel, direct=True)
    got = np.empty_like(fine)
    for y in range(m * ds):
        for x in range(n * ds):
            I, py, J, px = y // ds, y % ds, x // ds, x % ds
            sp = sw = 0.0
            for a in range(na):
                for b in range(na):
                    II, JJ = I + a + amin, J + b + amin
                    if 0 <= II < m and 0 <= JJ < n:
                        sp += table[py, px, a, b] * low[II, JJ]
                        sw += table[py, px, a, b]
            got[y, x] = sp / sw
    bound = ((2 * r + 1) ** 2 - 1) * 2.0 ** -53
    assert np.abs(got - want).max() <= bound * np.abs(want).max()
