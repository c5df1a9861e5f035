"""Every kernel path of pysteps_amd/csrc/probmatch.hip at the smallest input that reaches it, through all three entry
routes on resident arrays - psh_probmatch_dev, psh_probmatch_plan_create + psh_probmatch_planned_dev, and
psh_probmatch_async_dev with its status word - against oracle.nonparam_match_empirical_cdf.

The cases and the proof that each reaches its path are in tests/helpers/probmatch_cases.py and
tests/test_probmatch_cases_cpu.py.  The bar is np.array_equal: the operation selects and copies float64 values, and the
one computed number, the percentile p, is numpy's expression in numpy's order."""

import ctypes

import numpy as np
import pytest

from helpers import probmatch_cases as pc
from oracle import probmatch as oracle

pytestmark = pytest.mark.gpu

ROUTES = ("direct", "planned", "async")


class Routes:
    """The three routes for one target: the plan is made once, as the member loop does."""

    def __init__(self, target):
        from pysteps_amd import _lib
        from pysteps_amd.device import DeviceArray

        self._lib, self.lib, self.DeviceArray = _lib, _lib.lib(), DeviceArray
        self.n = target.size
        self.d_target = DeviceArray.from_host(target)
        self.plan = ctypes.c_void_p()
        _lib.check(self.lib.psh_probmatch_plan_create(self.d_target.ptr, self.n, ctypes.byref(self.plan)))
        self.status = DeviceArray((1,), np.int32)

    def close(self):
        self._lib.check(self.lib.psh_probmatch_plan_destroy(self.plan))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def run(self, route, initial):
        """(return code, field or None when the route declined)"""
        d_i, d_o = self.DeviceArray.from_host(initial), self.DeviceArray((self.n,), np.float64)
        if route == "direct":
            rc = self.lib.psh_probmatch_dev(d_i.ptr, self.d_target.ptr, self.n, d_o.ptr)
        elif route == "planned":
            rc = self.lib.psh_probmatch_planned_dev(self.plan, d_i.ptr, self.n, d_o.ptr, None)
        else:
            self._lib.check(self.lib.psh_probmatch_async_dev(d_i.ptr, self.d_target.ptr, self.n, d_o.ptr, self.status.ptr))
            rc = self.lib.psh_probmatch_status(int(self.status.to_host()[0]))
        return rc, (d_o.to_host() if rc == 0 else None)


def _assert_every_route_equals(routes, initial, want, what):
    for route in ROUTES:
        rc, got = routes.run(route, initial)
        assert rc == 0, (what, route, rc)
        wrong = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
        assert wrong.size == 0, "%s, %s: %d of %d pixels differ, the first at %d: %r for %r" % (
            what, route, wrong.size, want.size, wrong[0], got[wrong[0]], want[wrong[0]])
        assert np.array_equal(got, want), (what, route)


@pytest.mark.parametrize("name", pc.with_outcome("handled"))
def test_handled_cases_equal_the_oracle_on_every_route(name):
    case = pc.get(name)
    with Routes(case.target) as routes:
        _assert_every_route_equals(routes, case.initial, pc.expected(name), name)


@pytest.mark.parametrize("name", ["probe_sorted_target", "probe_initial_ranks"])
def test_probes_say_which_half_is_wrong(name):
    """probe_sorted_target: the output, un-permuted, is the sorted target element for element (holds tw in full, whatever
    the ranks of the initial array do with a permutation).  probe_initial_ranks: the output is the stable rank of every
    wet pixel and 0 on the dry ones (holds the ranks, with a target whose sorted form is the ramp)."""
    case = pc.get(name)
    want = pc.probe_expected(case)
    with Routes(case.target) as routes:
        _assert_every_route_equals(routes, case.initial, want, name)


@pytest.mark.parametrize("with_nan", [False, True])
def test_every_pair_of_wet_counts_up_to_nine_pixels(with_nan):
    """Every branch of pm_threshold (tests/test_probmatch_cases_cpu.py shows the coverage), the NaNs of the target
    counted as zeros in the second run."""
    for n in pc.SMALL_N:
        for initial, target, pair in pc.wet_count_pairs(n, with_nan):
            want = oracle.nonparam_match_empirical_cdf(initial, target)
            with Routes(target) as routes:
                _assert_every_route_equals(routes, initial, want, (n, pair, pc.threshold_branch(n, *pair)))


@pytest.mark.parametrize("name", pc.with_outcome("declined"))
def test_declined_cases_are_declined_on_every_route_and_answered_by_the_reference(ref_pysteps, name):
    from pysteps.postprocessing.probmatching import nonparam_match_empirical_cdf as ref

    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.postprocessing.probmatching import nonparam_match_empirical_cdf

    case = pc.get(name)
    ramp = np.random.default_rng(5).permutation(case.initial.size).astype(np.float64)  # handled on either side
    with Routes(case.target) as routes:  # a plan carries the target's verdict: making it succeeds
        for route in ROUTES:
            rc, _ = routes.run(route, case.initial)
            assert rc == _lib.PSH_EUNSUPPORTED, (name, route, rc)
        if name.endswith("_initial"):  # the next call on the same plan and stream, with an array the kernels handle
            _assert_every_route_equals(routes, ramp, oracle.nonparam_match_empirical_cdf(ramp, case.target), name + ", then a ramp")
        else:  # the target itself is declined, whatever the initial array
            for route in ROUTES:
                assert routes.run(route, ramp)[0] == _lib.PSH_EUNSUPPORTED, (name, route)
    if name.endswith("_target"):  # the next call on the same stream with a target the kernels handle
        with Routes(ramp) as routes:
            _assert_every_route_equals(routes, case.initial, oracle.nonparam_match_empirical_cdf(case.initial, ramp),
                                       name + ", then a ramp as the target")
    want = ref(case.initial, case.target)
    resident = nonparam_match_empirical_cdf(DeviceArray.from_host(case.initial), DeviceArray.from_host(case.target))
    assert isinstance(resident, DeviceArray) and np.array_equal(resident.to_host(), want)
    assert np.array_equal(nonparam_match_empirical_cdf(case.initial, case.target), want)


@pytest.mark.parametrize("name", pc.with_outcome("degenerate"))
def test_degenerate_scales_give_the_oracles_field_or_a_decline(name):
    """max - min infinite (scale 0, (v - z) * scale NaN for the far values) and a denormal range (scale inf): a route
    may decline, it must never return another field than the oracle's."""
    from pysteps_amd import _lib

    case = pc.get(name)
    with Routes(case.target) as routes:
        for route in ROUTES:
            rc, got = routes.run(route, case.initial)
            print(name, route, "rc", rc)
            assert rc in (0, _lib.PSH_EUNSUPPORTED), (name, route, rc)
            if rc == 0:
                assert np.array_equal(got, pc.expected(name)), (name, route)


def _order_statistic(values, index):
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    got, d_values = ctypes.c_double(), DeviceArray.from_host(values)
    _lib.check(_lib.lib().psh_order_statistic_dev(d_values.ptr, values.size, index, ctypes.byref(got)))
    return got.value


@pytest.mark.parametrize("name", ["hash_overflow_64x64", "bucket_257_target"])
def test_order_statistics_of_a_target(name):
    target = pc.get(name).target
    ranked = np.sort(target)
    n, zeros = target.size, int((target == target.min()).sum())
    crowd = np.flatnonzero(np.floor(ranked) == np.floor(ranked[n // 2]))  # the bucket of the median: the crowded one
    if name == "bucket_257_target":
        crowd = np.flatnonzero(np.floor(ranked) == 100.0)
        assert crowd.size == 257
    for index in sorted({0, zeros - 1, zeros, int(crowd[0]), int(crowd[-1]), n - 1}):
        assert _order_statistic(target, index) == ranked[index], (name, index)
