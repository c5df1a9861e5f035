"""The yardstick of tests/helpers/outliers.py and the conditions its cases must meet (no GPU).

tests/test_outliers_gpu.py holds the three kernels of csrc/sparse_qc.hip to EXACT flag equality with that yardstick.
That is only fair where the inputs keep every verdict away from the threshold and every selected neighbour set away
from a rounding boundary; this module asserts those conditions for every case (a case that misses one gets another
seed, never another bound), checks the yardstick against the reference's stored outputs, the host implementation and
the unmodified reference, and shows that the cases can tell the kernels' likely mistakes apart.

Not an outlier by rank: with two neighbours (k = 2, or three vectors in all) the covariance has rank 1 in exact
arithmetic.  The reference inverts it all the same and returns whatever the rounding residue of the determinant
gives; the host implementation used to flag 2 of the 3 vectors of ``cont-n3-k30`` and raised ``LinAlgError`` on
``chunks-n700-k2``, the kernels flagged at random.  Yardstick, host and kernels now say "singular" there.
"""

import json
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import outliers as ho
from pysteps_amd.utils import cleansing

MARGINS = os.path.join(GOLDEN, "outliers_margins.json")


def _host(case):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cleansing.detect_outliers(case.uv, case.thr, case.xy, case.k)


def test_case_ids_name_the_kernel():
    assert len(set(ho.NAMES)) == len(ho.NAMES) == len(ho.IDS)
    for name, cid in zip(ho.NAMES, ho.IDS):
        assert cid == ho.case(name).id
    assert {ho.case(n).kernel for n in ho.NAMES} == {"sorted16", "sorted32", "rescan"}
    assert [ho.kernel_of(n) for n in (1024, 1025, 2048, 2049, 8192)] == [
        "sorted16", "sorted32", "sorted32", "rescan", "rescan"]


def test_yardstick_reproduces_the_stored_reference_outputs():
    """Exactly where no tie sits at the kk-th place; cKDTree's tie order is not the kernels', so with ties the
    bound of tests/test_idw_gpu.py (at most max(1, 1 %) flags) stands."""
    exact = 0
    z = np.load(os.path.join(GOLDEN, "sparse_reference.npz"))
    stored = [(z[c + "/xy"], z[c + "/uv"], z[c + "/outliers"]) for c in ("a", "b", "c")]
    z = np.load(os.path.join(GOLDEN, "cleansing_reference.npz"))
    stored += [(z["L%d/xy" % L], z["L%d/uv" % L], z["L%d/outliers_local" % L]) for L in (2, 5, 31, 32, 700)]
    for xy, uv, want in stored:
        got = ho.oracle_flags(xy, uv, 30)
        ties = ho.tie_rows(xy, 30).any()
        diff = int(np.count_nonzero(got != want))
        print("%d vectors: ties %s, %d flags differ" % (len(xy), ties, diff))
        if not ties:
            exact += 1
            assert diff == 0
        assert diff <= max(1, 0.01 * want.size)
    assert exact >= 3


@pytest.mark.parametrize("name", [n for n in ho.NAMES if ho.case(n).tie_free])
def test_yardstick_equals_the_host_implementation(name):
    case, exp = ho.case(name), ho.expected(name)
    assert not ho.tie_rows(case.xy, case.k, exp.rows).any()
    assert np.array_equal(_host(case)[exp.rows], exp.flags)


@pytest.mark.parametrize("name", ho.NAMES)
def test_input_conditions(name):
    case, exp = ho.case(name), ho.expected(name)
    rec = ho.recorded(name)
    print(name, rec)
    assert case.n <= ho.MAX_N and case.thr == ho.THR
    assert rec["margin"] >= ho.MIN_MARGIN
    assert rec["formula_dev"] <= ho.MAX_FORMULA_DEV
    assert exp.singular_agrees and np.array_equal(exp.flags64, exp.flags)
    assert ho.fragile_keys(case.xy, case.k, exp.rows) == 0
    if case.n > ho.SAMPLE_ABOVE:
        assert len(exp.rows) >= ho.SAMPLE_ROWS and {0, 63, 64, case.n - 1} <= set(exp.rows.tolist())
    else:
        assert len(exp.rows) == case.n
    if case.kind == "collinear" or min(case.n, case.k + 1) - 1 < ho.MIN_NEIGHBOURS:
        assert rec["flagged"] == 0 and rec["singular"] == len(exp.rows)
    elif case.n >= 31:
        assert rec["singular"] == 0 and rec["flagged"] >= 1
    if case.kind == "lattice":
        assert np.array_equal(case.xy, np.round(case.xy)) and case.xy.min() >= 0
        assert 2 * case.xy.max() ** 2 < 2 ** 24  # every squared distance exact in float32
        assert case.n - len(np.unique(case.xy, axis=0)) >= 0.05 * case.n
        assert rec["tie_share"] >= 0.01
    with open(MARGINS) as f:
        kept = json.load(f)[name]
    for key, val in rec.items():
        if key in ("margin", "tie_share"):
            assert kept[key] == pytest.approx(val, rel=1e-6), key
        elif key == "formula_dev":  # rounding noise itself: the order of magnitude is what is recorded
            assert kept[key] <= ho.MAX_FORMULA_DEV
        else:
            assert kept[key] == val, key


def test_margins_file_lists_exactly_the_cases():
    with open(MARGINS) as f:
        assert sorted(json.load(f)) == sorted(ho.NAMES)


def test_near_tie_case_bites():
    case = ho.case("neartie-n600-k8")
    rows = ho.near_tie_rows(case)
    assert len(rows) >= ho.NEAR_TIE_MIN
    by32, by64 = ho.knn_by_key(case.xy, case.k, rows), ho.knn_by_float64(case.xy, case.k, rows)
    for r, a, b in zip(rows, by32.tolist(), by64.tolist()):
        assert len(set(a) ^ set(b)) == 2, r  # one neighbour swapped
        gone, = set(b) - set(a)
        kept, = set(a) - set(b)
        assert kept < gone  # the float32 key took the lower index, the farther vector


def test_large_coordinates_shift_exactly():
    shifted, base = ho.case("large-n1025-k30"), ho.large_base()
    assert np.array_equal(shifted.xy - ho.LARGE_SHIFT, base.xy) and np.array_equal(shifted.uv, base.uv)
    assert np.array_equal(ho.expected("large-n1025-k30").flags, ho.Expected(base).flags)


def _differs(name, mistake):
    rows, wrong = ho.mistaken_flags(ho.case(name), mistake)
    exp = ho.expected(name)
    return int(np.count_nonzero(wrong != exp.flags[np.isin(exp.rows, rows)]))


def test_cases_tell_the_likely_mistakes_apart():
    """The device returns flags only, so a wrong neighbour set shows where it moves a flag.  Under each deliberate
    mistake the yardstick's own flags must change in at least one case per kernel that the mistake can reach."""
    chunked = [n for n in ho.NAMES if n.startswith("chunks-") and ho.case(n).k + 1 > 64]
    for kernel in ("sorted16", "sorted32", "rescan"):
        assert sum(_differs(n, "second_chunk") for n in chunked if ho.case(n).kernel == kernel) >= 1, kernel
    for name in ho.NAMES:
        if ho.case(name).kind == "lattice":
            assert _differs(name, "higher_index") >= 1, name
    assert _differs("neartie-n600-k8", "float64_key") >= ho.NEAR_TIE_MIN
    assert _differs("neartie-n600-k8", "higher_index") >= ho.NEAR_TIE_MIN
    for name in ("last-n1025-k30", "last-n2049-k30"):
        assert _differs(name, "last_vector_missing") >= 1, name


def test_reference_and_host_call_collinear_vectors_singular(ref_pysteps):
    """v = u, v = 2u, v = -u, v = 0 and identical vectors: the unmodified reference warns "Singular matrix" and
    flags nobody; so does the host implementation."""
    from pysteps.utils import cleansing as ref_cleansing

    for name in ho.NAMES:
        case = ho.case(name)
        if case.kind != "collinear" or case.n > 1500:
            continue
        with pytest.warns(UserWarning, match="Singular matrix"):
            ref = ref_cleansing.detect_outliers(case.uv, case.thr, case.xy, case.k)
        assert not np.asarray(ref).any(), name
        with pytest.warns(UserWarning, match="Singular matrix"):
            host = cleansing.detect_outliers(case.uv, case.thr, case.xy, case.k)
        assert not host.any(), name
