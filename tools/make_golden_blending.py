"""Golden vectors for the linear and salient blending (``pysteps_amd.blending``), written by the UNMODIFIED reference.

    python tools/make_golden_blending.py    (-> tests/golden/blending_reference.npz, tests/golden/blending_bars.json)

Runs pysteps/blending/linear_blending.py ``forecast`` of the reference package that ``oracle.build_ref`` prepares under
oracle/_ref.  A stub name added to the reference's ``_nowcast_methods`` returns a prepared stack, so the blend stage is
isolated from the extrapolator; metadata is ``{"transform": None, "unit": "mm/h"}``, which the reference's unit
conversion copies through.  Per case of tests/helpers/blending.py the file holds the arguments (JSON), the SHA-256 of
the inputs the recipe gave, and the reference's output with ``saliency`` off and on; the exception type of a call whose
NWP stack is shorter than the nowcast; and the reference's float64 dB inverse of the helper's 0.25 dB field.
blending_bars.json holds the largest deviation of that inverse from the long-double restatement, in units in the last
place of the result, and the NumPy version.  Needs the reference; never runs on the GPU machine.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "tests", "golden", "blending_reference.npz")
BARS = os.path.join(ROOT, "tests", "golden", "blending_bars.json")
META = {"transform": None, "unit": "mm/h"}


def main():
    import warnings

    from helpers import blending as hb
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    import pysteps.nowcasts.interface as now_if
    from pysteps.blending import linear_blending as ref
    from pysteps.utils import conversion

    prepared = {}
    now_if._nowcast_methods["prepared_stack"] = lambda precip, velocity, timesteps, **kw: prepared["stack"].copy()

    def run(nowcast, nwp, kwargs, saliency):
        prepared["stack"] = nowcast
        nwp_before = nwp.copy()
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            res = ref.forecast(np.zeros(nowcast.shape[-2:]), dict(META), None, kwargs["timesteps"], kwargs["timestep"],
                               "prepared_stack", precip_nwp=nwp, precip_nwp_metadata=dict(META),
                               start_blending=kwargs["start_blending"], end_blending=kwargs["end_blending"],
                               fill_nwp=kwargs["fill_nwp"], saliency=saliency)
        assert np.array_equal(nwp, nwp_before, equal_nan=True)
        return res

    out = {"versions": np.array(json.dumps({"numpy": np.__version__})), "cases": np.array(sorted(hb.CASES))}
    for name in sorted(hb.CASES):
        nowcast, nwp, kwargs = hb.make_case(name)
        out[name + "__args"] = np.array(json.dumps(kwargs))
        out[name + "__sha256"] = np.array(hb.digest(nowcast, nwp))
        for saliency in (False, True):
            res = run(nowcast, nwp, kwargs, saliency)
            assert not np.isnan(res).any(), name
            out[name + ("__salient" if saliency else "__linear")] = res

    nowcast, nwp, kwargs = hb.make_case("single_37x53")
    try:
        run(nowcast, nwp[:2], kwargs, False)
        raise SystemExit("the short NWP stack did not raise")
    except Exception as exc:
        out["short_nwp_exception"] = np.array(type(exc).__name__)

    db = hb.db_field()
    rate, _ = conversion.to_rainrate(db, dict(hb.DB_META))
    out["db__rainrate"] = rate
    out["db__sha256"] = np.array(hb.digest(db))
    exact = hb.db_inverse_longdouble(db)
    ok = np.isfinite(rate) & (rate > 0)
    assert np.array_equal(rate == 0, np.asarray(exact == 0)) and ok.any()
    ulp = np.spacing(rate[ok]).astype(np.longdouble)
    deviation = float(np.max(np.abs(rate[ok].astype(np.longdouble) - exact[ok]) / ulp))
    with open(BARS, "w") as f:
        json.dump({"numpy": np.__version__, "db_inverse_f64_own_deviation_ulp": deviation,
                   "note": "largest |reference - long double restatement| of 10 ** (R / 10) over the helper's dB field, "
                           "in units in the last place of the reference's result"}, f, indent=1)
        f.write("\n")
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %.1f KiB; dB inverse deviates by %.3f ulp" % (OUT, len(hb.CASES), os.path.getsize(OUT) / 1024.0, deviation))


if __name__ == "__main__":
    main()
