"""The pointwise comparison of tests/test_fft_pointwise_gpu.py for the column lengths 1024 / 2048 / 4096 with n in
{2, 34}, in a process of its own: csrc/fft.hip reads PYSTEPS_HIP_FFT_FOURSTEP once per process, and with the value 2
these lengths take fft_cols_step (log1 / log2 = 5 / 5, 5 / 6, 6 / 6) instead of the one-sweep column pass.  Started by
the test as a fresh child with that variable set; one JSON line per case on stdout:
{"shape", "op", "case", "family", "err" (in u), "at"}.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import fft_pointwise as fp  # noqa: E402
from helpers import fft_pointwise_cases as pc  # noqa: E402


def main():
    if os.environ.get("PYSTEPS_HIP_FFT_FOURSTEP") != "2":
        print("fft_fourstep_child: PYSTEPS_HIP_FFT_FOURSTEP=2 must be set", file=sys.stderr)
        return 2
    for shape in pc.FOURSTEP_SHAPES:
        for op in fp.OPS[:4]:
            want = pc.wants(shape, op)
            for key, x in pc.inputs(shape, op).items():
                err, at = fp.compare(fp.device_op(op, x, shape), want[key])
                print(json.dumps(dict(shape=list(shape), op=op, case=key, family=pc.family(key), err=err, at=list(at))), flush=True)
        banks = pc.weight_banks(shape)
        want = pc.weighted_wants(shape)
        for name, bank in banks.items():
            got = fp.device_weighted(pc.weighted_field(shape), bank, shape)
            for k in range(pc.N_LEVELS):
                err, at = fp.compare(got[k], want[(name, k)])
                print(json.dumps(dict(shape=list(shape), op="weighted", case="%s[%d]" % (name, k), family=name, err=err,
                                      at=list(at))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
