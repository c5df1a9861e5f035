"""The entry points of csrc/dimension.hip (pysteps_amd._lib.DIMENSION_SIGNATURES) called with every argument zero or NULL
on a library that is not initialised: as loaded, or - with ``--after-shutdown`` (needs a GPU) - after psh_init, one real
call and psh_shutdown.  Prints one JSON object name -> return value.  tests/helpers/entry_points.py does the same for
the entry points of _lib.SIGNATURES."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from pysteps_amd import _lib  # noqa: E402


def main():
    lib = _lib.load()
    if "--after-shutdown" in sys.argv:
        import numpy as np

        from pysteps_amd.device import DeviceArray
        from pysteps_amd.utils import dimension

        x = DeviceArray.from_host(np.arange(24, dtype=np.float32).reshape(4, 6))
        got = dimension.aggregate_fields(x, 2, axis=0, method="sum").to_host()
        assert np.array_equal(got, np.arange(24, dtype=np.float32).reshape(2, 2, 6).sum(axis=1)), got
        del x
        assert lib.psh_shutdown() == 0
    answers = {name: int(getattr(lib, name)(*[t() for t in argtypes])) for name, (_, argtypes) in _lib.DIMENSION_SIGNATURES.items()}
    print(json.dumps(answers, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
