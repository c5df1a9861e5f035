"""psh_shutdown releases everything the library owns, and psh_init starts over from nothing.

The cycles run in a child process (tests/helpers/shutdown_cycle.py): this process's own binding is never shut down
under the other tests."""

import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "shutdown_cycle.py")


@pytest.fixture(scope="module")
def run():
    """one run of the child for the tests below"""
    return subprocess.run([sys.executable, HELPER], capture_output=True, text=True, timeout=300)


def test_three_init_shutdown_cycles_give_the_same_bits(run):
    """Window kernel with two order tables and the cached step factors, host path around trim_cache, dense LK and a
    corner request, FFT tables of a plain and a chirp-z length, the mask word, the probability-matching slots: cycle 1
    against each operation's oracle, cycles 2 and 3 bit-identical to cycle 1; one device block and one pinned block
    held across the second shutdown.  The cross-device case (psh_init of another device) needs two devices and is not
    run."""
    print(run.stdout[-3000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert "shutdown cycles: ok" in run.stdout


def test_after_the_last_shutdown_every_entry_point_answers_as_before_psh_init(run):
    """The table of tests/test_entry_points_cpu.py once more, in the child after its third psh_shutdown: in-process, every
    argument zero or NULL, none of the calls gets as far as the device."""
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert "entry points answer as before psh_init" in run.stdout
