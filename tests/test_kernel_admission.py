"""grlx_create refuses what it refused before its admission checks were moved to the kernel table: same code, same message, byte for
byte, over the grid of tests/admission_grid.py (no device needed: what is admitted shows up as GRLX_ERR_NO_DEVICE; with a device the
admitted contexts are created, small, and destroyed)."""
import ctypes as C
import os

from tests import admission_grid

LISTING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "kernel_admission.txt")


def test_refusals_equal_the_recorded_listing(grlx):
    lib = C.CDLL(grlx.capi.lib_path())
    with open(LISTING) as f:
        want = f.read().split("\n")
    if want[-1] == "":
        want.pop()
    got = admission_grid.listing(lib)
    assert len(want) > 108 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
