"""The map readout's entry points (fs2.h "map readout": fs2_map_summary, fs2_map_density,
fs2_debug_map_times) as far as they go without a device: the library exports them with
the signatures the binding declares, a null handle is FS2_ERR_ARG before anything touches
HIP, the timing hook answers, and the header declares all three."""
import ctypes as C
import os
import re

import numpy as np

NAMES = ("fs2_map_summary", "fs2_map_density", "fs2_debug_map_times")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fs2.h")


def test_symbols_are_bound():
    from fast_slam_2 import _native as nat
    lib = nat.load()
    sigs = {name: (res, args) for name, res, args in nat.SIGNATURES}
    for name in NAMES:
        assert name in sigs
        fn = getattr(lib, name)
        assert fn.restype is sigs[name][0] and list(fn.argtypes) == sigs[name][1]
    assert len(sigs["fs2_map_summary"][1]) == 3 and len(sigs["fs2_map_density"][1]) == 10


def test_null_handle_is_an_argument_error_without_a_device():
    from fast_slam_2 import _native as nat
    lib = nat.load()
    grid = np.full((4, 4), 12345, dtype=np.uint64)
    bbox, counts = np.full(4, -7.5), np.full(4, -7, dtype=np.int64)
    e, out = C.c_int32(-99), C.c_uint64(77)
    assert lib.fs2_map_summary(None, nat.ptr(bbox), nat.ptr(counts)) == nat.FS2_ERR_ARG
    assert "null handle" in nat.last_error()
    for weighted in (0, 1):
        rc = lib.fs2_map_density(None, weighted, 0.0, 0.0, 1.0, 4, 4, nat.ptr(grid), C.byref(e), C.byref(out))
        assert rc == nat.FS2_ERR_ARG
    assert np.all(grid == 12345) and np.all(bbox == -7.5) and np.all(counts == -7)
    assert e.value == -99 and out.value == 77


def test_timing_hook_answers_without_a_device():
    from fast_slam_2 import _native as nat
    lib = nat.load()
    ms = np.full(3, -1.0)
    assert lib.fs2_debug_map_times(-1, nat.ptr(ms)) == 0      # -1: leaves the switch alone
    assert np.all(ms >= 0.0)                                  # the last timed call's, or 0
    assert lib.fs2_debug_map_times(-1, None) == 0


def test_header_declares_the_map_readout():
    text = open(HEADER).read()
    assert "map readout" in text
    assert text.index("posterior readout") < text.index("map readout")
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", text, re.M), name
    assert re.search(r"int fs2_map_summary\(fs2_handle \*h, double bbox\[4\], int64_t counts\[4\]\);", text)
    assert "#define FS2_ABI_VERSION 2" in text
