"""float.__repr__ as libfs2 writes it (csrc/fs2_repr.hpp), on the CPU: the routine the
device runs, called through fs2_repr_doubles(on_host=1), against CPython's own
float.__repr__ / json.dumps for every input (no device needed)."""
import json

import numpy as np

import repr_cases as rc


def _check(v):
    out, ln = rc.native_repr(v, on_host=True)
    rc.assert_matches_cpython(np.asarray(v, dtype=np.float64), out, ln)


def test_curated_values():
    v = rc.curated()
    _check(v)
    # the layouts the issue names, spelled out (the yardstick itself agrees)
    for x, s in [(1e-5, "1e-05"), (1e16, "1e+16"), (5e-324, "5e-324"), (1.0, "1.0"), (-0.0, "-0.0"),
                 (9999999999999998.0, "9999999999999998.0"), (1e-4, "0.0001"),
                 (-2.2250738585072014e-308, "-2.2250738585072014e-308")]:
        assert json.dumps(x) == s
        out, ln = rc.native_repr([x], on_host=True)
        assert bytes(out[0, :ln[0]]).decode() == s


def test_non_finite_spellings():
    v = np.concatenate([rc.nans(), [np.inf, -np.inf]])
    out, ln = rc.native_repr(v, on_host=True)
    got = [bytes(out[i, :ln[i]]).decode() for i in range(len(v))]
    assert got == ["NaN"] * 6 + ["Infinity", "-Infinity"]


def test_every_power_of_two_and_ten_with_neighbours():
    _check(rc.boundaries())


def test_random_bit_patterns():
    _check(rc.random_patterns(2_000_000, seed=20240611))


def test_pose_like_values():
    _check(rc.pose_like(2_000_000, seed=20240612))


def test_empty_and_bad_arguments():
    from fast_slam_2 import _native as nat
    lib = nat.load()
    assert lib.fs2_repr_doubles(0, None, 0, None, None, 1) == nat.FS2_OK
    assert lib.fs2_repr_doubles(0, None, 3, None, None, 1) == nat.FS2_ERR_ARG
    assert lib.fs2_repr_doubles(0, None, -1, None, None, 1) == nat.FS2_ERR_ARG
