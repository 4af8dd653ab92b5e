"""fs2_density_scale on the host (fs2.h): the exponent e of fs2_pose_density's weighted
amounts q = rint(w 2^e), against its definition restated in Python:

    frexp(wmax) = (m, ex), m in [0.5, 1);  B = min(52, 62 - ceil(log2(max(n, 2))));  e = B - ex.

For every valid case n rint(wmax 2^e) < 2^63 and rint(wmax 2^e) >= 2^(B-1).  A wmax so
small that 2^e itself is no double (e > 1023: a subnormal wmax gives up to e = 1126) is
not treated specially: the function returns B - ex as for any other wmax, because the
amount is formed as ldexp(w, e), which takes any integer exponent and is exact there
(w 2^e < 2^B); the bound above holds in that case too, and the case is pinned below.
The pose_density window rule (fit_density_window) is pure Python and pinned here too."""
import ctypes as C
import math

import numpy as np
import pytest

NS = [1, 2, 3, 64, 4099, 10 ** 6, 2 ** 22, 2 ** 31]
WMAX = [1.0, 0.75, 1e-5, 1.0 / 3.0, 5e-324, 1e300]


def scale(wmax, n):
    from fast_slam_2 import _native as nat
    e = C.c_int32(-12345)
    rc = nat.load().fs2_density_scale(wmax, n, C.byref(e))
    return rc, e.value


def expected(wmax, n):
    v = max(n, 2)
    cl = (v - 1).bit_length()                       # ceil(log2(v)) in integers, v >= 2
    assert cl == math.ceil(math.log2(v))            # (exact for these n)
    B = min(52, 62 - cl)
    _, ex = math.frexp(wmax)
    return B - ex, B


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("wmax", WMAX)
def test_density_scale_matches_definition(wmax, n):
    rc, e = scale(wmax, n)
    want, B = expected(wmax, n)
    assert rc == 0 and e == want
    q = np.rint(np.ldexp(np.float64(wmax), e))      # the amount of the largest weight, as numpy forms it
    qi = int(q)
    assert qi >= 2 ** (B - 1) and qi <= 2 ** B
    assert n * qi < 2 ** 63


def test_density_scale_beyond_ldexp_range_of_two_to_the_e():
    """wmax = 5e-324 (2^-1074): e = B + 1073 > 1023, so 2^e overflows a double, yet
    ldexp(w, e) is exact and the amount is 2^(B-1); nothing is clamped."""
    for n in NS:
        rc, e = scale(5e-324, n)
        _, B = expected(5e-324, n)
        assert rc == 0 and e == B + 1073 and e > 1023
        with np.errstate(over="ignore"):
            assert math.isinf(float(np.ldexp(np.float64(1.0), e)))
        assert np.rint(np.ldexp(np.float64(5e-324), e)) == 2.0 ** (B - 1)


@pytest.mark.parametrize("wmax", [0.0, -0.0, -1.0, -5e-324, float("inf"), float("-inf"), float("nan")])
def test_density_scale_rejects_bad_wmax(wmax):
    from fast_slam_2 import _native as nat
    rc, e = scale(wmax, 64)
    assert rc == nat.FS2_ERR_ARG and e == -12345    # nothing written
    assert "fs2_density_scale" in nat.last_error()


def test_density_scale_rejects_bad_n_and_null():
    from fast_slam_2 import _native as nat
    assert scale(1.0, 0)[0] == nat.FS2_ERR_ARG
    assert scale(1.0, -3)[0] == nat.FS2_ERR_ARG
    assert nat.load().fs2_density_scale(1.0, 4, None) == nat.FS2_ERR_ARG


def _indices(bbox, shape, origin, cell):
    ny, nx = shape
    return (math.floor((bbox[0] - origin[0]) / cell), math.floor((bbox[1] - origin[1]) / cell),
            math.floor((bbox[2] - origin[0]) / cell), math.floor((bbox[3] - origin[1]) / cell))


@pytest.mark.parametrize("shape", [(1, 1), (1, 17), (17, 1), (256, 256), (3, 300)])
@pytest.mark.parametrize("bbox", [(-0.1, -0.2, 0.1, 0.3), (1000.0, -2000.0, 1000.004, -1999.99), (2.0, 3.0, 2.0, 3.0),
                                  (-7.25, 0.0, -7.25, 5.0), (0.0, 0.0, 16.0, 16.0)])
def test_fitted_window_covers_the_box(shape, bbox):
    from fast_slam_2.algorithms.fast_slam_2 import fit_density_window
    ny, nx = shape
    origin, cell = fit_density_window(bbox, shape)
    assert cell > 0 and origin[0] <= bbox[0] and origin[1] <= bbox[1]
    ix0, iy0, ix1, iy1 = _indices(bbox, shape, origin, cell)
    assert 0 <= ix0 <= ix1 <= nx - 1 and 0 <= iy0 <= iy1 <= ny - 1
    for a, n in ((0, nx), (1, ny)):                 # snapped to a multiple of the cell where the axis has > 1 cell
        if n > 1:
            assert origin[a] == math.floor(bbox[a] / cell) * cell
        else:
            assert origin[a] == bbox[a]
    # the starting cell of the rule, grown by 17/16 a whole number of times
    c0 = max((bbox[2] - bbox[0]) / max(nx - 1, 1), (bbox[3] - bbox[1]) / max(ny - 1, 1)) or 1.0
    k = round(math.log(cell / c0) / math.log(1.0625))
    assert k >= 0 and cell == pytest.approx(c0 * 1.0625 ** k, rel=1e-12)


def test_fitted_window_with_one_of_origin_and_cell():
    from fast_slam_2.algorithms.fast_slam_2 import fit_density_window
    bbox = (-0.13, 0.21, 0.4, 0.9)
    origin, cell = fit_density_window(bbox, (8, 8), cell=0.25)
    assert cell == 0.25 and origin == (-0.25, 0.0)
    origin, cell = fit_density_window(bbox, (8, 4), origin=(-1.0, 0.0))
    assert origin == (-1.0, 0.0)
    ix0, iy0, ix1, iy1 = _indices(bbox, (8, 4), origin, cell)
    assert ix1 <= 3 and iy1 <= 7 and cell >= max(1.4 / 4, 0.9 / 8)
    with pytest.raises(ValueError):
        fit_density_window((0.0, 0.0, float("nan"), 1.0), (4, 4))
