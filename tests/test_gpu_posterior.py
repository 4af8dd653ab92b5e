"""The posterior readout on the device (fs2_pose_moments / fs2_pose_density, DESIGN.md
§14) against host references.

Moments.  The references are math.fsum over per-term float64 products (numpy's sin and
cos), i.e. the exact sum of the rounded terms.  Tolerances are derived: a sum of N terms
t_i in any order, each term built by at most 3 roundings, errs by at most
(N + 8) 2^-52 sum|t_i|; normalised quantities divide that by W; each sin / cos term gets a
further 4 2^-52 w_i (the 4 ulp the device math library is held to); mean_yaw's bound is
the two sums' bound over R W plus 4 2^-52.  The covariance is the second pass about the
first pass's mean (fs2.h), so its reference is formed about the mean the call returned,
which is itself checked against its own bound.  bbox and the count are exact.

Density.  Raw uint64 counts against np.add.at with the index and amount formulas of
fs2.h; every comparison is np.array_equal."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
TWO_PI = 2.0 * math.pi
MOMENT_NS = [1, 63, 64, 65, 255, 256, 257, 4099, 70001]
DENSITY_NS = [1, 64, 257, 4099, 70001]


def make(N, seed=3, guard=False, **kw):
    import fast_slam_2
    from gpu_util import configure
    configure()
    kw.setdefault("reduce", "auto")
    old = os.environ.get("FS2_GUARD")
    if guard:
        os.environ["FS2_GUARD"] = "1"
    try:
        return fast_slam_2.FastSLAM2(N, rng="device", seed=seed, record_assoc=True, verbose=False, **kw)
    finally:
        if guard:
            if old is None:
                os.environ.pop("FS2_GUARD", None)
            else:
                os.environ["FS2_GUARD"] = old


def weights(N, seed):
    """Positive weights over six decades, not normalised, a few exactly 0."""
    rng = np.random.default_rng([seed, 77])
    w = 10.0 ** rng.uniform(-6.0, 0.0, N)
    if N >= 63:
        w[rng.choice(N, 3, replace=False)] = 0.0
    return w


def cloud(N, seed=0, centre=(0.0, 0.0), scale=1.0, yaw=None):
    import fs2_synthetic as syn
    x, y, t = syn.particle_poses(N, seed)
    x = centre[0] + scale * x
    y = centre[1] + scale * y
    return x, y, (t if yaw is None else yaw)


def wrap(d):
    return d - TWO_PI * np.floor((d + math.pi) / TWO_PI)


def fsum(a):
    return math.fsum(a.tolist())


def angle_diff(a, b):
    return abs(math.remainder(a - b, TWO_PI))


def check_moments(pm, x, y, yaw, w, label=""):
    """pm against the fsum references of (x, y, yaw) with weights w (ones: unweighted)."""
    N = len(x)
    k = (N + 8) * U
    W = fsum(w)
    assert pm.weight_sum == pytest.approx(W, rel=0, abs=k * W), label
    assert pm.weight_sq_sum == pytest.approx(fsum(w * w), rel=0, abs=k * fsum(w * w)), label
    assert np.array_equal(pm.bbox, [x.min(), y.min(), x.max(), y.max()]), label
    for a, v in ((0, x), (1, y)):
        t = w * v
        bound = k * fsum(np.abs(t)) / W
        err = abs(pm.mean[a] - fsum(t) / W)
        print(f"{label} mean[{a}] err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (label, a, err, bound)
    ts, tc = w * np.sin(yaw), w * np.cos(yaw)
    S, Cc = fsum(ts), fsum(tc)
    R = math.hypot(S, Cc) / W
    assert R >= 0.5, label                                   # the division by R W stays tame
    bs, bc = k * fsum(np.abs(ts)) + 4 * U * W, k * fsum(np.abs(tc)) + 4 * U * W
    byaw = (bs + bc) / (R * W) + 4 * U
    err = angle_diff(pm.mean[2], math.atan2(S, Cc))
    print(f"{label} mean_yaw err {err:.3e} bound {byaw:.3e}")
    assert err <= byaw, (label, err, byaw)
    assert -math.pi <= pm.mean[2] <= math.pi
    # R = hypot(S, C) / W: the sums' bounds over W, W's own relative bound, hypot and the division
    assert abs(pm.resultant - R) <= (bs + bc) / W + k * R + 4 * U, label
    # the second pass, about the returned mean
    d = (x - pm.mean[0], y - pm.mean[1], wrap(yaw - pm.mean[2]))
    assert np.array_equal(pm.cov, pm.cov.T), label
    for a in range(3):
        for b in range(a, 3):
            t = w * d[a] * d[b]
            bound = k * fsum(np.abs(t)) / W
            err = abs(pm.cov[a, b] - fsum(t) / W)
            print(f"{label} cov[{a}{b}] err {err:.3e} bound {bound:.3e} value {pm.cov[a, b]:.6e}")
            assert err <= bound, (label, a, b, err, bound)


def both_ways(f, x, y, yaw, w, label):
    f.set_state(x, y, yaw, w)
    check_moments(f.pose_moments(True), x, y, yaw, w, label + " weighted")
    check_moments(f.pose_moments(False), x, y, yaw, np.ones(len(x)), label + " unweighted")


def bits(pm):
    return np.concatenate([np.ravel(np.asarray(v, dtype=np.float64)) for v in pm]).view(np.uint64)


STAT_FIELDS = ("resampled", "n_eff", "total_weight", "best_index", "hits", "appends", "max_count")


def check_guards(f):
    from fast_slam_2 import _native as nat
    name = C.create_string_buffer(128)
    bad = nat.load().fs2_debug_check_guards(f._h, name, 128)
    assert bad == 0, f"{bad} guard bytes overwritten after buffer {name.value.decode()}"


# ------------------------------------------------------------------ moments ---

@pytest.mark.parametrize("N", MOMENT_NS)
def test_moments_match_fsum_reference(N):
    f = make(N)
    x, y, yaw = cloud(N, seed=N)
    w = weights(N, N)
    both_ways(f, x, y, yaw, w, f"N={N}")
    pm = f.pose_moments()
    assert pm.mean.shape == (3,) and pm.cov.shape == (3, 3) and pm.bbox.shape == (4,)
    sums = np.empty(4)
    from fast_slam_2 import _native as nat
    nat.check(nat.load().fs2_pose_moments(f._h, 1, None, None, nat.ptr(sums), None), f._h)   # null outputs
    assert sums[3] == N and sums[0] == pm.weight_sum and sums[2] == pm.resultant
    f.close()


@pytest.mark.parametrize("N", [257, 4099])
def test_tight_cloud_far_from_the_origin(N):
    """sigma = 1e-3 about (1000, -2000): raw second moments would lose the covariance
    (x^2 ~ 1e6 against a variance of 1e-6); the second pass keeps it within its bound."""
    f = make(N)
    x, y, yaw = cloud(N, seed=5, centre=(1000.0, -2000.0), scale=1e-3 / 0.05)
    both_ways(f, x, y, yaw, weights(N, 9), f"tight N={N}")
    pm = f.pose_moments(False)
    assert 0.5e-6 < pm.cov[0, 0] < 2e-6 and 0.5e-6 < pm.cov[1, 1] < 2e-6
    f.close()


@pytest.mark.parametrize("N", [65, 4099])
def test_yaws_around_pi(N):
    f = make(N)
    x, y, _ = cloud(N, seed=6)
    rng = np.random.default_rng([N, 5])
    yaw = rng.normal(math.pi, 0.3, N)
    yaw = np.where(yaw > math.pi, yaw - TWO_PI, yaw)          # into (-pi, pi]
    assert yaw.min() > -math.pi and yaw.max() <= math.pi and (yaw > 0).any() and (yaw < 0).any()
    both_ways(f, x, y, yaw, weights(N, 4), f"pi N={N}")
    pm = f.pose_moments(False)
    assert angle_diff(pm.mean[2], math.pi) < 0.15             # not 0
    assert 0.05 < pm.cov[2, 2] < 0.14                         # ~ 0.09, not ~ pi^2
    assert abs(pm.resultant - math.exp(-0.045)) < 0.05
    f.close()


def test_one_particle_has_zero_covariance():
    f = make(1)
    x, y, yaw, w = np.array([1.7]), np.array([-0.3]), np.array([2.9]), np.array([0.3])
    f.set_state(x, y, yaw, w)
    for weighted in (True, False):
        pm = f.pose_moments(weighted)
        assert np.array_equal(pm.cov, np.zeros((3, 3)))
        assert np.array_equal(pm.mean, [1.7, -0.3, 2.9])
        assert pm.resultant == 1.0
    check_moments(f.pose_moments(), x, y, yaw, w, "N=1")
    f.close()


def test_two_calls_and_another_handle_in_between_give_identical_bits():
    N = 70001
    f = make(N)
    x, y, yaw = cloud(N, seed=2)
    f.set_state(x, y, yaw, weights(N, 2))
    a = f.pose_moments()
    b = f.pose_moments()
    g = make(4099, seed=8)
    g.set_state(*cloud(4099, seed=3), weights(4099, 3))
    g.pose_moments()
    g.pose_density((64, 64))
    g.close()
    c = f.pose_moments()
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    ga = f.pose_density((64, 64), raw=True)
    gb = f.pose_density((64, 64), raw=True)
    assert np.array_equal(ga[0], gb[0]) and ga[1:] == gb[1:]
    f.close()


@pytest.mark.parametrize("kind", ["zeros", "negative", "nan"])
def test_invalid_weights_are_a_state_error_and_write_nothing(kind):
    from fast_slam_2 import _native as nat
    N = 4099
    f = make(N)
    x, y, yaw = cloud(N, seed=1)
    w = weights(N, 1)
    if kind == "zeros":
        w[:] = 0.0
    elif kind == "negative":
        w[2500] = -1e-9
    else:
        w[4098] = float("nan")
    f.set_state(x, y, yaw, w)
    lib = nat.load()
    mean, cov, sums, bbox = np.full(3, -7.5), np.full(9, -7.5), np.full(4, -7.5), np.full(4, -7.5)
    rc = lib.fs2_pose_moments(f._h, 1, nat.ptr(mean), nat.ptr(cov), nat.ptr(sums), nat.ptr(bbox))
    assert rc == nat.FS2_ERR_STATE and nat.last_error(f._h)
    for a in (mean, cov, sums, bbox):
        assert np.all(a == -7.5)
    grid = np.full((8, 8), 12345, dtype=np.uint64)
    e, out = C.c_int32(-99), C.c_uint64(77)
    rc = lib.fs2_pose_density(f._h, 1, -1.0, -1.0, 0.25, 8, 8, nat.ptr(grid), C.byref(e), C.byref(out))
    assert rc == nat.FS2_ERR_STATE and nat.last_error(f._h)
    assert np.all(grid == 12345) and e.value == -99 and out.value == 77
    with pytest.raises(nat.FS2Error):
        f.pose_moments()
    # the unweighted forms do not read the weights
    check_moments(f.pose_moments(False), x, y, yaw, np.ones(N), kind)
    assert f.pose_density((8, 8), weighted=False, raw=True)[0].sum() == N
    f.close()


# ------------------------------------------------------------------ density ---

def ref_density(x, y, w, x0, y0, cell, nx, ny, weighted):
    """(grid, outside, e) by the formulas of fs2.h."""
    from fast_slam_2 import _native as nat
    N = len(x)
    e = 0
    q = np.ones(N, dtype=np.uint64)
    if weighted:
        ce = C.c_int32()
        nat.check(nat.load().fs2_density_scale(float(w.max()), N, C.byref(ce)))
        e = ce.value
        q = np.rint(np.ldexp(w, e)).astype(np.uint64)
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = np.floor((x - x0) / cell), np.floor((y - y0) / cell)
        inside = (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny)
    grid = np.zeros((ny, nx), dtype=np.uint64)
    np.add.at(grid, (fy[inside].astype(np.int64), fx[inside].astype(np.int64)), q[inside])
    return grid, int(q[~inside].sum(dtype=np.uint64)), e, int(q.sum(dtype=np.uint64))


def check_density(f, x, y, w, x0, y0, cell, nx, ny, label=""):
    for weighted in (True, False):
        grid, outside, origin, c, e = f.pose_density((ny, nx), (x0, y0), cell, weighted=weighted, raw=True)
        rg, rout, re_, total = ref_density(x, y, w, x0, y0, cell, nx, ny, weighted)
        assert grid.dtype == np.uint64 and grid.shape == (ny, nx)
        assert e == re_ and origin == (x0, y0) and c == cell, label
        assert np.array_equal(grid, rg), (label, weighted)
        assert outside == rout, (label, weighted)
        assert int(grid.sum(dtype=np.uint64)) + outside == total, (label, weighted)
        fg, fo, _, _ = f.pose_density((ny, nx), (x0, y0), cell, weighted=weighted)
        assert fg.dtype == np.float64 and np.array_equal(fg, np.ldexp(rg.astype(np.float64), -re_))
        assert fo == math.ldexp(float(rout), -re_)
    return rg


def spread(N, seed, lo, hi):
    rng = np.random.default_rng([seed, 13])
    return rng.uniform(lo, hi, N), rng.uniform(lo, hi, N)


@pytest.mark.parametrize("N", DENSITY_NS)
def test_density_clouds_and_windows(N):
    f = make(N)
    w = weights(N, N + 1)
    _, _, yaw = cloud(N)
    # a tight cloud in one cell
    x, y, _ = cloud(N, seed=N, centre=(0.503, 0.507), scale=1e-4)
    f.set_state(x, y, yaw, w)
    g = check_density(f, x, y, w, 0.0, 0.0, 0.01, 256, 256, "tight")
    assert np.count_nonzero(g) == 1
    # the config-3-like cloud (sigma 0.05 m) on 1 cm cells: workgroup boxes fit the LDS window
    x, y, _ = cloud(N, seed=N + 1)
    f.set_state(x, y, yaw, w)
    check_density(f, x, y, w, -1.28, -1.28, 0.01, 256, 256, "config 3")
    # uniform over a 300 x 300 grid: a workgroup's box exceeds the window, lanes add to memory
    x, y = spread(N, N, 0.0, 300.0)
    f.set_state(x, y, yaw, w)
    check_density(f, x, y, w, 0.0, 0.0, 1.0, 300, 300, "spread")
    # a mix: the first half tight, the second half spread
    xt, yt, _ = cloud(N, seed=N + 2, centre=(150.2, 150.7), scale=0.2)
    h = N // 2
    xm, ym = np.concatenate((xt[:h], x[h:])), np.concatenate((yt[:h], y[h:]))
    f.set_state(xm, ym, yaw, w)
    check_density(f, xm, ym, w, 0.0, 0.0, 1.0, 300, 300, "mix")
    # grids of one row, one column, one cell (most of the cloud outside)
    for ny, nx in ((1, 1), (1, 17), (17, 1)):
        check_density(f, xm, ym, w, 140.0, 145.0, 1.25, nx, ny, f"{ny}x{nx}")
    f.close()


def test_density_boundaries_and_non_finite_poses():
    N = 257
    f = make(N)
    w = weights(N, 21)
    w[:8] = [0.5, 0.25, 1.0, 0.125, 0.75, 0.3, 0.2, 0.9]
    x, y = spread(N, 21, 0.0, 4.0)
    yaw = np.zeros(N)
    x0, y0, cell, nx, ny = -0.75, -0.5, 0.25, 19, 18      # the spread lies inside: x in [0, 4), y in [0, 4)
    x[0] = x0                                     # exactly at x0: column 0
    x[1] = x0 + nx * cell                         # exactly at the far edge (4.0): outside
    y[2] = y0 + ny * cell
    y[3] = y0                                     # row 0
    x[4] = float("nan")
    x[5] = x0 - 1e-9                              # the negative side
    y[6] = float("inf")
    y[7] = float("-inf")
    f.set_state(x, y, yaw, w)
    check_density(f, x, y, w, x0, y0, cell, nx, ny, "edges")
    grid, outside = f.pose_density((ny, nx), (x0, y0), cell, weighted=False, raw=True)[:2]
    assert outside == 6                           # particles 1, 2, 4, 5, 6, 7
    assert grid[:, 0].sum() == 1 and grid[0, :].sum() == 1 and grid.sum() == N - 6
    f.close()


def test_density_bad_arguments():
    from fast_slam_2 import _native as nat
    f = make(64)
    lib = nat.load()
    grid = np.zeros((4, 4), dtype=np.uint64)

    def call(cell=1.0, nx=4, ny=4, g=grid, h=None):
        return lib.fs2_pose_density(f._h if h is None else h, 0, 0.0, 0.0, cell, nx, ny, nat.ptr(g), None, None)

    assert call() == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(cell=bad) == nat.FS2_ERR_ARG
    assert call(nx=0) == nat.FS2_ERR_ARG and call(ny=0) == nat.FS2_ERR_ARG and call(nx=-3) == nat.FS2_ERR_ARG
    assert call(nx=4097, ny=4096) == nat.FS2_ERR_ARG          # nx ny > 2^24 (checked before the grid is touched)
    assert call(g=None) == nat.FS2_ERR_ARG
    assert lib.fs2_pose_density(None, 0, 0.0, 0.0, 1.0, 4, 4, nat.ptr(grid), None, None) == nat.FS2_ERR_ARG
    assert lib.fs2_pose_moments(None, 0, None, None, None, None) == nat.FS2_ERR_ARG
    with pytest.raises(ValueError):
        f.pose_density((4, 4), (0.0, 0.0), -2.0)
    f.close()
    for fn in (f.pose_moments, lambda: f.pose_density((4, 4))):
        with pytest.raises(nat.FS2Error):
            fn()


@pytest.mark.parametrize("shape", [(256, 256), (1, 1), (17, 1), (3, 40)])
def test_fitted_window_holds_every_particle(shape):
    from fast_slam_2.algorithms.fast_slam_2 import fit_density_window
    N = 4099
    f = make(N)
    x, y, yaw = cloud(N, seed=4, centre=(3.0, -11.0))
    w = weights(N, 4)
    f.set_state(x, y, yaw, w)
    grid, outside, origin, cell, e = f.pose_density(shape, raw=True)
    assert outside == 0
    bbox = f.pose_moments(False).bbox
    assert (origin, cell) == fit_density_window(bbox, shape)
    ny, nx = shape
    rg, rout, re_, _ = ref_density(x, y, w, origin[0], origin[1], cell, nx, ny, True)
    assert np.array_equal(grid, rg) and rout == 0 and e == re_
    # one of the two given
    _, o2, org2, c2 = f.pose_density(shape, cell=cell * 2)
    assert c2 == cell * 2 and (org2, c2) == fit_density_window(bbox, shape, cell=cell * 2)
    _, o3, org3, c3 = f.pose_density(shape, origin=origin)
    assert org3 == origin and (org3, c3) == fit_density_window(bbox, shape, origin=origin) and o3 == 0.0
    f.close()


# ----------------------------------------------------------- non-interference ---

def run_scans(f, N, L, scans, readout):
    import fs2_synthetic as syn
    out, resampled_at = [], []
    for s in range(scans):
        pose, st = f.step(*syn.odometry(s), np.ascontiguousarray(syn.scan_measurements(L, s, 0)))
        out.append((pose.copy(), tuple(getattr(st, k) for k in STAT_FIELDS), f.associations()))
        if st.resampled:
            resampled_at.append(s)
        if readout:
            readout(s, st)
    return out, resampled_at


def populate(f, N, L):
    import fs2_synthetic as syn
    x, y, yaw = syn.particle_poses(N, 0)
    lm = syn.particle_maps(N, L, 0)
    f.set_state(x, y, yaw, np.full(N, 1.0 / N), np.full(N, L, dtype=np.int32), lm)


def test_readouts_do_not_change_the_filter():
    N, L, scans = 4099, 12, 6
    a, b = make(N, seed=11, landmark_capacity=L + 4 * scans + 8), make(N, seed=11, landmark_capacity=L + 4 * scans + 8)
    populate(a, N, L)
    populate(b, N, L)
    checked = []

    def readout(s, st):
        a.pose_moments(True)
        pm = a.pose_moments(False)
        a.pose_density((256, 256))
        a.pose_density((300, 300), (-150.0, -150.0), 1.0, weighted=False)
        if st.resampled:
            x, y, yaw = a.get_state(lm_cap=0)[:3]
            check_moments(pm, x, y, yaw, np.ones(N), f"after the resample of scan {s}")
            checked.append(s)

    ra, res_a = run_scans(a, N, L, scans, readout)
    rb, res_b = run_scans(b, N, L, scans, None)
    assert res_a == res_b and len(res_a) >= 1 and checked == res_a
    for u, v in zip(ra, rb):
        assert np.array_equal(u[0], v[0]) and u[1] == v[1] and np.array_equal(u[2], v[2])
    for u, v in zip(a.get_state(), b.get_state()):
        assert u.shape == v.shape and np.array_equal(u, v)
    a.close()
    b.close()


def test_readouts_write_past_no_buffer():
    import fs2_synthetic as syn
    N, L = 20011, 12
    f = make(N, seed=3, guard=True, landmark_capacity=L + 32)
    populate(f, N, L)
    for s in range(4):
        f.step(*syn.odometry(s), np.ascontiguousarray(syn.scan_measurements(L, s, 0)))
        f.pose_moments()
        f.pose_density((256, 256))
        f.pose_density((300, 7), (-1.0, -1.0), 0.01, weighted=False)     # (another grid size: the buffer is remade)
        check_guards(f)
    f.close()


def test_pending_scan_refuses_the_readouts():
    import fs2_synthetic as syn
    from fast_slam_2 import _native as nat
    N, L = 4099, 12
    f = make(N, landmark_capacity=L + 16)
    populate(f, N, L)
    f.step_submit(*syn.odometry(0), np.ascontiguousarray(syn.scan_measurements(L, 0, 0)))
    for fn in (f.pose_moments, lambda: f.pose_density((16, 16)), lambda: f.pose_density((16, 16), (0.0, 0.0), 1.0)):
        with pytest.raises(nat.FS2Error) as ei:
            fn()
        assert ei.value.code == nat.FS2_ERR_STATE
    f.step_wait()
    pm = f.pose_moments()
    assert pm.weight_sum > 0 and f.pose_density((16, 16), raw=True)[1] == 0
    f.close()
