"""Known-landmark clustering (fs2_cluster.hip) at its path decisions and on maps
the filter built itself.  Every assertion is bit-exact.

Stand-alone entry point (GeometryUtils.dbscan / fs2_cluster_points): every case of
tests/golden/cluster_edges.npz (gen_cluster_edges.py; cluster_edge_props.py states
what each reaches) against the recorded sklearn labels, the recorded reference
centres and tests/ref_dbscan.py computed here -- near-ties within 2 ulps of the
eps circle, the 7x7 window's outer ring and its corner cells (reachable only through
the rounding of the cell index), a cell whose first core point lies beyond
its first 64, components of thousands of cells, clusters around the 64-member
prefetch chunk, K > 64, n = 1, the span limit; device buffers; the C ABI's buffer
protocol and refusals.

Device-resident maps (FastSLAM2.cluster_landmarks / LandmarkUtils.
update_known_landmarks(f.particles)): maps grown by appends and changed by EKF
updates, resamples and copy-on-write; ragged imported maps with empty first and
last particles; the min_samples < 1 skip; hundreds of page rows; maps replaced
after scans.  The expected value is always ref_dbscan over the maps get_state
returns, with Python's own int(total / N * fraction).
"""
import ctypes as C
import os
import time

import numpy as np
import pytest

import cluster_edge_props as props
import ref_dbscan
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = ("window", "window_corners", "late_core", "border_right_first", "border_left_first", "snake", "snake_pair_touch",
         "snake_pair_apart", "sizes", "extremes_far", "extremes_identical", "extremes_n1_ms1", "extremes_n1_ms2",
         "extremes_ms_np1")
REPEATED = ("snake", "snake_pair_touch", "snake_pair_apart", "sizes")     # the union-find is concurrent


@pytest.fixture(scope="module")
def fs():
    import torch  # noqa: F401  (loads the HIP runtime first)
    import fast_slam_2
    from gpu_util import configure
    configure()
    yield fast_slam_2
    configure()


@pytest.fixture(scope="module")
def edges():
    d = np.load(os.path.join(GOLDEN, "cluster_edges.npz"))
    d = {k: d[k] for k in d.files}
    assert tuple(d["names"]) == CASES
    return d


def _case(d, n):
    return d[f"{n}_points"], float(d[f"{n}_eps"]), int(d[f"{n}_min_samples"])


# ---------------------------------------------------------------- stand-alone

@pytest.mark.parametrize("name", CASES)
def test_edge_case(fs, edges, name):
    pts, eps, ms = _case(edges, name)
    before = pts.copy()
    rlab, rcen = ref_dbscan.dbscan(pts, eps, ms)
    for rep in range(4 if name in REPEATED else 1):
        cen, lab = fs.GeometryUtils.dbscan(pts, eps, ms)
        assert lab.dtype == np.int32 and np.array_equal(lab, edges[f"{name}_labels"]), (name, rep)
        assert cen.shape == edges[f"{name}_centres"].shape, (name, rep)
        assert np.array_equal(cen, edges[f"{name}_centres"]), (name, rep)
        assert np.array_equal(lab, rlab) and np.array_equal(cen, rcen), (name, rep)
    assert np.array_equal(pts, before)


@pytest.mark.parametrize("e", range(len(props.EPS_LIST)))
def test_tie_groups(fs, edges, e):
    """150 near-ties per eps, one call each (the origin keeps the coordinates' ulp at
    the scale of ulp(eps^2)): the per-point predicate fl(fl(dx^2) + fl(dy^2)) <= fl(eps^2),
    which here is also sklearn's answer (48 fillers keep the pair out of a tight node)."""
    eps = float(edges["tie_eps"][e])
    counts = props.tie_groups(edges)[e]
    t0 = time.perf_counter()
    got = [fs.GeometryUtils.dbscan(edges["tie_groups_points"][e, g], eps, 2) for g in range(props.TIE_GROUPS)]
    wall = time.perf_counter() - t0
    print(f"tie_groups eps={eps}: groups, predicate != exact / hypot / fma = {counts}; "
          f"{props.TIE_GROUPS} calls in {wall:.3f} s")
    for g, (cen, lab) in enumerate(got):
        rlab, rcen = ref_dbscan.dbscan(edges["tie_groups_points"][e, g], eps, 2)
        assert np.array_equal(lab, edges["tie_groups_labels"][e, g]), (eps, g)
        assert np.array_equal(lab, rlab) and np.array_equal(cen, rcen), (eps, g)
        assert len(cen) == edges["tie_groups_k"][e, g], (eps, g)
        if len(cen):
            assert np.array_equal(cen[0], edges["tie_groups_centres"][e, g]), (eps, g)


def test_tie_two_point(fs, edges):
    """Two-point near-ties on which sklearn's KD-tree (whole node accepted on a
    square-rooted bound; the node's far corner is the other point) answers
    differently from the per-point predicate.  libfs2 follows the predicate: the
    expected value is ref_dbscan's, the recorded sklearn labels are documentation."""
    for e, eps in enumerate(edges["tie_eps"]):
        for g in range(props.TIE_PAIRS):
            pts = edges["tie_two_points"][e, g]
            rlab, rcen = ref_dbscan.dbscan(pts, float(eps), 2)
            cen, lab = fs.GeometryUtils.dbscan(pts, float(eps), 2)
            assert np.array_equal(lab, rlab) and np.array_equal(cen, rcen), (eps, g)
            assert np.array_equal(rlab, edges["tie_two_labels"][e, g]), (eps, g)
            assert not np.array_equal(lab, edges["tie_two_labels_sklearn"][e, g]), (eps, g)


@pytest.mark.parametrize("name", ["sizes", "window"])
def test_cluster_device_buffers(fs, edges, name):
    """fs2_cluster_points(where=FS2_DEVICE) on torch device buffers: bit-equal to FS2_HOST."""
    import torch
    from fast_slam_2 import _native as nat
    pts, eps, ms = _case(edges, name)
    cen, lab = fs.GeometryUtils.dbscan(pts, eps, ms)
    n, K = len(pts), len(cen)
    dp = torch.from_numpy(pts).cuda()
    dc = torch.full((K, 2), float("nan"), dtype=torch.float64, device="cuda")
    dl = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    k = C.c_int64(-9)
    nat.check(nat.load().fs2_cluster_points(0, C.c_void_p(dp.data_ptr()), n, eps, ms, C.c_void_p(dc.data_ptr()), K,
                                            C.byref(k), C.c_void_p(dl.data_ptr()), nat.FS2_DEVICE))
    assert k.value == K
    assert np.array_equal(dc.cpu().numpy(), cen) and np.array_equal(dl.cpu().numpy(), lab)
    assert np.array_equal(dp.cpu().numpy(), pts)           # the input is left as it was


def _raw(nat, pts, eps, ms, cen, cap, lab, n=None):
    k = C.c_int64(-9)
    rc = nat.load().fs2_cluster_points(0, nat.ptr(pts), len(pts) if n is None else n, eps, ms, nat.ptr(cen), cap,
                                       C.byref(k), nat.ptr(lab), nat.FS2_HOST)
    return rc, k.value


def test_cluster_buffer_protocol(fs, edges):
    from fast_slam_2 import _native as nat
    pts, eps, ms = _case(edges, "sizes")
    K, n = len(edges["sizes_centres"]), len(pts)
    # one row short: refused, and *n_clusters tells how many rows are needed
    cen, lab = np.full((K, 2), 7.0), np.full(n, -9, np.int32)
    assert _raw(nat, pts, eps, ms, cen, K - 1, lab) == (nat.FS2_ERR_ARG, K)
    # no centre buffer at all: the count and the labels are still delivered
    lab = np.full(n, -9, np.int32)
    assert _raw(nat, pts, eps, ms, None, 0, lab) == (nat.FS2_ERR_ARG, K)
    assert np.array_equal(lab, edges["sizes_labels"])
    # ... and with no cluster that call succeeds
    p0, e0, m0 = _case(edges, "extremes_ms_np1")
    lab = np.full(len(p0), -9, np.int32)
    assert _raw(nat, p0, e0, m0, None, 0, lab) == (nat.FS2_OK, 0)
    assert np.all(lab == -1)
    # labels are optional
    cen = np.full((K, 2), 7.0)
    assert _raw(nat, pts, eps, ms, cen, K, None) == (nat.FS2_OK, K)
    assert np.array_equal(cen, edges["sizes_centres"])


def test_cluster_refusals(fs, edges):
    from fast_slam_2 import _native as nat
    pts, eps, ms = _case(edges, "extremes_far")
    # the same blobs around (+-2e8, +-2e8): more than 2e9 cells of side eps / (2 sqrt 2)
    # across, which 32-bit cell indices cannot hold.  sklearn itself would cluster them.
    moved = pts + np.sign(pts) * 1.2e8
    assert np.abs(moved).min() > 1.9e8
    with pytest.raises(ValueError, match="span too many eps-cells"):
        fs.GeometryUtils.dbscan(moved, eps, ms)
    # bad arguments: FS2_ERR_ARG before anything is launched, outputs untouched
    small = edges["extremes_ms_np1_points"]
    for kw in (dict(eps=0.0), dict(eps=-0.5), dict(eps=float("nan")), dict(ms=0), dict(ms=-3), dict(n=0)):
        cen, lab = np.full((4, 2), 7.0), np.full(len(small), -9, np.int32)
        rc, k = _raw(nat, small, kw.get("eps", 0.5), kw.get("ms", 2), cen, 4, lab, n=kw.get("n"))
        assert rc == nat.FS2_ERR_ARG and k == -9, kw
        assert np.all(cen == 7.0) and np.all(lab == -9), kw


# ------------------------------------------------------- device-resident maps

def _expect(f, N, fraction=0.7, eps=0.5):
    """(ref_dbscan centres or None, cnt, min_samples) for the maps the handle holds now."""
    *_, cnt, lm = f.get_state()
    pts = ref_dbscan.known_landmark_points(cnt, lm)
    assert len(pts) == int(cnt.sum())
    ms = ref_dbscan.min_samples_of(len(pts), N, fraction)
    return (ref_dbscan.dbscan(pts, eps, ms)[1] if ms >= 1 else None), cnt, ms


def _check_known(fs, f, N):
    """cluster_landmarks and update_known_landmarks(f.particles) against the reference."""
    want, cnt, ms = _expect(f, N)
    assert want is not None, "the case must cluster"
    got = f.cluster_landmarks()
    assert got.shape == want.shape and np.array_equal(got, want)
    fs.LandmarkUtils.known_landmarks = []
    fs.LandmarkUtils.update_known_landmarks(f.particles)
    known = np.array([[k.x, k.y] for k in fs.LandmarkUtils.known_landmarks]).reshape(-1, 2)
    assert np.array_equal(known, want)
    fs.LandmarkUtils.known_landmarks = []
    return want, cnt, ms


def test_filter_built_maps(fs):
    """N = 300 (a 256-thread block plus 44), maps grown from empty over three page rows
    and then the run stream of test_gpu_appended.py, with the C oracle alongside on the
    same injected draws: clustered after the build-up, after the first resampling scan
    and at the end (14 run scans: at N = 300 the stream's first duplicate append, which
    makes the map sizes ragged, comes in run scan 12; resamples in run scans 6 and 8)."""
    import fs2_synthetic as syn
    from oracle import oracle as orc
    N, L, S = 300, 24, 14
    nb = syn.buildup_scans(L)
    cap = L + S + 16
    f = fs.FastSLAM2(N, reduce="auto", record_assoc=True, landmark_capacity=cap, verbose=False)
    o = orc.OracleFilter(N, cap)
    rng = np.random.default_rng(123)
    scans = [("build", s) for s in range(nb)] + [("run", s) for s in range(S)]
    resamples, clustered = 0, []
    for i, (kind, s) in enumerate(scans):
        if kind == "build":
            rot, tr = 0.0, 0.0
            ms = syn.buildup_measurements(L, s)
        else:
            rot, tr = syn.odometry(s)
            ms = syn.scan_measurements(L, s)
        nz = rng.normal(0, 0.001 if rot else 0.0055, N)
        u0 = rng.uniform(0, 1.0 / N)
        _, st = f.step(rot, tr, ms, None, nz, u0)
        _, oassoc, ors, _ = o.iterate(rot, tr, ms, nz, u0)
        assert np.array_equal(f.associations(), oassoc) and bool(st.resampled) == ors, (kind, s)
        resamples += st.resampled
        if i == nb - 1 or (st.resampled and resamples == 1) or i == len(scans) - 1:
            cen, cnt, m = _check_known(fs, f, N)
            assert np.array_equal(cnt, o.cnt), (kind, s)
            clustered.append((kind, s, int(cnt.sum()), m, len(cen)))
    assert resamples >= 1 and len(clustered) == 3
    assert cnt.min() < cnt.max()                                    # ragged at the end
    print("filter-built maps clustered at (kind, scan, points, min_samples, K):", clustered)
    # second reference: the oracle's own maps give the same clusters
    opts = ref_dbscan.known_landmark_points(o.cnt, o.lm)
    ocen = ref_dbscan.dbscan(opts, 0.5, ref_dbscan.min_samples_of(len(opts), N, 0.7))[1]
    assert ocen.shape == cen.shape and np.allclose(cen, ocen, rtol=1e-9, atol=1e-12)
    f.close()


def _ragged_maps(rng, cnt, spread=20.0):
    cap = int(cnt.max())
    base = rng.uniform(-spread, spread, (cap, 2))
    lm = np.zeros((len(cnt), cap, 6))
    for i, c in enumerate(cnt):
        lm[i, :c, :2] = base[:c] + rng.normal(0, 0.02, (c, 2))
        lm[i, :c, 2] = lm[i, :c, 5] = 0.1
    return lm


@pytest.mark.parametrize("shape", ["empty_ends", "last_is_largest"])
def test_ragged_imported_maps(fs, shape):
    """N = 321 with map sizes either side of the 8-slot page rows; off[n-1] + cnt[n-1]
    with an empty and with the largest last particle."""
    N = 321
    rng = np.random.default_rng(17)
    cnt = rng.choice([0, 1, 7, 8, 9, 15, 16, 17, 40], N).astype(np.int32)
    if shape == "empty_ends":
        cnt[0] = cnt[-1] = 0
        cnt[5] = 40
        assert (cnt[1:-1] == 0).sum() >= 10
    else:
        cnt[-1] = 40
        cnt[:-1] = np.minimum(cnt[:-1], 17)
        assert cnt[-1] == cnt.max() and (cnt == 40).sum() == 1
    lm = _ragged_maps(rng, cnt)
    f = fs.FastSLAM2(N, verbose=False, landmark_capacity=40)
    f.set_state(np.zeros(N), np.zeros(N), np.zeros(N), np.full(N, 1.0 / N), cnt, lm)
    cen, got_cnt, ms = _check_known(fs, f, N)
    assert np.array_equal(got_cnt, cnt)
    assert np.array_equal(cen, ref_dbscan.dbscan(ref_dbscan.known_landmark_points(cnt, lm), 0.5, ms)[1])
    f.close()


def test_skip_rule(fs):
    """min_samples = int(total / N * 0.7) < 1 returns without updating
    (landmark_utils.py:131-134); both expectations are Python's own expression."""
    sentinel = [fs.Landmark(1.0, 2.0)]

    def run(N, cnt):
        f = fs.FastSLAM2(N, verbose=False, landmark_capacity=8)
        if cnt is not None:
            cnt = np.array(cnt, np.int32)
            f.set_state(np.zeros(N), np.zeros(N), np.zeros(N), np.full(N, 1.0 / N), cnt,
                        _ragged_maps(np.random.default_rng(3), cnt))
        want, _, ms = _expect(f, N)
        got = f.cluster_landmarks()
        fs.LandmarkUtils.known_landmarks = sentinel
        fs.LandmarkUtils.update_known_landmarks(f.particles)
        known = fs.LandmarkUtils.known_landmarks
        fs.LandmarkUtils.known_landmarks = []
        f.close()
        return want, ms, got, known

    want, ms, got, known = run(64, None)                       # a fresh handle: no landmark
    assert ms == 0 and want is None and got is None and known is sentinel
    want, ms, got, known = run(10, [2, 2, 2, 2, 1, 1, 1, 1, 1, 1])
    assert ms == int(14 / 10 * 0.7) == 0 and got is None and known is sentinel
    want, ms, got, known = run(7, [2, 2, 2, 1, 1, 1, 1])
    assert ms == int(10 / 7 * 0.7) == 1                        # 1.4285714285714286 * 0.7 rounds to 1.0
    assert np.array_equal(got, want)
    assert np.array_equal(np.array([[k.x, k.y] for k in known]), want)


def test_many_page_rows(fs):
    """N = 5 with maps of up to 2100 landmarks (263 page rows, rows >> particles: the
    gather's t / n, t % n indexing), min_samples = 2 through min_fraction."""
    N, L = 5, 2100
    cnt = np.array([2100, 1, 2099, 1050, 2100], np.int32)
    g = np.arange(L)
    base = np.stack([(g % 50) * 1.5, (g // 50) * 1.5], 1)
    rng = np.random.default_rng(5)
    lm = np.zeros((N, L, 6))
    for i, c in enumerate(cnt):
        lm[i, :c, :2] = base[:c] + rng.normal(0, 0.02, (c, 2))
        lm[i, :c, 2] = lm[i, :c, 5] = 0.1
    total = int(cnt.sum())
    fraction = 2.5 / (total / N)
    assert ref_dbscan.min_samples_of(total, N, fraction) == 2
    f = fs.FastSLAM2(N, verbose=False, landmark_capacity=L)
    f.set_state(np.zeros(N), np.zeros(N), np.zeros(N), np.full(N, 1.0 / N), cnt, lm)
    want, got_cnt, ms = _expect(f, N, fraction)
    assert ms == 2 and np.array_equal(got_cnt, cnt) and len(want) == L
    got = f.cluster_landmarks(min_fraction=fraction)
    assert got.shape == want.shape and np.array_equal(got, want)
    f.close()


def test_maps_replaced_after_scans(fs):
    """set_state on a handle that has run scans: the clustering sees the new maps only."""
    import fs2_synthetic as syn
    N, L = 130, 12
    rng = np.random.default_rng(29)
    f = fs.FastSLAM2(N, seed=4, landmark_capacity=L + 12, verbose=False)
    for s in range(syn.buildup_scans(L)):
        f.step(0.0, 0.0, syn.buildup_measurements(L, s))
    for s in range(3):
        f.step(*syn.odometry(s), syn.scan_measurements(L, s))
    old, *_ = _check_known(fs, f, N)
    cnt = rng.choice([3, 9, 10], N).astype(np.int32)
    lm = _ragged_maps(rng, cnt, spread=40.0)
    lm[:, :, :2] += 100.0                                      # nowhere near the old maps
    f.set_state(np.zeros(N), np.zeros(N), np.zeros(N), np.full(N, 1.0 / N), cnt, lm)
    new, got_cnt, ms = _check_known(fs, f, N)
    assert np.array_equal(got_cnt, cnt) and new.min() > 50.0 > old.max()
    assert np.array_equal(new, ref_dbscan.dbscan(ref_dbscan.known_landmark_points(cnt, lm), 0.5, ms)[1])
    f.close()


def test_sharded_handle_is_refused(fs):
    """Clustering needs every particle on one rank: FS2_ERR_STATE on a two-rank handle."""
    from fast_slam_2 import _native as nat
    key = os.urandom(128)
    shards = [fs.FastSLAM2(512, seed=5, rank=g, world_size=2, comm_id=key, comm_mode="local", verbose=False)
              for g in range(2)]
    for h in shards:
        with pytest.raises(nat.FS2Error) as err:
            h.cluster_landmarks()
        assert err.value.code == nat.FS2_ERR_STATE
    for h in shards:
        h.close()
