"""Compact snapshots on the device (fs2_snapshot_save / fs2_snapshot_load): a handle
restored from a snapshot continues bit for bit like the one that was never stopped,
pages that resampled siblings share are stored once and stay shared, a snapshot
assembled by hand restores to the maps it encodes, the kernels hold at their shape
edges, and every refused call leaves the handle as it was.  The feature moves bits:
every comparison is np.array_equal."""
import ctypes as C
import os

import numpy as np
import pytest

import snapshot_cases as sc

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("resampled", "n_eff", "total_weight", "best_index", "hits", "appends", "max_count")


def make(N, cap, seed=3, **kw):
    import fast_slam_2
    from gpu_util import configure
    configure()
    kw.setdefault("reduce", "auto")
    return fast_slam_2.FastSLAM2(N, rng="device", seed=seed, record_assoc=True, landmark_capacity=cap,
                                 verbose=False, **kw)


def scan(f, rot, tr, ms):
    """One scan's results, as compared between two handles."""
    pose, st = f.step(rot, tr, np.ascontiguousarray(ms, dtype=np.float64))
    return (pose.copy(), tuple(getattr(st, k) for k in STAT_FIELDS), f.associations(), st)


def same_scan(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


def same_state(a, b):
    return len(a) == len(b) and all(u.shape == v.shape and np.array_equal(u, v) for u, v in zip(a, b))


def info_of(buf):
    import fast_slam_2
    return fast_slam_2.FastSLAM2.snapshot_info(buf)


# ---------------------------------------------------------------- resume ---

# Workload(20000, 40, seed 0) on the C oracle (normal draws of the same sigmas): the
# resample rule fires at scans 4 and 6 (N_eff 6465 and 534 against N / 2 = 10000) and
# at scans 7 .. 10 (865, 9851, 7007, 9566), so K = 7 scans before the save and K2 = 3
# after it put resamples on both sides; the test asserts that they did.
N_RUN, L_RUN, K, K2 = 20_000, 40, 7, 3


@pytest.fixture(scope="module")
def run():
    import fs2_synthetic as syn
    wl = syn.Workload(N_RUN, L_RUN, 0)
    cap = L_RUN + 2 * (K + K2) + 8
    x, y, yaw = wl.poses()
    lm = wl.maps()
    a, b = make(N_RUN, cap), make(N_RUN, cap)
    for f in (a, b):
        f.set_state(x, y, yaw, np.full(N_RUN, 1.0 / N_RUN), np.full(N_RUN, L_RUN, np.int32), lm)
    out = {"before": [], "after_a": [], "after_c": []}
    for s in range(K):
        ra, rb = (scan(f, *wl.odometry(s), wl.measurements(s)) for f in (a, b))
        assert same_scan(ra, rb), s
        out["before"].append(ra)
    out["snap"] = b.snapshot()
    out["snap_again"] = b.snapshot()
    out["state_b"] = b.get_state()
    b.close()
    c = make(N_RUN, cap)
    c.restore(out["snap"])
    out["state_c"] = c.get_state()
    out["snap_c"] = c.snapshot()
    for s in range(K, K + K2):
        out["after_a"].append(scan(a, *wl.odometry(s), wl.measurements(s)))
        out["after_c"].append(scan(c, *wl.odometry(s), wl.measurements(s)))
    out["final_a"], out["final_c"] = a.get_state(), c.get_state()
    a.close()
    c.close()
    return out


def test_resume_equals_uninterrupted(run):
    assert any(r[1][0] for r in run["before"]), "no resample before the save"
    assert any(r[1][0] for r in run["after_a"]), "no resample after the save"
    for s, (ra, rc) in enumerate(zip(run["after_a"], run["after_c"])):
        assert np.array_equal(ra[0], rc[0]), ("pose", K + s)
        assert ra[1] == rc[1], (K + s, dict(zip(STAT_FIELDS, zip(ra[1], rc[1]))))
        assert np.array_equal(ra[2], rc[2]), ("associations", K + s)
    assert same_state(run["final_a"], run["final_c"])


def test_sharing_is_kept(run):
    ib, ic = info_of(run["snap"]), info_of(run["snap_c"])
    cnt = run["state_b"][4]
    assert ib["pages"] < int(((cnt + 7) // 8).sum()), ib          # shared pages are stored once
    assert ib["num_particles"] == N_RUN and ib["scan"] == K and ib["max_count"] == int(cnt.max())
    for k in ("pages", "records", "rows", "max_count", "scan"):
        assert ib[k] == ic[k], k
    assert same_state(run["state_b"], run["state_c"])
    assert np.array_equal(run["snap"], run["snap_again"])         # a save is deterministic


def test_hand_built_snapshot_restores_to_its_maps():
    buf, want = sc.hand_built()
    f = make(3, 16)
    f.restore(buf)
    got = f.get_state()
    assert same_state(got, want)
    assert info_of(f.snapshot())["pages"] == 3
    f.close()


# ----------------------------------------------------------- shape edges ---

def ragged_state(N, counts, seed):
    """Maps of counts[i % len(counts)] landmarks: the first of a common jittered grid."""
    import fs2_synthetic as syn
    Lm = max(max(counts), 1)
    base = syn.common_landmarks(Lm, seed)
    rng = np.random.default_rng(seed)
    cnt = np.array([counts[i % len(counts)] for i in range(N)], dtype=np.int32)
    lm = np.zeros((N, Lm, 6))
    lm[:, :, 0:2] = base[None] + rng.normal(0, syn.MAP_JITTER, (N, Lm, 2))
    lm[:, :, 2] = lm[:, :, 5] = syn.INIT_COV
    lm[np.arange(Lm)[None, :] >= cnt[:, None]] = 0.0
    x, y, yaw = syn.particle_poses(N, seed)
    return x, y, yaw, np.full(N, 1.0 / N), cnt, lm


def roundtrip(N, state, cap, scans, meas, expect=None, **kw):
    """Seed a handle, run `scans` scans, snapshot; the snapshot passes the host check,
    restores into a fresh handle to the same state, and one further scan agrees."""
    import fs2_synthetic as syn
    f = make(N, cap, **kw)
    f.set_state(*state)
    st = None
    for s in range(scans):
        st = scan(f, *syn.odometry(s), meas(s))[3]
    snap = f.snapshot()
    info = info_of(snap)                                          # fs2_snapshot_check accepts it
    cnt = f.get_state()[4]
    assert info["rows"] == (int(cnt.max()) + 7) // 8 and info["num_particles"] == N
    if expect:
        expect(info, st)
    g = make(N, cap, **kw)
    g.restore(snap)
    assert same_state(f.get_state(), g.get_state())
    assert np.array_equal(g.snapshot(), snap)
    rf, rg = (scan(h, *syn.odometry(scans), meas(scans)) for h in (f, g))
    assert same_scan(rf, rg)
    assert same_state(f.get_state(), g.get_state())
    f.close()
    g.close()
    return info


def test_edge_one_particle_empty_map():
    import fs2_synthetic as syn
    state = (np.zeros(1), np.zeros(1), np.zeros(1), np.ones(1), np.zeros(1, np.int32), np.zeros((1, 1, 6)))

    def expect(info, st):
        assert (info["rows"], info["pages"], info["records"]) == (0, 0, 0)
    roundtrip(1, state, 16, 0, lambda s: syn.scan_measurements(4, s, 0), expect)


def test_edge_ragged_counts_two_workgroups():
    import fs2_synthetic as syn
    info = roundtrip(257, ragged_state(257, [0, 1, 7, 8, 9, 17], 5), 40, 2, lambda s: syn.scan_measurements(17, s, 5))
    assert info["pages"] > 257


def test_edge_more_than_one_sweep_block():
    import fs2_synthetic as syn
    N, L = 600, 64
    # hits only: no append, so every particle keeps its 8 private pages
    info = roundtrip(N, ragged_state(N, [L], 6), L + 8, 1,
                     lambda s: syn.scan_measurements(L, s, 6, with_miss=False))
    assert info["pages"] >= 4800 > 4096


def test_edge_live_pages_fill_whole_count_blocks():
    """The count kernel's workgroup covers 4096 ids: 512 x 8 private pages fill one
    exactly (no partly filled last block)."""
    import fs2_synthetic as syn
    N, L = 512, 64

    def expect(info, st):
        assert info["pages"] == 4096 and st.appends == 0 and not st.resampled, info
    roundtrip(N, ragged_state(N, [L], 7), L + 8, 1,
              lambda s: syn.scan_measurements(L, s, 7, with_miss=False), expect)


def test_edge_maps_longer_than_the_row_boxes():
    import fs2_synthetic as syn
    L = 2056                                                      # 257 rows > kBBoxRows = 256
    info = roundtrip(2, ragged_state(2, [L], 8), L + 8, 1, lambda s: syn.scan_measurements(L, s, 8))
    assert info["rows"] >= 257


def test_edge_sparse_pools_after_collections():
    N, L = 300, 16

    def misses(s):                                                # four appends per particle and scan
        return np.array([[100.0 + 10.0 * s + 20.0 * k, 0.25 * k + 0.01 * s] for k in range(4)])

    def expect(info, st):
        assert st.collections > 0, st.collections
    roundtrip(N, ragged_state(N, [L], 9), L + 40, 5, misses, expect, page_pool=N * 2 + 4 * N + 64,
              record_pool=N * L + 6 * N)


# ------------------------------------------------------ used handle, errors ---

def test_restore_over_a_used_handle():
    import fs2_synthetic as syn
    N = 257
    src = make(N, 40)
    src.set_state(*ragged_state(N, [0, 1, 7, 8, 9, 17], 5))
    scan(src, *syn.odometry(0), syn.scan_measurements(17, 0, 5))
    snap = src.snapshot()
    src.close()
    used = make(N, 80)
    used.set_state(*ragged_state(N, [40], 11))                    # another workload, longer maps
    for s in range(3):
        scan(used, *syn.odometry(s), syn.scan_measurements(40, s, 11))
    assert int(used.get_state()[4].max()) > info_of(snap)["max_count"]
    fresh = make(N, 80)
    used.restore(snap)
    fresh.restore(snap)
    assert same_state(used.get_state(), fresh.get_state())
    assert np.array_equal(used.snapshot(), fresh.snapshot())
    ru, rf = (scan(h, *syn.odometry(1), syn.scan_measurements(17, 1, 5)) for h in (used, fresh))
    assert same_scan(ru, rf)
    assert same_state(used.get_state(), fresh.get_state())
    used.close()
    fresh.close()


def test_errors_leave_the_handle_unchanged():
    import fs2_synthetic as syn
    from fast_slam_2 import _native as nat
    lib = nat.load()
    N = 64
    f = make(N, 40)
    f.set_state(*ragged_state(N, [17, 9], 5))       # (no scan: every page is owned, the counts are known)
    before = f.get_state()
    snap = f.snapshot()

    def load(h, buf):
        a = np.ascontiguousarray(buf)
        return lib.fs2_snapshot_load(h._h, a.ctypes.data, a.size)

    # capacity one byte short: FS2_ERR_ARG, nothing written, *size set
    out = np.full(snap.size, 0xAB, dtype=np.uint8)
    size = C.c_int64(-1)
    assert lib.fs2_snapshot_save(f._h, out.ctypes.data, snap.size - 1, C.byref(size)) == nat.FS2_ERR_ARG
    assert size.value == snap.size and np.all(out == 0xAB)
    assert same_state(f.get_state(), before)
    # a snapshot of another particle count
    g = make(N + 1, 40)
    g.set_state(*ragged_state(N + 1, [3], 5))
    assert load(f, g.snapshot()) == nat.FS2_ERR_ARG
    g.close()
    assert same_state(f.get_state(), before)
    # a row entry == U: refused by the check before anything the handle reads changes
    bad = snap.copy()
    rows = sc.section(bad, sc.ROWS, "<u4")
    rows[1] = int(sc.header(bad)["pages"][0]) | (int(rows[1]) & sc.OWNED)
    assert load(f, bad) == nat.FS2_ERR_ARG
    assert same_state(f.get_state(), before)
    # a page with an owner and a sharer: met by the check kernel's second pass alone
    bad = snap.copy()
    rows = sc.section(bad, sc.ROWS, "<u4")
    # (row 0 of two of the even particles: their maps are equally long, so the page's
    # mirrors pass the first pass for either)
    even = np.arange(0, N, 2)
    owned = even[(rows[even] & sc.OWNED) != 0]
    assert owned.size, "no owned first page in the snapshot"
    other = even[even != owned[0]][0]
    rows[other] = int(rows[owned[0]]) & ~sc.OWNED
    assert load(f, bad) == nat.FS2_ERR_ARG
    assert "owned" in nat.last_error(f._h)
    assert same_state(f.get_state(), before)
    # maps above max_landmark_capacity
    small = make(N, 8, max_landmark_capacity=16)
    small.set_state(*ragged_state(N, [5], 5))
    sb = small.get_state()
    assert load(small, snap) == nat.FS2_ERR_CAPACITY
    assert same_state(small.get_state(), sb)
    small.close()
    # between step_submit and step_wait
    f.step_submit(*syn.odometry(1), np.ascontiguousarray(syn.scan_measurements(17, 1, 5)))
    assert lib.fs2_snapshot_save(f._h, None, 0, C.byref(size)) == nat.FS2_ERR_STATE
    assert load(f, snap) == nat.FS2_ERR_STATE
    f.step_wait()
    f.close()
    # the sharded path
    sh = make(N, 40, reduce="parallel", sharded_path=True, comm_mode="local", comm_id=os.urandom(128))
    sh.set_state(*ragged_state(N, [17, 9], 5))
    sb = sh.get_state()
    assert lib.fs2_snapshot_save(sh._h, None, 0, C.byref(size)) == nat.FS2_ERR_STATE
    assert load(sh, snap) == nat.FS2_ERR_STATE
    assert same_state(sh.get_state(), sb)
    sh.close()


def test_guards_after_save_and_restore():
    """FS2_GUARD=1 (set around the creation only): no snapshot kernel writes past a
    buffer fs2_create made."""
    import fs2_synthetic as syn
    from fast_slam_2 import _native as nat
    N = 257
    old = os.environ.get("FS2_GUARD")
    os.environ["FS2_GUARD"] = "1"
    try:
        f = make(N, 40)
    finally:
        if old is None:
            os.environ.pop("FS2_GUARD", None)
        else:
            os.environ["FS2_GUARD"] = old
    f.set_state(*ragged_state(N, [0, 1, 7, 8, 9, 17], 5))
    scan(f, *syn.odometry(0), syn.scan_measurements(17, 0, 5))
    snap = f.snapshot()
    f.restore(snap)
    name = C.create_string_buffer(128)
    bad = nat.load().fs2_debug_check_guards(f._h, name, 128)
    assert bad == 0, f"{bad} guard bytes overwritten after buffer {name.value.decode()}"
    assert np.array_equal(f.snapshot(), snap)
    f.close()
