"""The map readout on the device (fs2_map_summary / fs2_map_density)
against the dense maps of get_state().

The reference forms every live landmark (i, j), j < cnt_i, from the downloaded
[N][cap][6] maps and bins it with np.add.at by the formulas of fs2.h: cell
(floor((mx - x0) / cell), floor((my - y0) / cell)), amount 1 or q_i = rint(w_i 2^e) with
e = fs2_density_scale(wmax, max(T, 1)).  Everything is an integer or a minimum / maximum,
so every comparison is exact: np.array_equal on raw uint64 grids, == on counts and on the
bounding box.

Non-finite landmark means are not tested here (the rule of fs2.h stands as written): an
import of one would also reach the handle's import extent and row boxes, which are not
this readout's ground."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COV = 0.01
STAT_FIELDS = ("resampled", "n_eff", "total_weight", "best_index", "hits", "appends", "max_count")


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


def check_guards(f):
    from fast_slam_2 import _native as nat
    name = C.create_string_buffer(128)
    bad = nat.load().fs2_debug_check_guards(f._h, name, 128)
    assert bad == 0, f"{bad} guard bytes overwritten after buffer {name.value.decode()}"


def dense_maps(N, cap, seed, lo, hi):
    """[N][cap][6] maps with means uniform in [lo, hi)^2."""
    rng = np.random.default_rng([seed, 31])
    lm = np.zeros((N, max(cap, 1), 6))
    lm[:, :, 0:2] = rng.uniform(lo, hi, (N, max(cap, 1), 2))
    lm[:, :, 2] = COV
    lm[:, :, 5] = COV
    return lm


def upload(f, cnt, lm, w, seed=0):
    import fs2_synthetic as syn
    N = len(cnt)
    x, y, yaw = syn.particle_poses(N, seed)
    f.set_state(x, y, yaw, w, np.asarray(cnt, dtype=np.int32), lm)


def live_landmarks(state):
    """(particle index, mx, my) of every live landmark of get_state()'s arrays."""
    cnt, lm = state[4], state[5]
    live = np.arange(lm.shape[1])[None, :] < cnt[:, None]
    pi = np.broadcast_to(np.arange(len(cnt))[:, None], live.shape)[live]
    return pi, lm[:, :, 0][live], lm[:, :, 1][live]


def ref_summary(state):
    cnt = state[4].astype(np.int64)
    _, mx, my = live_landmarks(state)
    inf = float("inf")
    bbox = [np.fmin.reduce(mx, initial=inf), np.fmin.reduce(my, initial=inf),
            np.fmax.reduce(mx, initial=-inf), np.fmax.reduce(my, initial=-inf)]
    return int(cnt.sum()), int(((cnt + 7) // 8).sum()), int(cnt.max()), bbox


def ref_density(state, x0, y0, cell, nx, ny, weighted):
    """(grid, outside, e, sum_i q_i cnt_i) by the formulas of fs2.h."""
    from fast_slam_2 import _native as nat
    w, cnt = state[3], state[4].astype(np.int64)
    N, T = len(w), int(cnt.sum())
    e = 0
    q = np.ones(N, dtype=np.uint64)
    if weighted:
        ce = C.c_int32()
        nat.check(nat.load().fs2_density_scale(float(w.max()), max(T, 1), C.byref(ce)))
        e = ce.value
        q = np.rint(np.ldexp(w, e)).astype(np.uint64)
    pi, mx, my = live_landmarks(state)
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = np.floor((mx - x0) / cell), np.floor((my - y0) / cell)
        inside = (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny)
    grid = np.zeros((ny, nx), dtype=np.uint64)
    ql = q[pi]
    np.add.at(grid, (fy[inside].astype(np.int64), fx[inside].astype(np.int64)), ql[inside])
    total = int((q * cnt.astype(np.uint64)).sum(dtype=np.uint64))
    return grid, int(ql[~inside].sum(dtype=np.uint64)), e, total


def check_density(f, state, x0, y0, cell, nx, ny, label="", ways=(True, False)):
    for weighted in ways:
        grid, outside, origin, c, e = f.map_density((ny, nx), (x0, y0), cell, weighted=weighted, raw=True)
        rg, rout, re_, total = ref_density(state, x0, y0, cell, nx, ny, weighted)
        assert grid.dtype == np.uint64 and grid.shape == (ny, nx)
        assert e == re_ and origin == (x0, y0) and c == cell, (label, weighted)           # scale_exp
        assert np.array_equal(grid, rg), (label, weighted)                                # the grid
        assert outside == rout, (label, weighted)                                         # outside
        assert int(grid.sum(dtype=np.uint64)) + outside == total, (label, weighted)       # sum_i q_i cnt_i
        fg, fo, _, _ = f.map_density((ny, nx), (x0, y0), cell, weighted=weighted)
        assert fg.dtype == np.float64 and np.array_equal(fg, np.ldexp(rg.astype(np.float64), -re_))
        assert fo == math.ldexp(float(rout), -re_)
    return rg


def check_summary(f, state, label="", shared=False):
    ms = f.map_summary()
    T, R, mc, bbox = ref_summary(state)
    assert (ms.landmarks, ms.page_refs, ms.max_count) == (T, R, mc), label
    assert ms.pages <= R if shared else ms.pages == R, (label, ms.pages, R)
    assert ms.bbox.shape == (4,) and np.array_equal(ms.bbox, bbox), (label, ms.bbox, bbox)
    return ms


# ------------------------------------------------------- dense maps (set_state) ---

DENSE_CAP = 17


def dense_counts(N):
    """name -> cnt: the uniform page edges, and a ragged draw from 0..17 with some zeros."""
    cases = {f"L={L}": np.full(N, L) for L in (0, 1, 7, 8, 9, 17)}
    rng = np.random.default_rng([N, 5])
    rag = rng.integers(0, DENSE_CAP + 1, N)
    rag[rng.choice(N, max(N // 8, 1), replace=False)] = 0
    if N > 1:
        rag[N - 1] = DENSE_CAP
    cases["ragged"] = rag
    return cases


@pytest.mark.parametrize("N", [1, 64, 257, 4099])
def test_dense_maps_match_get_state(N):
    f = make(N, landmark_capacity=24)
    w = weights(N, N)
    lm = dense_maps(N, DENSE_CAP, N, -3.0, 3.0)
    for name, cnt in dense_counts(N).items():
        upload(f, cnt, lm, w)
        state = f.get_state()
        assert np.array_equal(state[4], cnt) and np.array_equal(state[3], w)
        label = f"N={N} {name}"
        check_summary(f, state, label)                       # nothing shared: U = R
        # a window smaller than the spread (some landmarks outside), 10 cm cells
        check_density(f, state, -2.5, -2.5, 0.1, 50, 48, label)
    f.close()


def test_null_outputs_and_shapes():
    from fast_slam_2 import _native as nat
    N = 64
    f = make(N, landmark_capacity=24)
    upload(f, np.full(N, 9), dense_maps(N, 9, 1, -1.0, 1.0), weights(N, 1))
    lib = nat.load()
    counts, bbox = np.empty(4, dtype=np.int64), np.empty(4)
    nat.check(lib.fs2_map_summary(f._h, None, None), f._h)
    nat.check(lib.fs2_map_summary(f._h, None, nat.ptr(counts)), f._h)
    nat.check(lib.fs2_map_summary(f._h, nat.ptr(bbox), None), f._h)
    ms = f.map_summary()
    assert counts.tolist() == [ms.landmarks, ms.page_refs, ms.pages, ms.max_count] == [9 * N, 2 * N, 2 * N, 9]
    assert np.array_equal(bbox, ms.bbox)
    grid = np.zeros((4, 4), dtype=np.uint64)
    nat.check(lib.fs2_map_density(f._h, 0, -1.0, -1.0, 0.5, 4, 4, nat.ptr(grid), None, None), f._h)
    assert grid.sum() == 9 * N
    f.close()


# ------------------------------------------------- filter-built, shared maps ---

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


def test_filter_built_shared_maps_match_get_state():
    """Scans after the resample append into pages the siblings share (copy-on-write): every
    referent of a page must still agree on its fill."""
    import fast_slam_2
    import fs2_synthetic as syn
    from fast_slam_2.algorithms.fast_slam_2 import fit_density_window
    N, L, scans = 4099, 12, 6
    f = make(N, seed=11, landmark_capacity=L + 4 * scans + 8)
    populate(f, N, L)
    base = syn.common_landmarks(L, 0)
    shared_seen, appended_after = [], []

    def readout(s, st):
        state = f.get_state()
        shared = bool(shared_seen) or bool(st.resampled)
        ms = check_summary(f, state, f"scan {s}", shared=shared)
        (x0, y0), cell = fit_density_window(ms.bbox, (128, 128))
        check_density(f, state, x0, y0, cell, 128, 128, f"scan {s} fitted")
        assert f.map_density((128, 128), (x0, y0), cell, weighted=False, raw=True)[1] == 0
        # 1 cm cells about one landmark: most of the map outside
        check_density(f, state, base[0, 0] - 0.32, base[0, 1] - 0.32, 0.01, 64, 64, f"scan {s} tight")
        if shared_seen and st.appends:
            appended_after.append(s)
        if st.resampled and not shared_seen:
            assert ms.pages < ms.page_refs                                   # sharing really occurred
            assert ms.pages == fast_slam_2.FastSLAM2.snapshot_info(f.snapshot())["pages"]
            shared_seen.append(s)

    _, resampled_at = run_scans(f, N, L, scans, readout)
    assert resampled_at and shared_seen == resampled_at[:1]
    assert appended_after, "no scan appended after the first resample"
    f.close()


# ------------------------------------------------------------ record, not mirror ---

def test_bins_the_fp64_record_not_the_fp32_mirror():
    xm = 0.25 - 2.0 ** -40
    assert np.float32(xm) == np.float32(0.25) and math.floor(xm / 0.25) == 0
    f = make(1, landmark_capacity=8)
    lm = dense_maps(1, 1, 0, 0.0, 1.0)
    lm[0, 0, 0:2] = (xm, 0.1)
    upload(f, [1], lm, np.array([1.0]))
    state = f.get_state()
    assert state[5][0, 0, 0] == xm
    grid, outside = f.map_density((4, 4), (0.0, 0.0), 0.25, weighted=False, raw=True)[:2]
    assert outside == 0 and grid[0, 0] == 1 and grid.sum() == 1              # column 0, not column 1
    check_density(f, state, 0.0, 0.0, 0.25, 4, 4, "record")
    f.close()


# --------------------------------------------------------------------- edges ---

def test_window_edges_and_thin_grids():
    N, L = 257, 9
    f = make(N, landmark_capacity=16)
    w = weights(N, 21)
    lm = dense_maps(N, L, 21, 0.0, 4.0)
    x0, y0, cell, nx, ny = -0.75, -0.5, 0.25, 19, 18          # the spread lies inside: [0, 4)^2
    lm[0, 0, 0] = x0                                          # exactly at x0: column 0
    lm[1, 0, 0] = x0 + nx * cell                              # exactly at the far edge (4.0): outside
    lm[2, 8, 1] = y0 + ny * cell                              # (slot 8: the second page)
    lm[3, 0, 1] = y0                                          # row 0
    lm[5, 8, 0] = x0 - 1e-9                                   # just below x0
    upload(f, np.full(N, L), lm, w)
    state = f.get_state()
    assert np.array_equal(state[5][:, :L], lm[:, :L])
    check_density(f, state, x0, y0, cell, nx, ny, "edges")
    grid, outside = f.map_density((ny, nx), (x0, y0), cell, weighted=False, raw=True)[:2]
    assert outside == 3 and grid[:, 0].sum() == 1 and grid[0, :].sum() == 1 and grid.sum() == N * L - 3
    for gy, gx in ((1, 1), (1, 17), (17, 1)):
        check_density(f, state, 1.0, 1.5, 0.125, gx, gy, f"{gy}x{gx}")
    f.close()


def table_home(c):
    """The bin pass's table slot a cell index starts probing at (fs2_mapreadout.hip
    k_map_bin: multiplicative hash, the top 10 bits of the low 32)."""
    return ((c * 2654435761) & 0xFFFFFFFF) >> 22


def test_table_full_path_adds_straight_to_memory():
    """The bin pass's exit when a lane finds its table neighbourhood full.  Every landmark
    lies in one of K cells of a 300 x 300 grid that all start probing at the same table slot,
    so whatever a workgroup meets, those cells can only ever take the 8 slots a lane probes
    (kMbProbes).  Every page is full and holds 8 different such cells, and no two pages hold
    the same 8: any workgroup that opens two pages meets at least 9 of the cells, and a 9th
    cell's lanes find all 8 slots taken by other cells and add to memory.  The pass runs at
    most 2048 workgroups (kMrGrid) and there are 2 N = 8198 pages, so some workgroup opens
    at least two (pigeonhole; by the pool's layout nearly all do), whatever ids the pages
    got.  A lane that added both ways, or neither, on that exit would break the equality."""
    N, L, K, nx, ny = 4099, 16, 20, 300, 300
    homes = {}
    for c in range(nx * ny):
        homes.setdefault(table_home(c), []).append(c)
    cells = np.array(next(v for _, v in sorted(homes.items()) if len(v) >= K)[:K])
    assert len({table_home(int(c)) for c in cells}) == 1 and len(set(cells.tolist())) == K
    rng = np.random.default_rng(17)
    subsets, seen = [], set()
    while len(subsets) < 2 * N:                               # pairwise different 8-subsets of the K cells
        s = rng.permutation(K)[:8]
        key = frozenset(s.tolist())
        if key not in seen:
            seen.add(key)
            subsets.append(s)
    pick = cells[np.array(subsets)].reshape(N, L)             # particle i: pages 2 i and 2 i + 1
    lm = dense_maps(N, L, 0, 0.0, 1.0)
    jit = rng.uniform(0.05, 0.95, (N, L, 2))
    lm[:, :, 0] = pick % nx + jit[:, :, 0]
    lm[:, :, 1] = pick // nx + jit[:, :, 1]
    f = make(N, landmark_capacity=L + 8)
    upload(f, np.full(N, L), lm, weights(N, 5))
    state = f.get_state()
    assert np.array_equal(state[5][:, :L, 0:2], lm[:, :, 0:2])
    g = check_density(f, state, 0.0, 0.0, 1.0, nx, ny, "table full")
    assert sorted(np.flatnonzero(g.ravel()).tolist()) == sorted(cells.tolist())
    assert f.map_summary().pages == 2 * N
    f.close()


def test_debug_map_times_reports_the_three_stages():
    """fs2_debug_map_times: with timing on, a call leaves the device time of each of its
    three stages (all of them run in both calls); with timing off, a call leaves the
    figures alone; a call that fails before its last stage leaves them alone too."""
    from fast_slam_2 import _native as nat
    N, L = 4099, 9
    f = make(N, landmark_capacity=16)
    w = weights(N, 6)
    lm = dense_maps(N, L, 6, 0.0, 4.0)
    upload(f, np.full(N, L), lm, w)
    lib = nat.load()
    ms = np.full(3, -1.0)
    try:
        assert lib.fs2_debug_map_times(1, None) == 0
        f.map_summary()
        assert lib.fs2_debug_map_times(-1, nat.ptr(ms)) == 0
        assert np.all(ms > 0.0) and np.all(ms < 1000.0), ms          # counts, tally, summary pass
        summary_ms = ms.copy()
        for weighted in (True, False):
            f.map_density((64, 64), (0.0, 0.0), 0.0625, weighted=weighted)
            assert lib.fs2_debug_map_times(-1, nat.ptr(ms)) == 0
            assert np.all(ms > 0.0) and np.all(ms < 1000.0), ms      # weights + counts, tally, zeroing + bin pass
        assert not np.array_equal(ms, summary_ms)                    # the last call's, not the first's
        last = ms.copy()
        bad = w.copy()
        bad[7] = -1.0
        upload(f, np.full(N, L), lm, bad)
        with pytest.raises(nat.FS2Error):
            f.map_density((64, 64), (0.0, 0.0), 0.0625)              # fails after its first stage
        assert lib.fs2_debug_map_times(0, nat.ptr(ms)) == 0 and np.array_equal(ms, last)
        f.map_summary()                                              # timing off
        assert lib.fs2_debug_map_times(-1, nat.ptr(ms)) == 0 and np.array_equal(ms, last)
    finally:
        lib.fs2_debug_map_times(0, None)
    f.close()


def test_spread_over_a_large_grid_and_packed_into_one_cell():
    N, L = 4099, 9
    f = make(N, landmark_capacity=16)
    w = weights(N, 8)
    # ~37000 landmarks over 90000 cells, a handful of them per workgroup: the table's
    # ordinary path with many distinct keys (the table-full exit has its own test above)
    lm = dense_maps(N, L, 8, 0.0, 300.0)
    upload(f, np.full(N, L), lm, w)
    state = f.get_state()
    g = check_density(f, state, 0.0, 0.0, 1.0, 300, 300, "spread")
    assert np.count_nonzero(g) > 20000
    check_summary(f, state, "spread")
    # every landmark of every particle in one cell of a 256 x 256 grid
    lm = dense_maps(N, L, 9, 0.5031, 0.5069)
    upload(f, np.full(N, L), lm, w)
    state = f.get_state()
    g = check_density(f, state, 0.0, 0.0, 0.01, 256, 256, "one cell")
    assert np.count_nonzero(g) == 1
    f.close()


# -------------------------------------------------------------- fitted window ---

@pytest.mark.parametrize("shape", [(256, 256), (1, 1), (17, 1), (3, 40)])
def test_fitted_window_holds_every_landmark(shape):
    from fast_slam_2.algorithms.fast_slam_2 import fit_density_window
    N, L = 257, 9
    f = make(N, landmark_capacity=16)
    lm = dense_maps(N, L, 4, -11.0, 3.0)
    upload(f, np.full(N, L), lm, weights(N, 4))
    state = f.get_state()
    grid, outside, origin, cell, e = f.map_density(shape, raw=True)
    assert outside == 0
    bbox = f.map_summary().bbox
    assert (origin, cell) == fit_density_window(bbox, shape)
    ny, nx = shape
    rg, rout, re_, _ = ref_density(state, origin[0], origin[1], cell, nx, ny, True)
    assert np.array_equal(grid, rg) and rout == 0 and e == re_
    _, o2, org2, c2 = f.map_density(shape, cell=cell * 2)
    assert c2 == cell * 2 and (org2, c2) == fit_density_window(bbox, shape, cell=cell * 2)
    _, o3, org3, c3 = f.map_density(shape, origin=origin)
    assert org3 == origin and (org3, c3) == fit_density_window(bbox, shape, origin=origin) and o3 == 0.0
    f.close()


def test_empty_maps():
    N = 257
    f = make(N)
    ms = f.map_summary()
    inf = float("inf")
    assert (ms.landmarks, ms.page_refs, ms.pages, ms.max_count) == (0, 0, 0, 0)
    assert ms.bbox.tolist() == [inf, inf, -inf, -inf]
    with pytest.raises(ValueError):
        f.map_density((16, 16))                               # no window to fit
    with pytest.raises(ValueError):
        f.map_density((16, 16), cell=0.5)
    for weighted in (True, False):
        grid, outside, _, _, e = f.map_density((16, 16), (0.0, 0.0), 1.0, weighted=weighted, raw=True)
        assert not grid.any() and outside == 0
    f.close()


# ------------------------------------------------- bad arguments, bad weights ---

def test_density_bad_arguments():
    from fast_slam_2 import _native as nat
    N = 64
    f = make(N, landmark_capacity=16)
    upload(f, np.full(N, 3), dense_maps(N, 3, 2, 0.0, 4.0), weights(N, 2))
    lib = nat.load()
    grid = np.full((4, 4), 12345, dtype=np.uint64)

    def call(cell=1.0, nx=4, ny=4, g=grid, h=None):
        return lib.fs2_map_density(f._h if h is None else h, 0, 0.0, 0.0, cell, nx, ny, nat.ptr(g), None, None)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(cell=bad) == nat.FS2_ERR_ARG
    assert call(nx=0) == nat.FS2_ERR_ARG and call(ny=0) == nat.FS2_ERR_ARG and call(nx=-3) == nat.FS2_ERR_ARG
    assert call(nx=4097, ny=4096) == nat.FS2_ERR_ARG          # nx ny > 2^24 (checked before the grid is touched)
    assert call(g=None) == nat.FS2_ERR_ARG
    assert np.all(grid == 12345)                              # nothing written on error
    assert lib.fs2_map_density(None, 0, 0.0, 0.0, 1.0, 4, 4, nat.ptr(grid), None, None) == nat.FS2_ERR_ARG
    assert lib.fs2_map_summary(None, None, None) == nat.FS2_ERR_ARG
    assert call() == 0 and grid.sum() == 3 * N
    with pytest.raises(ValueError):
        f.map_density((4, 4), (0.0, 0.0), -2.0)
    f.close()
    for fn in (f.map_summary, lambda: f.map_density((4, 4)), lambda: f.map_density((4, 4), (0.0, 0.0), 1.0)):
        with pytest.raises(nat.FS2Error):
            fn()


@pytest.mark.parametrize("kind", ["zeros", "negative", "nan"])
def test_invalid_weights_are_a_state_error_and_write_nothing(kind):
    from fast_slam_2 import _native as nat
    N, L = 4099, 9
    f = make(N, landmark_capacity=16)
    w = weights(N, 1)
    if kind == "zeros":
        w[:] = 0.0
    elif kind == "negative":
        w[2500] = -1e-9
    else:
        w[4098] = float("nan")
    upload(f, np.full(N, L), dense_maps(N, L, 1, 0.0, 2.0), w)
    lib = nat.load()
    grid = np.full((8, 8), 12345, dtype=np.uint64)
    e, out = C.c_int32(-99), C.c_uint64(77)
    rc = lib.fs2_map_density(f._h, 1, 0.0, 0.0, 0.25, 8, 8, nat.ptr(grid), C.byref(e), C.byref(out))
    assert rc == nat.FS2_ERR_STATE and nat.last_error(f._h)
    assert np.all(grid == 12345) and e.value == -99 and out.value == 77
    with pytest.raises(nat.FS2Error):
        f.map_density((8, 8), (0.0, 0.0), 0.25)
    # the unweighted form and the summary do not read the weights
    assert f.map_density((8, 8), (0.0, 0.0), 0.25, weighted=False, raw=True)[0].sum() == N * L
    assert f.map_summary().landmarks == N * L
    f.close()


# ----------------------------------------------------------- non-interference ---

def test_readouts_do_not_change_the_filter():
    N, L, scans = 4099, 12, 6
    a, b = make(N, seed=11, landmark_capacity=L + 4 * scans + 8), make(N, seed=11, landmark_capacity=L + 4 * scans + 8)
    populate(a, N, L)
    populate(b, N, L)

    def readout(s, st):
        a.map_summary()
        a.map_density((256, 256))
        a.map_density((300, 300), (-150.0, -150.0), 1.0, weighted=False)

    ra, res_a = run_scans(a, N, L, scans, readout)
    rb, res_b = run_scans(b, N, L, scans, None)
    assert res_a == res_b and len(res_a) >= 1
    for u, v in zip(ra, rb):
        assert np.array_equal(u[0], v[0]) and u[1] == v[1] and np.array_equal(u[2], v[2])
    for u, v in zip(a.get_state(), b.get_state()):
        assert u.shape == v.shape and np.array_equal(u, v)
    a.close()
    b.close()


def test_readouts_write_past_no_buffer():
    """FS2_GUARD: the readout's scratch is sized from the pool at the time of the call, so
    it is remade when the pool has grown; two grid sizes remake the grid."""
    import fs2_synthetic as syn
    N, L = 20011, 12
    f = make(N, seed=3, guard=True, landmark_capacity=L + 32, page_pool=3 * N)
    f.map_summary()                                           # scratch for the pool as created: 3 N pages
    f.map_density((16, 16), (0.0, 0.0), 1.0)
    check_guards(f)
    populate(f, N, L)
    pools, appends = [], 0
    for s in range(4):
        _, st = f.step(*syn.odometry(s), np.ascontiguousarray(syn.scan_measurements(L, s, 0)))
        pools.append(int(st.pool_pages))
        appends += int(st.appends)
        f.map_summary()
        f.map_density((256, 256))
        f.map_density((300, 7), (-1.0, -1.0), 0.01, weighted=False)        # (another grid size: the buffer is remade)
        check_guards(f)
    assert appends > 0 and pools[0] > 3 * N, pools                         # the calls in the loop: after a pool growth
    f.close()


def test_pending_scan_refuses_the_readouts():
    import fs2_synthetic as syn
    from fast_slam_2 import _native as nat
    N, L = 4099, 12
    f = make(N, landmark_capacity=L + 16)
    populate(f, N, L)
    f.step_submit(*syn.odometry(0), np.ascontiguousarray(syn.scan_measurements(L, 0, 0)))
    for fn in (f.map_summary, lambda: f.map_density((16, 16)), lambda: f.map_density((16, 16), (0.0, 0.0), 1.0)):
        with pytest.raises(nat.FS2Error) as ei:
            fn()
        assert ei.value.code == nat.FS2_ERR_STATE
    f.step_wait()
    ms = f.map_summary()
    assert ms.landmarks >= N * L and f.map_density((16, 16), raw=True)[1] == 0
    f.close()


def test_two_calls_and_another_handle_in_between_give_identical_grids():
    N, L = 4099, 17
    f = make(N, landmark_capacity=24)
    upload(f, np.full(N, L), dense_maps(N, L, 2, -3.0, 3.0), weights(N, 2))
    a = f.map_density((64, 64), raw=True)
    b = f.map_density((64, 64), raw=True)
    sa = f.map_summary()
    g = make(257, seed=8, landmark_capacity=16)
    upload(g, np.full(257, 9), dense_maps(257, 9, 3, -1.0, 1.0), weights(257, 3))
    g.map_summary()
    g.map_density((64, 64))
    g.close()
    c = f.map_density((64, 64), raw=True)
    sc = f.map_summary()
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    assert np.array_equal(a[0], c[0]) and a[1:] == c[1:]
    assert sa[:4] == sc[:4] and np.array_equal(sa.bbox, sc.bbox)
    f.close()
