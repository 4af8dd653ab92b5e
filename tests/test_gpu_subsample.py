"""The weighted subsample on the device (fs2_subsample) against numpy.

The draw is integer arithmetic, so the reference is exact and every comparison is
np.array_equal:

    q   = np.rint(np.ldexp(w, e)).astype(np.uint64)      (ones when not weighted, e = 0)
    C   = np.cumsum(q, dtype=np.uint64),  Q = C[-1]
    t_j = (j Q + ((offset Q) >> 32)) // k                 (Python integers)
    idx = np.searchsorted(C, t, side="right")

Sizes: the wave (64), workgroup (256) and chunk (2048) edges, several chunks, and
N_TWO_TURNS = 256 * 2048 + 1 = 524289, the smallest n at which the one workgroup that
scans the chunk totals (256 totals a turn) takes a second turn."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_posterior import check_guards, cloud, make, populate, run_scans, weights

pytestmark = pytest.mark.gpu

N_TWO_TURNS = 256 * 2048 + 1
NS = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4099, 70001, N_TWO_TURNS]
LARGE = (70001, N_TWO_TURNS)                  # the two largest: offset 2^31 alone
OFFSETS = [0, 2 ** 31, 2 ** 32 - 1]
MID = 2 ** 31


def ks(n):
    return sorted({k for k in (1, 2, 63, 64, 65, n - 1, n, n + 1, 3 * n + 7) if 1 <= k <= 2 ** 30})


def density_scale(wmax, n):
    from fast_slam_2 import _native as nat
    e = C.c_int32()
    nat.check(nat.load().fs2_density_scale(float(wmax), int(n), C.byref(e)))
    return e.value


class Amounts:
    """q, its prefix and total for one weight vector (formed once, shared, never changed)."""

    def __init__(self, w=None, n=None):
        if w is None:
            self.e, self.q = 0, np.ones(n, dtype=np.uint64)
        else:
            self.e = density_scale(w.max(), len(w))
            self.q = np.rint(np.ldexp(w, self.e)).astype(np.uint64)
        self.C = np.cumsum(self.q, dtype=np.uint64)
        self.Q = int(self.C[-1])
        self.qo = self.q.astype(object)                      # Python integers, for the multiplicity bound
        assert self.Q == sum(self.qo) <= 2 ** 62             # (the uint64 prefix did not wrap)
        self.qmax = int(self.q.max())
        for a in (self.q, self.C):
            a.setflags(write=False)

    def idx(self, k, offset):
        Q, s = self.Q, (offset * self.Q) >> 32
        if k * Q + s < 2 ** 63:                              # the same integers, exactly, in int64
            t = ((np.arange(k, dtype=np.int64) * Q + s) // k).astype(np.uint64)
        else:
            t = np.array([(j * Q + s) // k for j in range(k)], dtype=np.uint64)
        assert int(t[-1]) < Q
        return np.searchsorted(self.C, t, side="right").astype(np.int64)

    def excess(self, m, k):
        """|k q_i - m_i Q| per particle, exact (int64 where the products fit, else Python integers)."""
        if k * self.qmax < 2 ** 62 and int(m.max()) * self.Q < 2 ** 62:
            return np.abs(self.q.astype(np.int64) * k - m.astype(np.int64) * self.Q)
        return np.abs(self.qo * k - m.astype(object) * self.Q)


def check_draw(sub, am, k, offset, label):
    """sub against the reference, then the properties that do not use its formula."""
    n = len(am.q)
    assert sub.idx.dtype == np.int64 and sub.idx.shape == (k,), label
    assert sub.total == am.Q and sub.scale_exp == am.e, label
    assert np.array_equal(sub.idx, am.idx(k, offset)), label
    assert sub.idx.min() >= 0 and sub.idx.max() < n and np.all(np.diff(sub.idx) >= 0), label
    m = np.bincount(sub.idx, minlength=n)
    assert not np.any(m[am.q == 0]), label                   # a zero amount is never drawn
    assert np.all(am.excess(m, k) < am.Q), label             # |k q_i - m_i Q| < Q


# -------------------------------------------------------------- the reference ---

@pytest.mark.parametrize("n", NS)
def test_draws_match_numpy(n):
    f = make(n)
    x, y, yaw = cloud(n, seed=n)
    w = weights(n, n)
    f.set_state(x, y, yaw, w)
    if n >= 63:
        assert np.count_nonzero(w == 0.0) == 3
    weighted, flat = Amounts(w), Amounts(n=n)
    for k in ks(n):
        for offset in ([MID] if n in LARGE else OFFSETS):
            check_draw(f.subsample(k, offset), weighted, k, offset, f"n={n} k={k} offset={offset} weighted")
            check_draw(f.subsample(k, offset, weighted=False), flat, k, offset, f"n={n} k={k} offset={offset} flat")
    a, b = f.subsample(min(n, 257)), f.subsample(min(n, 257), MID, True)     # offset=None is 2^31
    assert np.array_equal(a.idx, b.idx)
    f.close()


@pytest.mark.parametrize("n", [257, 4099])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_all_weight_on_one_particle(n, where):
    i = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    f = make(n)
    w = np.zeros(n)                                          # ("last": particle 0 at weight 0 too)
    w[i] = 0.37
    f.set_state(*cloud(n, seed=1), w)
    am = Amounts(w)
    for k in (1, 64, n, 3 * n + 7):
        for offset in OFFSETS:
            sub = f.subsample(k, offset)
            assert np.array_equal(sub.idx, np.full(k, i)), (k, offset)
            check_draw(sub, am, k, offset, f"{where} k={k}")
    f.close()


@pytest.mark.parametrize("n", [257, 4099])
def test_equal_weights_give_the_unweighted_draw(n):
    f = make(n)
    f.set_state(*cloud(n, seed=2), np.full(n, 0.003))
    for k in (1, 65, n - 1, n, n + 1, 3 * n + 7):
        for offset in OFFSETS:
            a, b = f.subsample(k, offset), f.subsample(k, offset, weighted=False)
            assert np.array_equal(a.idx, b.idx), (k, offset)
            assert b.scale_exp == 0 and b.total == n and a.total % n == 0
    assert np.array_equal(f.subsample(n, 0, weighted=False).idx, np.arange(n))
    f.close()


def test_subnormal_largest_weight():
    n = 2049
    rng = np.random.default_rng([n, 3])
    w = rng.integers(0, 1000, n).astype(np.float64) * 5e-324
    w[7] = 1000 * 5e-324
    f = make(n)
    f.set_state(*cloud(n, seed=3), w)
    am = Amounts(w)
    assert am.e > 1023
    for k in (1, 64, n, 3 * n + 7):
        check_draw(f.subsample(k, 12345), am, k, 12345, f"subnormal k={k}")
    f.close()


def test_unweighted_does_not_read_the_weights():
    from fast_slam_2 import _native as nat
    n = 4099
    w = weights(n, 5)
    w[[0, 2048, 4098]] = float("nan")
    w[17] = -1.0
    f = make(n)
    f.set_state(*cloud(n, seed=4), w)
    flat = Amounts(n=n)
    for k in (1, 257, 3 * n + 7):
        check_draw(f.subsample(k, 99, weighted=False), flat, k, 99, f"nan k={k}")
    with pytest.raises(nat.FS2Error) as ei:
        f.subsample(8)
    assert ei.value.code == nat.FS2_ERR_STATE
    f.close()


def test_two_calls_return_identical_arrays():
    n = 70001
    f = make(n)
    f.set_state(*cloud(n, seed=2), weights(n, 2))
    a = f.subsample(4099, 777)
    f.subsample(3 * n + 7, 1)                                # (another shape in between)
    f.subsample(5, 2, weighted=False)
    b = f.subsample(4099, 777)
    for u, v in zip(a, b):
        assert np.array_equal(np.asarray(u), np.asarray(v))
    f.close()


# --------------------------------------------------------------------- gather ---

def ragged(f, N, L, scans=3):
    """Maps whose counts differ per particle, then a few scans of the synthetic stream."""
    import fs2_synthetic as syn
    x, y, yaw = syn.particle_poses(N, 0)
    lm = syn.particle_maps(N, L, 0)
    cnt = (L - np.arange(N) % 4).astype(np.int32)
    f.set_state(x, y, yaw, weights(N, 8) + 1e-7, cnt, lm)
    for s in range(scans):
        f.step(*syn.odometry(s), np.ascontiguousarray(syn.scan_measurements(L, s, 0)))


def raw_call(f, k, offset, weighted, want, size=None):
    """fs2_subsample with the outputs named in `want` (the rest NULL) into buffers of
    `size` (k + 8) elements prefilled with a pattern."""
    from fast_slam_2 import _native as nat
    size = k + 8 if size is None else size
    bufs = {"idx": np.full(size, -77, dtype=np.int64)}
    for name in ("x", "y", "yaw", "w"):
        bufs[name] = np.full(size, -7.5) if name in want else None
    bufs["cnt"] = np.full(size, -77, dtype=np.int32) if "cnt" in want else None
    e, total = C.c_int32(-99), C.c_uint64(77)
    rc = nat.load().fs2_subsample(f._h, weighted, k, offset, nat.ptr(bufs["idx"]) if "idx" in want else None,
                                  *(nat.ptr(bufs[name]) for name in ("x", "y", "yaw", "w", "cnt")),
                                  C.byref(e), C.byref(total))
    return rc, bufs, e.value, total.value


def untouched(bufs, e, total, first=0):
    ok = e == -99 and total == 77 if first == 0 else True
    for name, a in bufs.items():
        if a is not None:
            ok = ok and bool(np.all(a[first:] == (-7.5 if a.dtype == np.float64 else -77)))
    return ok


def test_gather_returns_the_state_at_idx():
    N, L = 4099, 12
    f = make(N, seed=11, landmark_capacity=L + 24)
    ragged(f, N, L)
    x, y, yaw, w, cnt, _ = f.get_state(lm_cap=0)
    assert len(np.unique(cnt)) > 1 and len(np.unique(w)) > 1
    state = {"x": x, "y": y, "yaw": yaw, "w": w, "cnt": cnt}
    subsets = [("x", "y", "yaw", "w", "cnt"), (), ("x",), ("cnt",), ("y", "w"), ("yaw", "cnt"), ("x", "y", "yaw")]
    for k in (1, 257, 3 * N + 7):
        sub = f.subsample(k, 4242)
        for name, got in (("x", sub.x), ("y", sub.y), ("yaw", sub.yaw), ("w", sub.w), ("cnt", sub.counts)):
            assert got.dtype == state[name].dtype
            assert np.array_equal(got.view(np.uint8), state[name][sub.idx].view(np.uint8)), (k, name)
        for want in subsets:
            rc, bufs, e, total = raw_call(f, k, 4242, 1, ("idx",) + want)
            assert rc == 0 and e == sub.scale_exp and total == sub.total
            assert np.array_equal(bufs["idx"][:k], sub.idx)
            for name in want:
                assert np.array_equal(bufs[name][:k].view(np.uint8), state[name][sub.idx].view(np.uint8)), (k, want)
            assert untouched(bufs, e, total, first=k), (k, want)          # nothing past element k
    f.close()


# --------------------------------------------------------------------- errors ---

def test_bad_arguments_write_nothing():
    from fast_slam_2 import _native as nat
    n = 257
    f = make(n)
    f.set_state(*cloud(n, seed=1), weights(n, 1))
    every = ("idx", "x", "y", "yaw", "w", "cnt")
    for k in (0, -1, 2 ** 30 + 1):
        rc, bufs, e, total = raw_call(f, k, MID, 1, every, size=64)
        assert rc == nat.FS2_ERR_ARG and untouched(bufs, e, total), k
        with pytest.raises(ValueError):
            f.subsample(k)
    rc, bufs, e, total = raw_call(f, 16, MID, 1, every[1:])               # null idx
    assert rc == nat.FS2_ERR_ARG and untouched(bufs, e, total)
    assert nat.load().fs2_subsample(None, 1, 16, MID, nat.ptr(bufs["idx"]), None, None, None, None, None, None,
                                    None) == nat.FS2_ERR_ARG
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError):
            f.subsample(8, offset=bad)
    f.close()
    with pytest.raises(nat.FS2Error) as ei:                               # a closed Python handle
        f.subsample(8)
    assert ei.value.code == nat.FS2_ERR_ARG


@pytest.mark.parametrize("kind", ["negative", "inf", "nan", "zeros"])
def test_invalid_weights_are_a_state_error_and_write_nothing(kind):
    from fast_slam_2 import _native as nat
    n = 4099
    w = weights(n, 1)
    if kind == "zeros":
        w[:] = 0.0
    else:
        w[{"negative": 2500, "inf": 0, "nan": 4098}[kind]] = {"negative": -1e-9, "inf": float("inf"),
                                                              "nan": float("nan")}[kind]
    f = make(n)
    f.set_state(*cloud(n, seed=1), w)
    rc, bufs, e, total = raw_call(f, 300, MID, 1, ("idx", "x", "y", "yaw", "w", "cnt"))
    assert rc == nat.FS2_ERR_STATE and nat.last_error(f._h) and untouched(bufs, e, total)
    rc, bufs, e, total = raw_call(f, 300, MID, 0, ("idx", "w"))           # not weighted: fine
    assert rc == 0 and total == n and e == 0
    f.close()


def test_pending_scan_and_sharded_handle_are_refused():
    import fast_slam_2
    import fs2_synthetic as syn
    from fast_slam_2 import _native as nat
    N, L = 4099, 12
    every = ("idx", "x", "y", "yaw", "w", "cnt")
    f = make(N, landmark_capacity=L + 16)
    populate(f, N, L)
    f.step_submit(*syn.odometry(0), np.ascontiguousarray(syn.scan_measurements(L, 0, 0)))
    for weighted in (1, 0):
        rc, bufs, e, total = raw_call(f, 64, MID, weighted, every)
        assert rc == nat.FS2_ERR_STATE and untouched(bufs, e, total)
    with pytest.raises(nat.FS2Error) as ei:
        f.subsample(64)
    assert ei.value.code == nat.FS2_ERR_STATE
    f.step_wait()
    assert f.subsample(64).idx.shape == (64,)
    f.close()
    key = os.urandom(128)
    shards = [fast_slam_2.FastSLAM2(512, seed=5, rank=g, world_size=2, comm_id=key, comm_mode="local", verbose=False)
              for g in range(2)]
    for h in shards:
        for weighted in (1, 0):
            rc, bufs, e, total = raw_call(h, 64, MID, weighted, every)
            assert rc == nat.FS2_ERR_STATE and untouched(bufs, e, total)
    for h in shards:
        h.close()


# ----------------------------------------------------------- non-interference ---

def test_subsampling_does_not_change_the_filter():
    import fast_slam_2
    import snapshot_decode as sd
    N, L, scans = 4099, 12, 6
    a, b = (make(N, seed=11, landmark_capacity=L + 4 * scans + 8) for _ in range(2))
    populate(a, N, L)
    populate(b, N, L)

    def readout(s, st):
        before = a.snapshot()
        a.subsample(257)
        a.subsample(3 * N + 7, 5, weighted=False)
        a.subsample(N, 2 ** 32 - 1)
        assert np.array_equal(a.snapshot(), before), s         # pools, page table and boxes as they were

    ra, res_a = run_scans(a, N, L, scans, readout)
    rb, res_b = run_scans(b, N, L, scans, None)
    assert res_a == res_b and len(res_a) >= 1                  # at least one resample
    for u, v in zip(ra, rb):
        assert np.array_equal(u[0], v[0]) and u[1] == v[1] and np.array_equal(u[2], v[2])
    for u, v in zip(a.get_state(), b.get_state()):
        assert u.shape == v.shape and np.array_equal(u, v)
    # The twins' final snapshots hold the same filter.  Their bytes are compared decoded:
    # two handles never promised equal bytes (a mirror past a map's end keeps whatever
    # record its never-written bits name, tests/test_gpu_snapshot_select.py), the same
    # handle does, which `readout` asserts around every group of draws.
    sa, sb = a.snapshot(), b.snapshot()
    ia, ib = (fast_slam_2.FastSLAM2.snapshot_info(s) for s in (sa, sb))
    for key in ("num_particles", "rows", "max_count", "scan"):
        assert ia[key] == ib[key], key
    for u, v in zip(sd.decode(sa), sd.decode(sb)):
        assert u.shape == v.shape and np.array_equal(u, v)
    a.close()
    b.close()


def test_subsample_writes_past_no_buffer():
    n = 70001
    f = make(n, guard=True)
    f.set_state(*cloud(n, seed=6), weights(n, 6))
    am = Amounts(weights(n, 6))
    for k in (3 * n + 7, 1):                                   # the scratch shrinks in use, not in size
        check_draw(f.subsample(k, 31), am, k, 31, f"guard k={k}")
        check_guards(f)
        assert f.subsample(k, 31, weighted=False).total == n
        check_guards(f)
    f.close()


def test_thinned_filter_from_the_drawn_indices():
    import fs2_synthetic as syn
    N, L, k = 4099, 12, 257
    cap = L + 40
    f = make(N, seed=11, landmark_capacity=cap)
    populate(f, N, L)
    _, resampled = run_scans(f, N, L, 6, None)
    assert resampled
    sub = f.subsample(k)
    g = make(k, seed=11, landmark_capacity=cap)
    g.restore(f.snapshot(select=sub.idx))
    sf = f.get_state()
    sg = g.get_state(lm_cap=sf[5].shape[1])
    for name, u, v in zip(("x", "y", "yaw", "w", "cnt"), sf, sg):
        assert np.array_equal(u[sub.idx], v), name
    assert np.array_equal(sg[0], sub.x) and np.array_equal(sg[4], sub.counts)
    live = np.arange(sf[5].shape[1])[None, :] < sg[4][:, None]
    assert np.array_equal(sf[5][sub.idx][live], sg[5][live])
    g.step(*syn.odometry(6), np.ascontiguousarray(syn.scan_measurements(L, 6, 0)))
    g.close()
    f.close()
