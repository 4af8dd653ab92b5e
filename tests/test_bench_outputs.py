"""bench.py's --full / --dump-outputs options and dump_outputs' sampling (CPU test:
a stand-in for the filter handle serves get_state from host arrays)."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


class _Handle:
    """get_state of n particles with maps of cnt[i] landmarks; lm[i][j] = (i, j, ...)."""

    def __init__(self, n, cap):
        r = np.random.default_rng(5)
        self.n_local = n
        self.x, self.y, self.yaw, self.w = (r.normal(size=n) for _ in range(4))
        self.cnt = r.integers(1, cap + 1, n).astype(np.int32)

    def get_state(self, first=0, count=None, lm_cap=None):
        count = self.n_local - first if count is None else count
        s = slice(first, first + count)
        lm = np.zeros((count, max(lm_cap or 0, 1), 6))
        if lm_cap:
            for i in range(count):
                c = min(int(self.cnt[first + i]), lm_cap)
                lm[i, :c, 0] = first + i
                lm[i, :c, 1] = np.arange(c)
                lm[i, :c, 2:] = 1.0
        return self.x[s], self.y[s], self.yaw[s], self.w[s], self.cnt[s], lm


def _load(d):
    return {os.path.splitext(p)[0]: np.load(os.path.join(d, p)) for p in os.listdir(d)}


def test_options_default_off():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


def test_small_state_is_written_whole(tmp_path):
    import bench
    h = _Handle(300, 9)
    bench.dump_outputs(str(tmp_path / "o"), h, (1.0, 2.0, 3.0), 0)
    a = _load(tmp_path / "o")
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["pose"], [1.0, 2.0, 3.0])
    assert np.array_equal(a["particle_index"], np.arange(300))
    for k in ("x", "y", "yaw", "w", "cnt"):
        assert np.array_equal(a[k], getattr(h, k))
    m = a["map_index"].astype(int)
    assert len(m) == min(300, bench.DUMP_MAPS) and len(np.unique(m)) == len(m)
    assert a["lm"].shape == (len(m), int(h.cnt.max()), 6)
    for j, p in enumerate(m):
        c = int(h.cnt[p])
        assert (a["lm"][j, :c, 0] == p).all() and np.array_equal(a["lm"][j, :c, 1], np.arange(c))
        assert not a["lm"][j, c:].any()


def test_large_state_is_a_seeded_sample_within_the_bound(tmp_path):
    import bench
    n = bench.DUMP_PARTICLES + 40_000
    h = _Handle(n, 4000)                 # long maps: fewer than DUMP_MAPS fit DUMP_MAP_BYTES
    bench.dump_outputs(str(tmp_path / "a"), h, (0.0, 0.0, 0.0), 3)
    bench.dump_outputs(str(tmp_path / "b"), h, (0.0, 0.0, 0.0), 3)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["lm"].nbytes <= bench.DUMP_MAP_BYTES and 1 <= len(a["map_index"]) < bench.DUMP_MAPS
    idx = a["particle_index"].astype(int)
    assert len(idx) == bench.DUMP_PARTICLES == len(np.unique(idx)) and idx.max() < n
    assert np.isin(a["map_index"].astype(int), idx).all()
    assert np.array_equal(a["x"], h.x[idx]) and np.array_equal(a["cnt"], h.cnt[idx])
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    bench.dump_outputs(str(tmp_path / "c"), h, (0.0, 0.0, 0.0), 4)
    assert not np.array_equal(_load(tmp_path / "c")["particle_index"], a["particle_index"])


def test_any_step_count_fits_the_maps():
    import bench
    # a map of L landmarks takes at most 4 appends per scan: warm-up, a window's timed
    # scans and the 40 scans --full continues the last handle for stay within MAX_SLOTS
    for L, warmup in ((500, 3), (500, 0), (200, 5), (20, 3), (3000, 3)):
        win = bench.window_steps(L, warmup)
        assert 1 <= win <= bench.WINDOW_MAX
        assert L + 4 * (warmup + win + 40) + 8 <= bench.MAX_SLOTS
    assert bench.window_steps(500, 3) == bench.WINDOW_MAX      # the headline: 20 steps, one window
    assert bench.window_steps(4000, 3) < 1                     # no room: main() refuses
    assert bench.split_steps(20, 500) == [20]
    assert bench.split_steps(500, 500) == [500]
    assert bench.split_steps(1201, 500) == [500, 500, 201]
    assert sum(bench.split_steps(98765, 500)) == 98765
