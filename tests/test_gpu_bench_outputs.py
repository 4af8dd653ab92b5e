"""bench.py --dump-outputs and the plain run's result line.

A plain `bench.py --steps K --warmup W` times K scans and prints the headline
alone (no CPU baseline, no robustness runs, no other configs: those are
`--full`'s); `--dump-outputs DIR` writes what the last timed scan left a caller
(pose estimate, particle state) as float64 DIR/<name>.npy, the same from run to
run with the same arguments, and as a seeded sample when the state is larger
than the dump's bound.  N = 5000 runs the exact reduction of the headline
(above 4096 particles).  The first run is made once and shared.
"""
import contextlib
import io
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, L, STEPS, WARMUP = 5000, 40, 6, 2
NAMES = {"pose", "particle_index", "x", "y", "yaw", "w", "cnt", "map_index", "lm"}


def _run(out_dir, *more):
    import torch  # noqa: F401  -- one HIP runtime in the process
    import bench
    from gpu_util import configure
    configure()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        bench.main(["--gpus", "1", "--particles", str(N), "--landmarks", str(L), "--steps", str(STEPS),
                    "--warmup", str(WARMUP), "--dump-outputs", str(out_dir), *more])
    lines = [l for l in out.getvalue().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    arrays = {os.path.splitext(p)[0]: np.load(os.path.join(out_dir, p)) for p in os.listdir(out_dir)}
    return d, arrays


@pytest.fixture(scope="module")
def first_run(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("dump") / "a")


@pytest.fixture(scope="module")
def first(first_run):
    return first_run[1]


def test_plain_run_dumps_the_last_step(first_run):
    d, a = first_run
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["metric"] == "particle-updates/s"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(N / (d["ms_per_step"] * 1e-3))
    # the headline alone: what takes runs of its own is --full's
    assert d["cpu_baseline"] is None
    assert "robustness" not in d["extra"] and "configs" not in d["extra"]
    assert set(a) == NAMES
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["pose"].shape == (3,) and np.isfinite(a["pose"]).all()
    assert np.array_equal(a["particle_index"], np.arange(N))
    for k in ("x", "y", "yaw", "w", "cnt"):
        assert a[k].shape == (N,) and np.isfinite(a[k]).all()
    # every scan appends at least its miss, within the handle's landmark capacity
    assert a["cnt"].min() >= L + 1 and a["cnt"].max() <= L + STEPS + WARMUP + 8
    assert (a["w"] >= 0).all() and a["w"].sum() > 0
    k = len(a["map_index"])
    assert k >= 1 and a["lm"].shape == (k, int(a["cnt"].max()), 6)
    for j, p in enumerate(a["map_index"].astype(int)):
        c = int(a["cnt"][p])
        assert np.abs(a["lm"][j, :c, :2]).max() > 0 and not a["lm"][j, c:].any()


def test_same_arguments_same_outputs(tmp_path, first):
    _, b = _run(tmp_path / "b")
    for k in NAMES:
        assert np.array_equal(first[k], b[k]), k


def test_larger_state_is_sampled(tmp_path, first, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_PARTICLES", 1000)
    monkeypatch.setattr(bench, "DUMP_MAPS", 16)
    _, s = _run(tmp_path / "s")
    idx = s["particle_index"].astype(int)
    assert len(idx) == 1000 and len(np.unique(idx)) == 1000 and np.array_equal(idx, np.sort(idx))
    assert np.array_equal(s["pose"], first["pose"])
    for k in ("x", "y", "yaw", "w", "cnt"):
        assert np.array_equal(s[k], first[k][idx]), k
    midx = s["map_index"].astype(int)
    assert len(midx) == 16 and np.isin(midx, idx).all()
    # the sampled maps are the particles' own: their lengths and, where the first
    # run kept the same particle, its records
    for j, p in enumerate(midx):
        c = int(first["cnt"][p])
        assert not s["lm"][j, c:].any() and np.abs(s["lm"][j, c - 1, :2]).max() > 0
        hit = np.flatnonzero(first["map_index"].astype(int) == p)
        if len(hit):
            assert np.array_equal(s["lm"][j, :c], first["lm"][hit[0], :c])


def test_more_steps_than_a_handle_takes_run_as_windows(tmp_path, first, monkeypatch):
    """7 timed steps with 3 to a window: three handles in turn (3 + 3 + 1 scans, each
    after its own warm-up), one result line for all 7, and the last window's state
    dumped -- the state a run of WARMUP + 1 scans leaves."""
    import bench
    monkeypatch.setattr(bench, "WINDOW_MAX", 3)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        bench.main(["--gpus", "1", "--particles", str(N), "--landmarks", str(L), "--steps", "7",
                    "--warmup", str(WARMUP), "--dump-outputs", str(tmp_path / "w")])
    d = json.loads([l for l in out.getvalue().splitlines() if l.startswith("{")][0])
    assert d["steps"] == 7 and d["extra"]["windows"] == [3, 3, 1]
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(N / (d["ms_per_step"] * 1e-3))
    assert d["extra"]["slots_visited_per_particle_scan"] > 0
    monkeypatch.setattr(bench, "WINDOW_MAX", 500)
    with contextlib.redirect_stdout(io.StringIO()):
        bench.main(["--gpus", "1", "--particles", str(N), "--landmarks", str(L), "--steps", "1",
                    "--warmup", str(WARMUP), "--dump-outputs", str(tmp_path / "one")])
    for k in NAMES:
        assert np.array_equal(np.load(tmp_path / "w" / f"{k}.npy"), np.load(tmp_path / "one" / f"{k}.npy")), k
