"""The viewer JSON's particle block written on the device (csrc/fs2_json.hip): digits
equal to CPython's float.__repr__, the list's text equal to json.dumps(..., indent=4)
byte for byte at every size around a workgroup's 256 particles, the size protocol of
fs2_poses_json, and the handle path (fs2_particles_json, FastSLAM2.poses_json,
Serializer) after set_state, after real resampling scans, while a scan is
outstanding and under FS2_GUARD."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import repr_cases as rc
from golden_io import load_seq

pytestmark = pytest.mark.gpu

WG = 256                                    # kJsonBlock: particles per workgroup
LONGEST, SHORTEST = -2.2250738585072014e-308, 0.0      # 24 and 3 bytes


@pytest.fixture(scope="module")
def fs():
    import torch  # noqa: F401  (loads the HIP runtime first)
    import fast_slam_2
    from gpu_util import configure
    configure()
    yield fast_slam_2
    configure()


def expected_block(x, y, yaw, depth):
    """The list's text as json.dumps(..., indent=4) writes it `depth` levels deep:
    embedded in a document (as tests/test_serializer.py obtains it) and cut out."""
    doc = [{"x": float(a), "y": float(b), "yaw": float(c)} for a, b, c in zip(x, y, yaw)]
    for _ in range(depth):
        doc = {"p": doc}
    s = json.dumps(doc, indent=4)
    if depth == 0:
        return s.encode()
    start = s.index('"p": ', s.rindex("{\n" + " " * (4 * depth) + '"p": ')) + 5
    closing = sum(2 + 4 * k for k in range(depth))      # "\n" indent "}" per enclosing level
    return s[start:len(s) - closing].encode()


def poses_json(x, y, yaw, depth, where=0, device_ptrs=None):
    from fast_slam_2 import _native as nat
    lib = nat.load()
    n = len(x)
    px, py, pw = device_ptrs if device_ptrs else (nat.ptr(np.ascontiguousarray(a, dtype=np.float64)) for a in (x, y, yaw))
    size = C.c_int64(-1)
    assert lib.fs2_poses_json(0, px, py, pw, n, depth, None, 0, C.byref(size), where) == nat.FS2_OK, nat.last_error()
    buf = np.full(size.value + 64, 0xC3, dtype=np.uint8)
    size2 = C.c_int64(-1)
    rc_ = lib.fs2_poses_json(0, px, py, pw, n, depth, nat.ptr(buf), size.value, C.byref(size2), where)
    assert rc_ == nat.FS2_OK, nat.last_error()
    assert size2.value == size.value
    assert np.all(buf[size.value:] == 0xC3), "bytes past an exact-capacity buffer were written"
    return buf[:size.value].tobytes()


def mixed_values(n, seed):
    """x, y, yaw mixing 3-byte and 24-byte numbers with ordinary ones and the special
    spellings; for n > 2 WG, a run of all-longest and a run of all-shortest items, each
    longer than one workgroup (the extremes of the LDS staging size)."""
    rng = np.random.default_rng(seed)
    pool = np.array([SHORTEST, LONGEST, 1.5, -0.0, 1e-5, 1e16, np.nan, np.inf, -np.inf, 5e-324, 123456789012345.6])
    pick = rng.integers(0, len(pool) + 6, (3, n))
    v = np.where(pick < len(pool), pool[np.minimum(pick, len(pool) - 1)], rng.normal(0, 3, (3, n)))
    # 3-byte and 24-byte numbers next to each other
    v[0, 0::2], v[1, 1::4], v[2, 2::4] = SHORTEST, LONGEST, SHORTEST
    v[0, 1::8] = LONGEST
    if n > 4 * WG + 20:                      # (each run covers one whole workgroup and more)
        v[:, WG - 20:2 * WG + 20] = LONGEST
        v[:, 3 * WG - 20:4 * WG + 20] = SHORTEST
    return v[0].copy(), v[1].copy(), v[2].copy()


def test_digits_on_the_device(fs):
    v = np.concatenate([rc.curated(), rc.boundaries(), rc.random_patterns(200_000, seed=77)])
    out, ln = rc.native_repr(v, on_host=False)
    rc.assert_matches_cpython(v, out, ln)


BIG = 15241                                 # 60 workgroups (59.5 x 256), prime: enough segment starts to
                                            # meet every residue mod 16 (asserted below from the lengths)


@pytest.mark.parametrize("depth", [0, 1, 2])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, WG - 1, WG, WG + 1, BIG])
def test_poses_json_matches_json_dumps(fs, n, depth):
    x, y, yaw = mixed_values(n, seed=1000 + n)
    want = expected_block(x, y, yaw, depth)
    if n == BIG:
        # every residue mod 16 occurs among the particles' and the workgroups' first bytes
        lens = np.array([len(json.dumps(float(a))) + len(json.dumps(float(b))) + len(json.dumps(float(c)))
                         for a, b, c in zip(x, y, yaw)]) + (27 + 8 * (depth + 1) + 12 * (depth + 2))
        off = np.concatenate([[0], np.cumsum(lens)[:-1]])
        assert int(off[-1] + lens[-1]) + 2 + 4 * depth == len(want)
        assert set(off % 16) == set(range(16)) and set(off[::WG] % 16) == set(range(16))
        # one workgroup holds only longest items, one only shortest (72 / 9 bytes of numbers)
        per = lens[: (n // WG) * WG].reshape(-1, WG).sum(axis=1)
        assert per.max() == WG * lens.max() and per.min() == WG * lens.min()
        assert lens.max() - lens.min() == 3 * 24 - 3 * 3
    got = poses_json(x, y, yaw, depth)
    assert got == want, (n, depth, len(got), len(want))


def test_poses_json_from_device_buffers(fs):
    import torch
    n = 3 * WG + 5
    x, y, yaw = mixed_values(n, seed=5)
    t = [torch.from_numpy(a).to("cuda") for a in (x, y, yaw)]
    torch.cuda.synchronize()
    got = poses_json(x, y, yaw, 1, where=1, device_ptrs=tuple(a.data_ptr() for a in t))
    assert got == expected_block(x, y, yaw, 1)


def test_size_protocol(fs):
    from fast_slam_2 import _native as nat
    lib = nat.load()
    n = WG + 9
    x, y, yaw = mixed_values(n, seed=6)
    want = expected_block(x, y, yaw, 1)
    size = C.c_int64(-1)
    args = [nat.ptr(a) for a in (x, y, yaw)]
    assert lib.fs2_poses_json(0, *args, n, 1, None, 0, C.byref(size), 0) == nat.FS2_OK
    assert size.value == len(want)
    buf = np.full(len(want) + 64, 0x5A, dtype=np.uint8)
    size = C.c_int64(-1)
    assert lib.fs2_poses_json(0, *args, n, 1, nat.ptr(buf), len(want) - 1, C.byref(size), 0) == nat.FS2_ERR_ARG
    assert size.value == len(want) and np.all(buf == 0x5A)
    assert lib.fs2_poses_json(0, *args, n, 1, nat.ptr(buf), len(want), C.byref(size), 0) == nat.FS2_OK
    assert buf[:len(want)].tobytes() == want and np.all(buf[len(want):] == 0x5A)
    # n = 0: "[]" under the same protocol
    size = C.c_int64(-1)
    assert lib.fs2_poses_json(0, None, None, None, 0, 1, None, 0, C.byref(size), 0) == nat.FS2_OK and size.value == 2
    assert lib.fs2_poses_json(0, None, None, None, 0, 1, nat.ptr(buf), 1, C.byref(size), 0) == nat.FS2_ERR_ARG
    assert lib.fs2_poses_json(0, *args, n, -1, None, 0, C.byref(size), 0) == nat.FS2_ERR_ARG
    assert lib.fs2_poses_json(0, *args, n, 1, None, 0, None, 0) == nat.FS2_ERR_ARG


def _document(est, act, x, y, yaw, lms, res):
    return json.dumps({"estimated_robot_pos": est.to_dict(), "actual_robot_pos": act.to_dict(),
                       "particles": [{"x": float(a), "y": float(b), "yaw": float(c)} for a, b, c in zip(x, y, yaw)],
                       "landmarks": [lm.to_dict() for lm in lms], "results": res.to_dict()}, indent=4)


def test_serializer_takes_the_device_path(fs, monkeypatch, tmp_path):
    from fast_slam_2 import DirectedPoint, EvaluationResults, Point, Serializer
    from fast_slam_2 import _native as nat
    from fast_slam_2.utils import serializer
    N = 3000
    rng = np.random.default_rng(8)
    f = fs.FastSLAM2(N, verbose=False)
    f.set_state(rng.normal(0, 3, N), rng.normal(0, 3, N), rng.uniform(-3, 3, N), np.full(N, 1.0 / N))
    est, act = DirectedPoint(0.5, 0.25, 0.1), DirectedPoint(0.0, 0.0, 0.0)
    lms = [Point(1.0, 2.0)]
    res = EvaluationResults("t", 0.0, 0.0, 0.0, 0.0, 0.0)
    x, y, yaw, *_ = f.get_state()
    want = _document(est, act, x, y, yaw, lms, res)

    def boom(*a, **k):
        raise AssertionError("the host emitter ran")
    monkeypatch.setattr(serializer, "_poses_block", boom)
    assert Serializer.to_json(est, act, f.particles, lms, res) == want
    monkeypatch.setattr(Serializer, "shared_path", str(tmp_path / "shared"))
    monkeypatch.setattr(Serializer, "file_path", str(tmp_path / "shared" / Serializer.file_name))
    Serializer.serialize(est, act, f.particles, lms, res)
    assert open(Serializer.file_path, "rb").read() == want.encode()
    assert f.poses_json(2) == expected_block(x, y, yaw, 2)
    # sub-ranges and out-of-range arguments
    lib = nat.load()
    for first, count in [(0, 1), (10, 100), (N - WG - 1, WG + 1), (N, 0), (17, 0)]:
        size = C.c_int64(-1)
        assert lib.fs2_particles_json(f._h, first, count, 1, None, 0, C.byref(size)) == nat.FS2_OK
        buf = np.zeros(size.value, dtype=np.uint8)
        assert lib.fs2_particles_json(f._h, first, count, 1, nat.ptr(buf), size.value, C.byref(size)) == nat.FS2_OK
        sl = slice(first, first + count)
        assert buf.tobytes() == expected_block(x[sl], y[sl], yaw[sl], 1), (first, count)
    size = C.c_int64(-1)
    for first, count in [(-1, 5), (0, N + 1), (N - 1, 2), (0, -1)]:
        assert lib.fs2_particles_json(f._h, first, count, 1, None, 0, C.byref(size)) == nat.FS2_ERR_ARG
    assert lib.fs2_particles_json(f._h, 0, N, 7, None, 0, C.byref(size)) == nat.FS2_ERR_ARG
    f.close()


def test_after_resampling_scans(fs):
    """After every scan of a sequence that resamples, poses_json equals the text built
    from get_state (a resample switches the buffer set the poses live in)."""
    from gpu_util import from_fixture
    d = load_seq("resample_n64")
    S = int(d["S"])
    assert np.any(~np.isnan(d["uniform"][:S])), "the fixture records no resampling scan"
    f = from_fixture(d)
    resampled = 0
    for s in range(S):
        M = int(d["M"][s])
        u0 = d["uniform"][s]
        _, st = f.step(d["rotation"][s], d["translation"][s], d["meas"][s, :M], d["observed"][s, :M],
                       d["normals"][s], 0.0 if np.isnan(u0) else u0)
        resampled += st.resampled
        x, y, yaw, *_ = f.get_state()
        assert f.poses_json() == expected_block(x, y, yaw, 1), s
    assert resampled >= 1
    f.close()


def test_refused_while_a_scan_is_outstanding(fs):
    from fast_slam_2 import _native as nat
    from gpu_util import from_fixture
    d = load_seq("cfg1_n100_l20")
    f = from_fixture(d)
    M = int(d["M"][0])
    f.step_submit(d["rotation"][0], d["translation"][0], d["meas"][0, :M], d["observed"][0, :M], d["normals"][0], 0.0)
    size = C.c_int64(-1)
    assert nat.load().fs2_particles_json(f._h, 0, f.n_local, 1, None, 0, C.byref(size)) == nat.FS2_ERR_STATE
    f.step_wait()
    x, y, yaw, *_ = f.get_state()
    assert f.poses_json() == expected_block(x, y, yaw, 1)
    f.close()


@pytest.mark.parametrize("N", [3000, 70_000])
def test_guards_stay_clean(fs, N):
    from fast_slam_2 import _native as nat
    old = os.environ.get("FS2_GUARD")
    os.environ["FS2_GUARD"] = "1"
    try:
        f = fs.FastSLAM2(N, verbose=False)
    finally:
        if old is None:
            os.environ.pop("FS2_GUARD", None)
        else:
            os.environ["FS2_GUARD"] = old
    rng = np.random.default_rng(N)
    x, y, yaw = rng.normal(0, 3, N), rng.normal(0, 1e-3, N), rng.uniform(-np.pi, np.pi, N)
    f.set_state(x, y, yaw, np.full(N, 1.0 / N))
    want = expected_block(x, y, yaw, 1)
    name = C.create_string_buffer(128)
    for _ in range(2):                      # the second call reuses the handle's buffers
        assert f.poses_json() == want
        bad = nat.load().fs2_debug_check_guards(f._h, name, 128)
        assert bad == 0, f"{bad} guard bytes overwritten after buffer {name.value.decode()}"
    assert f.poses_json(0) == expected_block(x, y, yaw, 0)     # another size: the buffers are replaced
    assert nat.load().fs2_debug_check_guards(f._h, name, 128) == 0, name.value.decode()
    f.close()
