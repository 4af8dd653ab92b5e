"""Inputs shared by the float-repr tests (test_repr_host.py, test_gpu_json.py): the
curated values and the exhaustive boundaries of float.__repr__'s layouts and of the
rounding interval, plus the helpers that call fs2_repr_doubles and spell the expected
text.  The yardstick is CPython's own float.__repr__ as json.dumps writes it."""
import ctypes as C
import json

import numpy as np


def with_neighbours(vals):
    """Each value with its two nextafter neighbours where it is finite."""
    v = np.asarray(vals, dtype=np.float64)
    fin = v[np.isfinite(v)]
    with np.errstate(over="ignore"):        # (the largest finite value's neighbour is inf)
        return np.concatenate([v, np.nextafter(fin, np.inf), np.nextafter(fin, -np.inf)])


def nans():
    """NaNs of both signs and three payloads (quiet, signalling, all ones)."""
    bits = []
    for sign in (0, 1 << 63):
        for payload in (1 << 51, 1, (1 << 52) - 1):
            bits.append(sign | (0x7ff << 52) | payload)
    return np.array(bits, dtype=np.uint64).view(np.float64)


def curated():
    tiny = 5e-324
    vals = [0.0, -0.0, 1.0, 0.1, 0.30000000000000004, 1 / 3,
            1e-4, 1e-5, 0.0001234,
            1e15, 1e16, 9999999999999998.0, 123456789012345.6,
            1e22, 1e23, float(2 ** 53 + 1),
            tiny, 2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e308,
            np.inf, -np.inf]
    v = with_neighbours(vals)
    return np.concatenate([v, -v[np.isfinite(v)], nans()])


def boundaries():
    """Every power of two (where the rounding interval is asymmetric) and every finite
    power of ten (where the layouts and the digit counts change), with both neighbours."""
    p2 = np.array([np.ldexp(1.0, k) for k in range(-1074, 1024)])
    p10 = np.array([float(f"1e{k}") for k in range(-323, 309)])
    return with_neighbours(np.concatenate([p2, p10]))


def random_patterns(n, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64)


def pose_like(n, seed):
    rng = np.random.default_rng(seed)
    k = n // 3
    return np.concatenate([rng.normal(0, 3, k), rng.normal(0, 1e-3, k), rng.uniform(-np.pi, np.pi, n - 2 * k)])


def native_repr(v, on_host, device=0):
    """fs2_repr_doubles over v: the [n][24] text and the lengths."""
    from fast_slam_2 import _native as nat
    v = np.ascontiguousarray(v, dtype=np.float64)
    out = np.zeros((len(v), 24), dtype=np.uint8)
    ln = np.zeros(len(v), dtype=np.uint8)
    rc = nat.load().fs2_repr_doubles(device, nat.ptr(v), len(v), nat.ptr(out), nat.ptr(ln), 1 if on_host else 0)
    assert rc == nat.FS2_OK, nat.last_error()
    return out, ln


def assert_matches_cpython(v, out, ln):
    """Every text equals json.dumps(float) (float.__repr__, NaN / Infinity spellings)."""
    assert int(ln.max()) <= 24 and int(ln.min()) >= 3
    # one join and one bytes comparison instead of a Python loop over the mismatches
    want = [json.dumps(a).encode() for a in v.tolist()]
    wlen = np.fromiter(map(len, want), dtype=np.int64, count=len(want))
    bad = np.nonzero(wlen != ln)[0]
    assert bad.size == 0, [(v[i].hex(), want[i], bytes(out[i, :ln[i]])) for i in bad[:5]]
    mask = np.arange(24)[None, :] < ln[:, None]
    got = out[mask].tobytes()
    if got != b"".join(want):
        for i, w in enumerate(want):
            g = bytes(out[i, :ln[i]])
            assert g == w, (float(v[i]).hex(), w, g)
