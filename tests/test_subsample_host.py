"""fs2_subsample_threshold on the host (fs2.h): the 64-bit decomposition of

    t_j = floor((j Q + floor(offset Q / 2^32)) / k)

that the subsample kernel also runs (csrc/fs2_subsample.hpp sub_threshold), against the
same expression in Python's unbounded integers, over the extremes of Q, k, offset and j."""
import ctypes as C
import os
import re

import pytest

from conftest import REPO

QS = [1, 2, 3, 2 ** 20 + 1, 2 ** 52 * 1000, 2 ** 62 - 1, 2 ** 62]
KS = [1, 2, 3, 64, 4099, 2 ** 30 - 1, 2 ** 30]
OFFSETS = [0, 1, 2 ** 31, 2 ** 32 - 1]
SENTINEL = 0xDEADBEEFCAFEF00D


def lib():
    from fast_slam_2 import _native as nat
    return nat.load()


def threshold(Q, k, offset, j):
    t = C.c_uint64(SENTINEL)
    rc = lib().fs2_subsample_threshold(Q, k, offset, j, C.byref(t))
    return rc, t.value


def want(Q, k, offset, j):
    return (j * Q + ((offset * Q) >> 32)) // k


def js(k):
    return sorted(j for j in {0, 1, k // 2, k - 1} if 0 <= j < k)


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("k", KS)
def test_threshold_matches_python_integers(Q, k):
    assert 2 ** 52 * 1000 < 2 ** 62
    for offset in OFFSETS:
        prev = -1
        for j in js(k):
            rc, t = threshold(Q, k, offset, j)
            assert rc == 0 and t == want(Q, k, offset, j), (Q, k, offset, j, t)
            assert prev <= t < Q, (Q, k, offset, j, t)          # non-decreasing in j, below Q
            prev = t
        assert threshold(Q, k, offset, k - 1)[1] < Q


def test_thresholds_of_a_whole_small_draw_are_non_decreasing():
    for Q, k, offset in [(3, 64, 2 ** 32 - 1), (2 ** 62, 4099, 2 ** 31), (2 ** 20 + 1, 4099, 1), (1, 3, 2 ** 32 - 1)]:
        ts = [threshold(Q, k, offset, j) for j in range(k)]
        assert all(rc == 0 for rc, _ in ts)
        ts = [t for _, t in ts]
        assert ts == [want(Q, k, offset, j) for j in range(k)]
        assert all(a <= b for a, b in zip(ts, ts[1:])) and ts[-1] < Q


@pytest.mark.parametrize("Q,k,j", [(0, 4, 0), (2 ** 62 + 1, 4, 0), (2 ** 64 - 1, 4, 0), (5, 0, 0), (5, -1, 0),
                                   (5, 2 ** 30 + 1, 0), (5, 4, -1), (5, 4, 4), (5, 1, 1)])
def test_threshold_rejects_bad_arguments(Q, k, j):
    from fast_slam_2 import _native as nat
    rc, t = threshold(Q, k, 2 ** 31, j)
    assert rc == nat.FS2_ERR_ARG and t == SENTINEL              # nothing written
    assert "fs2_subsample_threshold" in nat.last_error()


def test_threshold_rejects_a_null_result():
    from fast_slam_2 import _native as nat
    assert lib().fs2_subsample_threshold(5, 4, 0, 0, None) == nat.FS2_ERR_ARG


def test_abi_version_is_still_2_and_the_prototypes_are_declared():
    assert lib().fs2_abi_version() == 2
    src = open(os.path.join(REPO, "include", "fs2.h")).read()
    assert re.search(r"#define\s+FS2_ABI_VERSION\s+2\b", src)
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    for proto in (
            "int fs2_subsample(fs2_handle *h, int32_t weighted, int64_t k, uint32_t offset, int64_t *idx, "
            "double *x, double *y, double *yaw, double *w, int32_t *cnt, int32_t *scale_exp, uint64_t *total);",
            "int fs2_subsample_threshold(uint64_t total, int64_t k, uint32_t offset, int64_t j, uint64_t *t);",
            "int fs2_debug_subsample_times(int32_t enable, double ms[3]);"):
        assert proto in code, proto
