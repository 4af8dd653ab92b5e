"""Selective snapshots on the host (no GPU): fs2_snapshot_save_select is declared,
exported and bound with matching ctypes arguments and refuses a null handle; and the
numpy decoder the GPU tests read selections with (tests/snapshot_decode.py) gives the
state the hand-built snapshot of snapshot_cases is stated to encode."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import snapshot_cases as sc
import snapshot_decode as sd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    import build
    build.build()
    from fast_slam_2 import _native
    _native.load()
    return _native


def test_entry_point_is_declared_exported_and_bound(nat):
    src = open(os.path.join(REPO, "include", "fs2.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"int\s+fs2_snapshot_save_select\s*\(([^)]*)\)\s*;", src)
    assert decl, "fs2_snapshot_save_select is not declared in include/fs2.h"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["fs2_handle *h", "const int64_t *idx", "int64_t m", "void *buf", "int64_t capacity",
                    "int64_t *size"]
    sigs = {n: (r, a) for n, r, a in nat.SIGNATURES}
    assert "fs2_snapshot_save_select" in sigs
    res, argtypes = sigs["fs2_snapshot_save_select"]
    assert res is C.c_int
    assert argtypes == [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    fn = getattr(nat.load(), "fs2_snapshot_save_select")
    assert fn.argtypes == argtypes and fn.restype is res
    assert re.search(r"#define FS2_ABI_VERSION 2\b", src)          # an added function: no bump


def test_null_handle_is_refused(nat):
    idx = np.zeros(1, dtype=np.int64)
    size = C.c_int64(-7)
    out = np.full(64, 0xAB, dtype=np.uint8)
    rc = nat.load().fs2_snapshot_save_select(None, idx.ctypes.data, 1, out.ctypes.data, out.size, C.byref(size))
    assert rc == nat.FS2_ERR_ARG
    assert size.value == -7 and np.all(out == 0xAB)
    assert "null handle" in nat.last_error()


def test_decoder_reads_the_hand_built_snapshot():
    buf, want = sc.hand_built()
    got = sd.decode(buf)
    assert len(got) == len(want) == 6
    for u, v in zip(got, want):
        assert u.shape == np.asarray(v).shape and u.dtype == np.asarray(v).dtype and np.array_equal(u, v)
    # the sections as the layout gives them
    h, x, y, yaw, w, cnt, rows, pages, records = sd.sections(buf)
    assert rows.shape == (2, 3) and pages.shape == (3, 8, 4) and records.shape == (9, 6)
    assert int(h["scan"]) == 5 and int(h["cnt_upper"]) == 9


def test_decoder_places_slots_by_the_mirror_index():
    """Page 0 of the hand-built snapshot holds its slots in a shuffled order: a decoder
    that placed records by mirror position would put record 3 into slot 0."""
    buf, want = sc.hand_built()
    _, _, _, _, _, _, rows, pages, records = sd.sections(buf)
    assert int(pages[0, 0, 2] & 0xFFF) == 3                         # position 0 holds slot 3
    lm = sd.decode(buf)[5]
    assert np.array_equal(lm[1, 3], records[3]) and not np.array_equal(lm[1, 0], records[3])
    assert np.array_equal(lm[0], np.zeros((9, 6)))                  # the empty map
