"""Compact snapshots on the host (no GPU): fs2_snapshot_check accepts a snapshot
assembled by hand from the documented layout and refuses each violated rule; the new
entry points are exported with ctypes signatures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import snapshot_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    import build
    build.build()
    from fast_slam_2 import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def good():
    buf, state = sc.hand_built()
    buf.setflags(write=False)
    return buf


def check(nat, buf, size=None):
    info = nat.fs2_snapshot_info()
    a = np.ascontiguousarray(buf)
    rc = nat.load().fs2_snapshot_check(a.ctypes.data, a.size if size is None else size, C.byref(info))
    return rc, info


def test_hand_built_snapshot_is_accepted(nat, good):
    rc, info = check(nat, good)
    assert rc == nat.FS2_OK, nat.last_error()
    assert (info.pages, info.rows, info.records) == (3, 2, 9)
    assert (info.num_particles, info.max_count, info.scan, info.version) == (3, 9, 5, 1)
    assert info.bytes == good.size
    # the Python wrapper, from any buffer object
    import fast_slam_2
    d = fast_slam_2.FastSLAM2.snapshot_info(bytes(good))
    assert d["pages"] == 3 and d["records"] == 9 and d["rows"] == 2 and d["bytes"] == good.size


def _magic(b):
    sc.header(b)["magic"] = b"FS2SNAQ"


def _version(b):
    sc.header(b)["version"] = 2


def _offset(b):
    sc.header(b)["sec"][0][sc.RECORDS][0] = b.size + 64


def _cnt(b):
    sc.section(b, sc.SCALARS, np.uint8)[32 * 3:].view("<i4")[1] = 17       # 8 R = 16


def _entry(b):
    sc.section(b, sc.ROWS, "<u4")[1] = 3                                    # == U


def _record(b):
    sc.section(b, sc.PAGES, "<u4").reshape(3, 8, 4)[0, 2, 3] = 9            # == C, a live mirror


def _slot(b):
    sc.section(b, sc.PAGES, "<u4").reshape(3, 8, 4)[1, 0, 2] = 9            # == cnt, a live mirror


def _owned_twice(b):
    sc.section(b, sc.ROWS, "<u4").reshape(2, 3)[1, 2] = 1 | sc.OWNED        # page 1: two owners


def _owned_and_shared(b):
    sc.section(b, sc.ROWS, "<u4").reshape(2, 3)[1, 2] = 1                   # page 1: an owner and a sharer


def _missing(b):
    sc.section(b, sc.ROWS, "<u4").reshape(2, 3)[0, 2] = sc.NONE


RULES = [_magic, _version, _offset, _cnt, _entry, _record, _slot, _owned_twice, _owned_and_shared, _missing]


@pytest.mark.parametrize("violate", RULES, ids=lambda f: f.__name__.lstrip("_"))
def test_each_rule_is_enforced(nat, good, violate):
    b = good.copy()
    violate(b)
    rc, _ = check(nat, b)
    assert rc == nat.FS2_ERR_ARG
    assert "invalid snapshot" in nat.last_error()


@pytest.mark.parametrize("delta", [-1, 1])
def test_size_must_equal_the_total(nat, good, delta):
    b = np.concatenate([good, np.zeros(1, dtype=np.uint8)])       # (one spare byte to read)
    rc, _ = check(nat, b, size=good.size + delta)
    assert rc == nat.FS2_ERR_ARG


def test_dead_mirror_garbage_is_accepted(nat, good):
    b = good.copy()
    pages = sc.section(b, sc.PAGES, "<u4").reshape(3, 8, 4)
    pages[1, 1:, 3] = 0xFFFFFFF0                                            # record ids past C
    pages[2, 5, 2] = 0xFFF                                                  # a slot index past cnt
    rc, info = check(nat, b)
    assert rc == nat.FS2_OK, nat.last_error()
    assert info.records == 9


def test_unaligned_buffer(nat, good):
    """The buffer may start anywhere (a slice of a file image)."""
    raw = np.zeros(good.size + 1, dtype=np.uint8)
    raw[1:] = good
    rc, info = check(nat, raw[1:])
    assert rc == nat.FS2_OK and info.pages == 3


def test_abi_exports_and_signatures(nat):
    src = open(os.path.join(REPO, "include", "fs2.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = ["fs2_snapshot_save", "fs2_snapshot_load", "fs2_snapshot_check"]
    sigs = {n: (r, a) for n, r, a in nat.SIGNATURES}
    lib = nat.load()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(lib, n) and n in sigs
        assert getattr(lib, n).argtypes == sigs[n][1]
    assert re.search(r"#define FS2_ABI_VERSION 2\b", src)
    body = re.search(r"typedef struct fs2_snapshot_info \{(.*?)\} fs2_snapshot_info;", src, re.S).group(1)
    fields = [nm.strip() for decl in body.split(";") if decl.strip() for nm in decl.split(None, 1)[1].split(",")]
    assert [f for f, _ in nat.fs2_snapshot_info._fields_] == fields
    assert C.sizeof(nat.fs2_snapshot_info) == 64
