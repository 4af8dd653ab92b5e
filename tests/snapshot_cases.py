"""A snapshot assembled by hand from the documented layout (csrc/fs2_snapshot.hpp,
DESIGN.md §13), shared by tests/test_snapshot_host.py and tests/test_gpu_snapshot.py.

N = 3 particles with cnt = [0, 9, 9]: particles 1 and 2 share their full first page
(un-owned), each has a private (owned) second page with one live mirror, and both of
those mirrors name the same record -- 3 pages, 2 rows, 9 records.  The dead mirrors of
the second pages carry garbage record ids."""
import numpy as np

HDR = np.dtype([("magic", "S8"), ("version", "<u4"), ("header_bytes", "<u4"), ("total", "<i8"),
                ("page_slots", "<u4"), ("page_bytes", "<u4"), ("rec_bytes", "<u4"), ("cnt_upper", "<i4"),
                ("n", "<i8"), ("rows", "<i8"), ("pages", "<i8"), ("records", "<i8"), ("scan", "<u8"),
                ("org", "<f4"), ("cell", "<f4"), ("ext_seen", "<f4"), ("slb", "<f4"),
                ("sec", "<i8", (4, 2)), ("pad", "u1", (96,))])
assert HDR.itemsize == 256
OWNED = 0x80000000
NONE = 0xFFFFFFFF
SCALARS, ROWS, PAGES, RECORDS = range(4)


def layout(N, R, U, C):
    """The section table [4][2] (offset, bytes) and the total byte count."""
    sec = np.zeros((4, 2), dtype=np.int64)
    at = 256
    for k, b in enumerate((36 * N, 4 * R * N, 128 * U, 48 * C)):
        sec[k] = (at, b)
        at = (at + b + 63) // 64 * 64
    return sec, at


def assemble(x, y, yaw, w, cnt, rows, pages, records, scan=0, cnt_upper=None, org=-127.0, cell=1.0,
             ext_seen=0.0, slb=0.0):
    """rows uint32 [R][N], pages uint32 [U][8][4] (mirror words x, y, s|slot, record),
    records float64 [C][6] -> the snapshot as a uint8 array."""
    N, R, U, C = len(cnt), rows.shape[0], pages.shape[0], records.shape[0]
    sec, total = layout(N, R, U, C)
    buf = np.zeros(total, dtype=np.uint8)
    h = np.zeros(1, dtype=HDR)
    h["magic"] = b"FS2SNAP"
    h["version"], h["header_bytes"], h["total"] = 1, 256, total
    h["page_slots"], h["page_bytes"], h["rec_bytes"] = 8, 128, 48
    h["cnt_upper"] = int(max(cnt)) if cnt_upper is None else cnt_upper
    h["n"], h["rows"], h["pages"], h["records"], h["scan"] = N, R, U, C, scan
    h["org"], h["cell"], h["ext_seen"], h["slb"] = org, cell, ext_seen, slb
    h["sec"] = sec
    buf[:256] = h.view(np.uint8)
    sc = np.concatenate([np.asarray(a, dtype="<f8").view(np.uint8) for a in (x, y, yaw, w)]
                        + [np.asarray(cnt, dtype="<i4").view(np.uint8)])
    for k, part in ((SCALARS, sc), (ROWS, rows.astype("<u4").reshape(-1).view(np.uint8)),
                    (PAGES, pages.astype("<u4").reshape(-1).view(np.uint8)),
                    (RECORDS, records.astype("<f8").reshape(-1).view(np.uint8))):
        assert part.size == sec[k, 1]
        buf[sec[k, 0]:sec[k, 0] + sec[k, 1]] = part
    return buf


def mirror(rec, slot, record_id):
    """The 4 words of a gate mirror: fp32 x, y, s = 0 (an unbounded slot: never
    rejected by the filter) with the slot index in its low 12 bits, the record id."""
    xy = np.asarray(rec[:2], dtype=np.float32).view(np.uint32)
    return [int(xy[0]), int(xy[1]), int(slot) & 0xFFF, int(record_id)]


def hand_built():
    """(snapshot bytes, the state it encodes as (x, y, yaw, w, cnt, lm[3][9][6]))."""
    rng = np.random.default_rng(12)
    records = np.zeros((9, 6))
    records[:, 0:2] = rng.uniform(-10, 10, (9, 2))
    records[:, 2] = records[:, 5] = 0.1
    records[:, 3] = records[:, 4] = 0.01
    pages = np.zeros((3, 8, 4), dtype=np.uint32)
    # page 0: slots in a shuffled order (a page may hold its slots in any order)
    order = [3, 0, 7, 1, 2, 6, 5, 4]
    for p, slot in enumerate(order):
        pages[0, p] = mirror(records[slot], slot, slot)
    for u in (1, 2):
        pages[u, 0] = mirror(records[8], 8, 8)
        for p in range(1, 8):
            pages[u, p] = [0, 0, 0, 0x12345678 + p]           # dead mirrors: garbage record ids
    rows = np.array([[NONE, 0, 0], [NONE, 1 | OWNED, 2 | OWNED]], dtype=np.uint32)
    x = np.array([0.5, 1.25, -2.0])
    y = np.array([0.0, -1.5, 3.0])
    yaw = np.array([0.1, 0.2, -0.3])
    w = np.array([0.25, 0.5, 0.25])
    cnt = np.array([0, 9, 9], dtype=np.int32)
    buf = assemble(x, y, yaw, w, cnt, rows, pages, records, scan=5, ext_seen=10.0)
    lm = np.zeros((3, 9, 6))
    lm[1] = lm[2] = records
    return buf, (x, y, yaw, w, cnt, lm)


def header(buf):
    """A writable structured view of the snapshot's header."""
    return buf[:256].view(HDR)


def section(buf, k, dtype):
    off, n = (int(v) for v in header(buf)["sec"][0][k])
    return buf[off:off + n].view(dtype)
