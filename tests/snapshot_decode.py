"""A numpy reading of the documented snapshot layout (csrc/fs2_snapshot.hpp, DESIGN.md
§13), independent of libfs2: snapshot bytes -> the state they encode, in the shape
FastSLAM2.get_state() returns.  tests/test_snapshot_select_host.py pins it against the
hand-built snapshot of snapshot_cases; the GPU tests then read selections with it."""
import numpy as np

import snapshot_cases as sc


def sections(buf):
    """(header, x, y, yaw, w, cnt, rows [R][N], pages [U][8][4] uint32, records [C][6])."""
    buf = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8))
    h = sc.header(buf)[0]
    N, R, U, C = (int(h[k]) for k in ("n", "rows", "pages", "records"))
    assert bytes(h["magic"]) == b"FS2SNAP" and int(h["version"]) == 1 and int(h["total"]) == buf.size
    sec, total = sc.layout(N, R, U, C)
    assert total == buf.size and np.array_equal(h["sec"], sec)
    s = sc.section(buf, sc.SCALARS, np.uint8)
    x, y, yaw, w = (s[8 * N * k:8 * N * (k + 1)].view("<f8") for k in range(4))
    cnt = s[32 * N:36 * N].view("<i4")
    rows = sc.section(buf, sc.ROWS, "<u4").reshape(R, N)
    pages = sc.section(buf, sc.PAGES, "<u4").reshape(U, 8, 4)
    records = sc.section(buf, sc.RECORDS, "<f8").reshape(C, 6)
    return h, x, y, yaw, w, cnt, rows, pages, records


def decode(buf):
    """(x, y, yaw, w, cnt, lm [N][max(max cnt, 1)][6]): mirror position p of row r of
    particle i is live when 8 r + p < cnt_i; its record goes to the slot the mirror's
    low 12 bits of s name."""
    h, x, y, yaw, w, cnt, rows, pages, records = sections(buf)
    N, R = rows.shape[1], rows.shape[0]
    assert cnt.min() >= 0 and (int(cnt.max()) + 7) // 8 == R
    lm = np.zeros((N, max(int(cnt.max()), 1), 6))
    for r in range(R):
        for p in range(8):
            who = np.nonzero(cnt > 8 * r + p)[0]
            if not who.size:
                break
            e = rows[r, who]
            assert np.all(e != sc.NONE)
            page = (e & ~np.uint32(sc.OWNED)).astype(np.int64)
            assert page.max() < pages.shape[0]
            slot = (pages[page, p, 2] & 0xFFF).astype(np.int64)
            rec = pages[page, p, 3].astype(np.int64)
            assert rec.max() < records.shape[0] and np.all(slot < cnt[who])
            lm[who, slot] = records[rec]
    return x.copy(), y.copy(), yaw.copy(), w.copy(), cnt.copy(), lm
