"""What makes each case of tests/golden/cluster_edges.npz discriminating, computed
from the fixture alone.  gen_cluster_edges.py asserts these when it writes the
fixture and test_cluster_golden.py asserts them again on the committed file, so a
regenerated fixture cannot silently stop reaching the path it was built for.

The cell layout is fs2_cluster.hip's own: origin at the minimum corner, cells of
side eps / (2 sqrt 2), points sorted by (cy, cx) and by index inside a cell."""
from fractions import Fraction as F

import numpy as np

import ref_dbscan

EPS_LIST = (0.5, 0.3, 0.7)
TIE_GROUPS = 150
TIE_PAIRS = 30
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 192, 193)
ISOLATED = 300


def kernel_cells(points, eps):
    """(cx, cy) of every point by k_cl_keys' formula."""
    pts = np.asarray(points, dtype=np.float64)
    ih = 1.0 / (eps * 0.35355339059327373)
    x0, y0 = pts[:, 0].min(), pts[:, 1].min()
    return (np.floor((pts[:, 0] - x0) * ih).astype(np.int64),
            np.floor((pts[:, 1] - y0) * ih).astype(np.int64))


def core_flags(points, eps, min_samples):
    return np.array([len(v) >= min_samples for v in ref_dbscan.neighbour_lists(points, eps)])


def predicate_forms(dx, dy, eps):
    """(stated predicate, exact rational, hypot form, FMA-contracted form) for one pair."""
    eps2 = eps * eps
    pred = dx * dx + dy * dy <= eps2
    exact = F(dx) ** 2 + F(dy) ** 2 <= F(eps) ** 2
    hyp = bool(np.hypot(dx, dy) <= eps)
    fma = float(F(dx) * F(dx) + F(dy * dy)) <= eps2      # fl(dx*dx + fl(dy*dy)), one rounding
    return bool(pred), bool(exact), hyp, bool(fma)


def tie_groups(d):
    """Per eps: [groups, predicate != exact, predicate != hypot, predicate != fma].
    Asserts that the recorded labels are the stated predicate's."""
    out = []
    for e, eps in enumerate(EPS_LIST):
        assert float(d["tie_eps"][e]) == eps
        pts, lab, pair = d["tie_groups_points"][e], d["tie_groups_labels"][e], d["tie_groups_pair"][e]
        assert pts.shape == (TIE_GROUPS, 50, 2)
        n_exact = n_hyp = n_fma = 0
        for g in range(TIE_GROUPS):
            o, q = pair[g]
            assert pts[g, o, 0] == 0.0 and pts[g, o, 1] == 0.0
            dx, dy = float(pts[g, q, 0]), float(pts[g, q, 1])
            pred, exact, hyp, fma = predicate_forms(dx, dy, eps)
            assert abs(dx * dx + dy * dy - eps * eps) <= 16 * np.spacing(eps * eps), (eps, g)   # a near-tie
            want = np.full(50, -1, dtype=np.int32)
            if pred:
                want[[o, q]] = 0
            assert np.array_equal(lab[g], want), (eps, g)
            assert int(d["tie_groups_k"][e, g]) == int(pred)
            n_exact += pred != exact
            n_hyp += pred != hyp
            n_fma += pred != fma
        out.append([TIE_GROUPS, int(n_exact), int(n_hyp), int(n_fma)])
        assert n_exact >= 100, (eps, n_exact)
    assert out[0][2] > 0 and out[0][3] > 0, out[0]
    assert np.array_equal(np.array(out), d["tie_groups_counts"])
    return out


def tie_two_point(d):
    """Every pair is a near-tie on which the recorded sklearn labels differ from the
    stated predicate's; returns the number of pairs per eps."""
    out = []
    for e, eps in enumerate(EPS_LIST):
        pts = d["tie_two_points"][e]
        assert pts.shape == (TIE_PAIRS, 2, 2)
        for g in range(TIE_PAIRS):
            dx, dy = pts[g, 1] - pts[g, 0]
            pred = predicate_forms(float(dx), float(dy), eps)[0]
            want = np.array([0, 0] if pred else [-1, -1], dtype=np.int32)
            assert np.array_equal(d["tie_two_labels"][e, g], want), (eps, g)
            assert not np.array_equal(d["tie_two_labels_sklearn"][e, g], want), (eps, g)
        out.append(TIE_PAIRS)
    return out


def window(d):
    """Cell offsets (x set, y set) of the tie pairs; ties cluster, twins are noise."""
    pts, lab, grp = d["window_points"], d["window_labels"], d["window_groups"]
    eps = float(d["window_eps"])
    dyadic = (pts * 1024.0 == np.round(pts * 1024.0)).all(axis=1)     # so every tie is exact
    assert dyadic[grp[:, 0]].all() and dyadic[grp[grp[:, 2] == 1, 1]].all()
    cx, cy = kernel_cells(pts, eps)
    anchor = int(d["window_anchor"])
    assert cx[anchor] == 0 and cy[anchor] == 0 and lab[anchor] == -1
    assert pts[anchor, 0] == pts[:, 0].min() and pts[anchor, 1] == pts[:, 1].min()
    offx, offy, lowx, lowy = set(), set(), 0, 0
    seen = set()
    for p, q, tie in grp:
        if tie:
            assert lab[p] == lab[q] >= 0 and (lab == lab[p]).sum() == 2, (p, q)
            assert lab[p] not in seen
            seen.add(int(lab[p]))
            offx.add(int(cx[q] - cx[p]))
            offy.add(int(cy[q] - cy[p]))
            lowx += bool(cx[p] < 3)
            lowy += bool(cy[p] < 3)
        else:
            assert lab[p] == -1 and lab[q] == -1, (p, q)
    assert {-3, -2, 2, 3} <= offx and {-3, -2, 2, 3} <= offy, (offx, offy)
    assert lowx >= 1 and lowy >= 1
    assert len(seen) == lab.max() + 1
    return sorted(offx), sorted(offy), lowx, lowy


def window_corners(d):
    """Cell offsets of the two pairs: 3 in both axes (both diagonals of the window),
    each pair a cluster although a cell's diagonal is eps/2."""
    pts, lab = d["window_corners_points"], d["window_corners_labels"]
    cx, cy = kernel_cells(pts, float(d["window_corners_eps"]))
    offs = []
    for k, (p, q) in enumerate(d["window_corners_groups"]):
        assert lab[p] == lab[q] == k and (lab == k).sum() == 2
        offs.append((int(cx[q] - cx[p]), int(cy[q] - cy[p])))
    assert offs == [(3, 3), (3, -3)], offs
    assert (lab == -1).sum() == len(lab) - 4 and lab.max() == 1
    assert pts[:, 0].min() == 0.0 and pts[:, 1].min() == 0.0
    return offs


def late_core(d):
    """(points in the big cell, sorted position of its first core point)."""
    pts, lab = d["late_core_points"], d["late_core_labels"]
    eps, ms = float(d["late_core_eps"]), int(d["late_core_min_samples"])
    cx, cy = kernel_cells(pts, eps)
    key = cy * (1 << 32) + cx
    members = np.flatnonzero(key == key[0])        # index order = the stable sort's order in the cell
    assert len(members) == 130
    core = core_flags(pts, eps, ms)
    first = int(np.argmax(core[members]))
    assert core[members].any() and first >= 64, first
    far = members[:first]
    assert not core[far].any() and np.all(lab[far] == 0)      # border points of the one cluster
    assert np.all(lab == 0)
    return len(members), first


def border_both_orders(d):
    """x of cluster 0's centre in the two orders; the lone point is a border point in
    reach of both clusters and takes the lower number."""
    out = []
    for name in ("border_right_first", "border_left_first"):
        pts, lab = d[f"{name}_points"], d[f"{name}_labels"]
        eps, ms = float(d[f"{name}_eps"]), int(d[f"{name}_min_samples"])
        lone = int(d[f"{name}_lone"])
        nb = ref_dbscan.neighbour_lists(pts, eps)
        core = np.array([len(v) >= ms for v in nb])
        assert lab.max() == 1 and not core[lone] and lab[lone] == 0
        reach = {int(lab[q]) for q in nb[lone] if core[q]}
        assert reach == {0, 1}, reach
        out.append(float(d[f"{name}_centres"][0, 0]))
    assert out[0] > 0.7 > out[1]
    return out


def snake(d):
    """Distinct cells of the one cluster."""
    pts, lab = d["snake_points"], d["snake_labels"]
    assert np.all(lab == 0)
    cx, cy = kernel_cells(pts, float(d["snake_eps"]))
    cells = len(np.unique(cy * (1 << 32) + cx))
    assert cells >= 3000, cells
    return len(pts), cells


def snake_pair(d):
    a, b = d["snake_pair_touch_points"], d["snake_pair_apart_points"]
    diff = np.flatnonzero((a != b).any(axis=1))
    assert len(diff) == 1 and a[diff[0], 0] == -0.5 and b[diff[0], 0] == -np.nextafter(0.5, 1.0)
    assert np.all(d["snake_pair_touch_labels"] == 0)
    lab = d["snake_pair_apart_labels"]
    assert set(lab.tolist()) == {0, 1}
    return len(a), int((lab == 0).sum()), int((lab == 1).sum())


def sizes(d):
    """(K, clusters of >= 65 members whose sequential mean differs from the pairwise one)."""
    pts, lab, cen = d["sizes_points"], d["sizes_labels"], d["sizes_centres"]
    K = int(lab.max()) + 1
    assert lab.min() == 0 and K == len(SIZES) + ISOLATED and K > 64
    count = np.bincount(lab)
    assert sorted(count[count > 1].tolist() + [1]) == sorted(SIZES)
    assert (count == 1).sum() == ISOLATED + 1
    differ = big = 0
    for k in np.flatnonzero(count >= 65):
        m = pts[lab == k]
        pairwise = np.array([np.add.reduce(np.ascontiguousarray(m[:, c])) for c in range(2)]) / len(m)
        big += 1
        differ += bool((pairwise != cen[k]).any())
    assert big == 6 and differ >= 5, (big, differ)
    return K, differ


def extremes(d):
    far = d["extremes_far_points"]
    eps = float(d["extremes_far_eps"])
    ext = np.abs(far).max()
    assert 7.9e7 < ext and 2.0 * ext / (eps * 0.35355339059327373) <= 2.0e9     # inside the span limit
    assert d["extremes_far_labels"].max() == 2
    same = d["extremes_identical_points"]
    assert len(same) == 100 and (same == same[0]).all() and np.all(d["extremes_identical_labels"] == 0)
    assert np.array_equal(d["extremes_identical_centres"], same[:1])
    assert len(d["extremes_n1_ms1_points"]) == 1 and d["extremes_n1_ms1_labels"].tolist() == [0]
    assert np.array_equal(d["extremes_n1_ms1_centres"], d["extremes_n1_ms1_points"])
    assert len(d["extremes_n1_ms2_points"]) == 1 and d["extremes_n1_ms2_labels"].tolist() == [-1]
    n = len(d["extremes_ms_np1_points"])
    assert int(d["extremes_ms_np1_min_samples"]) == n + 1 and np.all(d["extremes_ms_np1_labels"] == -1)
    # one fewer would cluster them all: the points are within eps of each other
    assert np.all(ref_dbscan.dbscan(d["extremes_ms_np1_points"], eps, n)[0] == 0)
    return float(ext)


def check_all(d):
    """Every condition above; the measured figures, for the generator's and the test's output."""
    return {"tie_groups [groups, != exact, != hypot, != fma] per eps": tie_groups(d),
            "tie_two_point pairs per eps": tie_two_point(d),
            "window (x offsets, y offsets, ties with cx < 3, with cy < 3)": window(d),
            "window_corners cell offsets": window_corners(d),
            "late_core (cell size, first core position)": late_core(d),
            "border_both_orders cluster-0 x": border_both_orders(d),
            "snake (points, cells)": snake(d),
            "snake_pair (points, cluster sizes apart)": snake_pair(d),
            "sizes (K, sequential != pairwise of 6)": sizes(d),
            "extremes max |coordinate|": extremes(d)}
