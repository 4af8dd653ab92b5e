#!/usr/bin/env python3
"""Edge-case fixtures for the known-landmark clustering (fs2_cluster.hip): inputs
built to reach one path decision of the kernels each, with sklearn's labels and
the centres returned by the reference's own GeometryUtils.cluster_points
(fast_slam_2/utils/geometry_utils.py:26-62), imported as in gen_cluster.py.
Nothing from the reference is copied; only outputs on seeded inputs are saved.

For every case sklearn's labels are asserted equal to tests/ref_dbscan.py (the
brute-force restatement of the predicate in the header of fs2_cluster.hip) and
the reference's centres equal to its index-order means.  The one exception is
tie_two_point, which exists because sklearn differs there: its KD-tree accepts a
whole node on a square-rooted bound, and on a two-point input the node's far
corner is the other point.  What makes each case discriminating is asserted by
tests/cluster_edge_props.py, here and again in tests/test_cluster_golden.py.

Run:  python tests/golden/gen_cluster_edges.py   (writes tests/golden/cluster_edges.npz)
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import cluster_edge_props as props   # noqa: E402
import ref_dbscan                    # noqa: E402
from gen_cluster import import_reference   # noqa: E402

SIDE = 0.35355339059327373           # cell side / eps


def near_tie(rng, eps):
    """A partner (dx, dy) of the origin on the eps circle, dy moved by 0-2 ulps; None
    unless it is a near-tie worth keeping (every pair the stated predicate decides
    differently from the real-number comparison or from a square-rooted one, and a
    tenth of the others)."""
    th = rng.uniform(0, 2 * np.pi)
    dx, dy = eps * np.cos(th), eps * np.sin(th)
    for _ in range(int(rng.integers(0, 3))):
        dy = np.nextafter(dy, rng.choice([-np.inf, np.inf]))
    dx, dy = float(dx), float(dy)
    pred, exact, _, _ = props.predicate_forms(dx, dy, eps)
    if pred == exact and np.sqrt(dx * dx + dy * dy) <= eps and pred:
        return None
    if pred == exact and rng.random() < 0.9:
        return None
    return dx, dy


def tie_cases(rng, DBSCAN, cluster_points, data):
    fill = np.array([[a, b] for a in range(-18, 19, 6) for b in range(-18, 19, 6) if (a, b) != (0, 0)], float)
    assert len(fill) == 48
    G, P = props.TIE_GROUPS, props.TIE_PAIRS
    E = len(props.EPS_LIST)
    gp, gl, gk, gc = np.zeros((E, G, 50, 2)), np.zeros((E, G, 50), np.int32), np.zeros((E, G), np.int32), \
        np.full((E, G, 2), np.nan)
    gpair, counts = np.zeros((E, G, 2), np.int32), np.zeros((E, 4), np.int64)
    tp, tl, ts = np.zeros((E, P, 2, 2)), np.zeros((E, P, 2), np.int32), np.zeros((E, P, 2), np.int32)
    for e, eps in enumerate(props.EPS_LIST):
        g = p = agree = 0
        while g < G or p < P:
            t = near_tie(rng, eps)
            if t is None:
                continue
            pair = np.array([[0.0, 0.0], t])
            want = ref_dbscan.dbscan(pair, eps, 2)[0]
            if p < P:
                sk2 = DBSCAN(eps=eps, min_samples=2).fit(pair).labels_
                if not np.array_equal(sk2, want):
                    tp[e, p], tl[e, p], ts[e, p] = pair, want, sk2
                    p += 1
            if g < G:
                perm = rng.permutation(50)
                pts = np.concatenate([pair, fill])[perm]
                lab = DBSCAN(eps=eps, min_samples=2).fit(pts).labels_
                rl, rc = ref_dbscan.dbscan(pts, eps, 2)
                ok = np.array_equal(lab, rl)
                agree += ok
                assert ok, ("sklearn differs from the predicate on a filled group", eps, g)   # none dropped
                cen = np.array(cluster_points([tuple(q) for q in pts], eps=eps, min_samples=2)).reshape(-1, 2)
                assert np.array_equal(cen, rc)
                gp[e, g], gl[e, g], gk[e, g] = pts, lab, len(cen)
                if len(cen):
                    gc[e, g] = cen[0]
                inv = np.argsort(perm)
                gpair[e, g] = inv[:2]
                g += 1
        forms = np.array([props.predicate_forms(float(gp[e, k, gpair[e, k, 1], 0]),
                                                float(gp[e, k, gpair[e, k, 1], 1]), eps) for k in range(G)])
        counts[e] = [agree, (forms[:, 0] != forms[:, 1]).sum(), (forms[:, 0] != forms[:, 2]).sum(),
                     (forms[:, 0] != forms[:, 3]).sum()]
        assert agree == G
    data.update(tie_eps=np.array(props.EPS_LIST), tie_groups_points=gp, tie_groups_labels=gl, tie_groups_k=gk,
                tie_groups_centres=gc, tie_groups_pair=gpair, tie_groups_counts=counts,
                tie_two_points=tp, tie_two_labels=tl, tie_two_labels_sklearn=ts)


def window_case(rng):
    """Pairs at exactly eps (one cluster) and one step further out (noise), with p at
    fractional positions 0 / 0.01 / 0.5 / 0.99 of its cell in both axes, so the
    partners fall into cells 2 and 3 away in each axis and sign.  Every coordinate is
    a multiple of 2^-10, so every comparison is exact.  No dyadic vector off the axes
    has length exactly 0.5 (no Pythagorean triple has a power-of-two hypotenuse):
    the diagonal partners are the two lattice neighbours straddling the circle."""
    eps, q = 0.5, 1024.0
    side = eps * SIDE
    anchor = np.array([-7.25, 3.5])

    def coord(c, f):                 # offset from the anchor of fraction ~f of cell c
        v = (c + f) * side * q
        return (math.ceil(v) if f < 0.5 else math.floor(v)) / q

    a, b_in, b_out = 0.3125, 399 / q, 400 / q
    assert a * a + b_in * b_in < eps * eps < a * a + b_out * b_out
    partners = [((sx * eps, 0.0), (sx * eps, 0.0), 0) for sx in (1, -1)] + \
               [((0.0, sy * eps), (0.0, sy * eps), 1) for sy in (1, -1)] + \
               [((sx * a, sy * b_in), (sx * a, sy * b_out), -1) for sx in (1, -1) for sy in (1, -1)]
    pts, groups = [anchor], []

    def add(p, partner, tie):
        inner, outer, axis = partner
        p = np.asarray(p, dtype=np.float64)
        if tie:
            qq = p + inner
        elif axis < 0:
            qq = p + outer
        else:                        # one nextafter further out along the axis
            qq = p + inner
            qq[axis] = np.nextafter(qq[axis], np.inf if inner[axis] > 0 else -np.inf)
        groups.append((len(pts), len(pts) + 1, int(tie)))
        pts.extend([p, qq])

    fr = (0.0, 0.01, 0.5, 0.99)
    g = 0
    for fx in fr:
        for fy in fr:
            for partner in partners:
                for tie in (1, 0):
                    gi, gj = divmod(g, 16)
                    cbx, cby = round(5.0 * (gi + 1) / side), round(5.0 * (gj + 1) / side)
                    add(anchor + [coord(cbx, fx), coord(cby, fy)], partner, tie)
                    g += 1
    # cell indices below 3 (the window reaches below cell 0 there)
    for k, tie in enumerate((1, 0)):
        add(anchor + [coord(1, 0.5), coord(round(5.0 * (k + 1) / side), 0.5) + 2.5], partners[2], tie)
        add(anchor + [coord(round(5.0 * (k + 1) / side), 0.5) + 2.5, coord(1, 0.5)], partners[0], tie)
    pts = np.array(pts)
    perm = rng.permutation(len(pts))
    inv = np.argsort(perm)
    extra = {"window_groups": np.array([(inv[p], inv[qq], t) for p, qq, t in groups], np.int32),
             "window_anchor": np.array(inv[0])}
    return pts[perm], eps, 2, extra


def window_corners_case():
    """The corner cells of the 7x7 window.  A cell's diagonal is eps/2, so cells 3 away
    in both axes are out of reach in real numbers; in floating point a point whose
    scaled coordinate rounds to just below a cell boundary and a partner two cell
    sides away whose scaled coordinate rounds up onto one land there and still
    satisfy the predicate.  Both diagonals, with two far points fixing the origin."""
    eps = 0.5
    ih = 1.0 / (eps * SIDE)

    def cell(u):
        return int(np.floor(u * ih))

    def last_of(k):                  # the largest coordinate of cell k
        u = (k + 1) / ih
        while cell(u) > k:
            u = np.nextafter(u, -np.inf)
        while cell(np.nextafter(u, np.inf)) == k:
            u = np.nextafter(u, np.inf)
        return float(u)

    def first_of(k):                 # the smallest coordinate of cell k
        u = k / ih
        while cell(u) < k:
            u = np.nextafter(u, np.inf)
        while cell(np.nextafter(u, -np.inf)) == k:
            u = np.nextafter(u, -np.inf)
        return float(u)

    a0, a3, b6, b9 = last_of(0), first_of(3), last_of(6), first_of(9)
    for lo, hi in ((a0, a3), (b6, b9)):
        d = hi - lo
        assert d * d + d * d <= eps * eps, (lo, hi)
    pts = np.array([[0.0, 50.0], [50.0, 0.0], [a0, b6], [a3, b9], [b6, a3], [b9, a0]])
    # isolated fillers, as in tie_groups: they keep the pairs out of a tight KD-tree node,
    # so that sklearn tests them point by point
    fill = np.array([[a, b] for a in range(6, 43, 6) for b in range(6, 43, 6)], float)
    return np.concatenate([pts, fill]), eps, 2, {"window_corners_groups": np.array([[2, 3], [4, 5]], np.int32)}


def late_core_case(rng):
    """A cell of 130 points whose first 70 (by index) are out of reach of a tight blob
    of 150 and whose last 60 are in reach: with min_samples 200 only those 60 and the
    blob are core, so the cell's first core point is at sorted position 70."""
    eps = 0.5
    far = np.stack([rng.uniform(0.0, 0.07, 70), rng.uniform(0.0, 0.016, 70)], 1)
    far[0] = 0.0                                           # the set's minimum corner
    near = np.stack([rng.uniform(0.10, 0.17, 60), rng.uniform(0.0, 0.016, 60)], 1)
    blob = np.stack([0.585 + rng.uniform(-0.008, 0.008, 150), rng.uniform(0.0, 0.016, 150)], 1)
    return np.concatenate([far, blob, near]) + [12.0, -3.0], eps, 200, {}


def border_cases(rng):
    """gen_cluster.py's border_ms30 construction, with the lower-numbered cluster on
    the right and on the left; drawn again until the lone point is in reach of a
    core point of both."""
    while True:
        a2 = rng.normal([0, 0], 0.08, (300, 2))
        b2 = rng.normal([1.4, 0], 0.08, (300, 2))
        out = []
        for name, first, second in (("border_right_first", b2, a2), ("border_left_first", a2, b2)):
            pts = np.concatenate([first, [[0.7, 0.0]], second])
            nb = ref_dbscan.neighbour_lists(pts, 0.5)
            core = np.array([len(v) >= 30 for v in nb])
            sides = {bool(q < 300) for q in nb[300] if core[q]}
            if core[300] or sides != {True, False}:
                break
            out.append((name, pts, 0.5, 30, {f"{name}_lone": np.array(300)}))
        if len(out) == 2:
            return out


def snake_path(rows, per_row):
    """Boustrophedon: points 7/16 apart along rows 5/8 apart (out of reach of each
    other), rows joined at their ends by one point half-way up."""
    pts = []
    for r in range(rows):
        xs = np.arange(per_row) * (7 / 16)
        if r % 2:
            xs = xs[::-1]
        pts.extend((x, r * (5 / 8)) for x in xs)
        if r + 1 < rows:
            pts.append((xs[-1], r * (5 / 8) + 5 / 16))
    return np.array(pts)


def snake_pair_cases():
    """Two paths either side of x = -0.5: A starts at (0, 0) and runs right, B is its
    mirror image starting at (-1, 0), with one more point between them at (-0.5, 0):
    exactly eps from A's first point (one cluster), or one nextafter further (two)."""
    a = snake_path(10, 100)
    b = a * [-1.0, 1.0] + [-1.0, 0.0]
    out = []
    for name, x in (("snake_pair_touch", -0.5), ("snake_pair_apart", -np.nextafter(0.5, 1.0))):
        out.append((name, np.concatenate([a, [[x, 0.0]], b]), 0.5, 2, {}))
    return out


def sizes_case():
    """Clusters of 1 .. 193 members around large, uneven offsets (the sums round at
    every step) plus 300 isolated points, interleaved in index order; the seed is the
    first for which the sequential mean differs from numpy's pairwise sum / count in
    at least 5 of the 6 clusters of 65 or more."""
    offs = [(1234.5, -987.25), (-2048.75, 512.5), (77.125, 4096.5), (-333.375, -1500.0), (910.0625, 45.5),
            (-6000.5, 6000.25), (3000.75, 3100.125), (-450.25, 2222.5), (5120.375, -4096.625), (-777.5, -777.75)]
    iso = np.array([(7000.0 + 3 * i, -7000.0 + 3 * j) for i in range(20) for j in range(15)])
    for seed in range(1000):
        rng = np.random.default_rng(seed)
        pts = np.concatenate([rng.normal(c, 0.05, (m, 2)) for c, m in zip(offs, props.SIZES)] + [iso])
        pts = pts[rng.permutation(len(pts))]
        lab, cen = ref_dbscan.dbscan(pts, 0.5, 1)
        try:
            props.sizes({"sizes_points": pts, "sizes_labels": lab, "sizes_centres": cen})
        except AssertionError:
            continue
        return pts, 0.5, 1, {"sizes_seed": np.array(seed)}
    raise AssertionError("no seed gives the sizes condition")


def extremes_cases(rng):
    far = np.concatenate([rng.normal(c, 0.1, (100, 2)) for c in ([8e7, 8e7], [-8e7, 8e7], [8e7, -8e7])])
    tight = rng.uniform(-0.1, 0.1, (20, 2))
    return [("extremes_far", far[rng.permutation(300)], 0.5, 10, {}),
            ("extremes_identical", np.tile([[3.25, -1.5]], (100, 1)), 0.5, 50, {}),
            ("extremes_n1_ms1", np.array([[2.5, -4.0]]), 0.5, 1, {}),
            ("extremes_n1_ms2", np.array([[2.5, -4.0]]), 0.5, 2, {}),
            ("extremes_ms_np1", tight, 0.5, 21, {})]


def main():
    GeometryUtils, _, _, _ = import_reference()
    from sklearn.cluster import DBSCAN
    import sklearn
    rng = np.random.default_rng(2025)
    data = {"versions": np.array([f"numpy={np.__version__}", f"sklearn={sklearn.__version__}"])}
    tie_cases(rng, DBSCAN, GeometryUtils.cluster_points, data)
    cases = [("window",) + window_case(rng), ("window_corners",) + window_corners_case(),
             ("late_core",) + late_core_case(rng)] + border_cases(rng) + \
            [("snake", snake_path(40, 100), 0.5, 2, {})] + snake_pair_cases() + [("sizes",) + sizes_case()] + \
            extremes_cases(rng)
    names = []
    for name, pts, eps, ms, extra in cases:
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        labels = DBSCAN(eps=eps, min_samples=ms).fit(pts).labels_.astype(np.int32)
        centres = np.array(GeometryUtils.cluster_points([tuple(p) for p in pts], eps=eps, min_samples=ms),
                           dtype=np.float64).reshape(-1, 2)
        rl, rc = ref_dbscan.dbscan(pts, eps, ms)
        assert np.array_equal(labels, rl), name
        assert np.array_equal(centres, rc), name
        data[f"{name}_points"] = pts
        data[f"{name}_eps"] = np.array(eps)
        data[f"{name}_min_samples"] = np.array(ms)
        data[f"{name}_labels"] = labels
        data[f"{name}_centres"] = centres
        data.update(extra)
        names.append(name)
    data["names"] = np.array(names)
    for k, v in props.check_all(data).items():
        print(f"  {k}: {v}")
    out = os.path.join(HERE, "cluster_edges.npz")
    np.savez_compressed(out, **data)
    print("wrote cluster_edges.npz:", names, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
