"""Known-landmark clustering fixtures (tests/golden/gen_cluster.py and
gen_cluster_edges.py) pinned against sklearn's DBSCAN in this environment (the
library the reference calls in geometry_utils.py:26-62): labels equal, and each
recorded reference centre equals the numpy mean of its cluster's points in index
order.  tests/ref_dbscan.py -- the brute-force restatement of the predicate that
the GPU tests compare with -- is pinned to both fixtures and to sklearn here, and
the properties that make each edge case discriminating (cluster_edge_props.py) are
asserted from the committed file alone."""
import os

import numpy as np
import pytest

import cluster_edge_props as props
import ref_dbscan
from conftest import GOLDEN


def _load():
    return np.load(os.path.join(GOLDEN, "cluster_cases.npz"))


@pytest.fixture(scope="module")
def edges():
    d = np.load(os.path.join(GOLDEN, "cluster_edges.npz"))
    return {k: d[k] for k in d.files}


def test_fixture_labels_match_sklearn():
    sk = pytest.importorskip("sklearn.cluster")
    d = _load()
    for n in d["names"]:
        pts = d[f"{n}_points"]
        lab = sk.DBSCAN(eps=float(d[f"{n}_eps"]), min_samples=int(d[f"{n}_min_samples"])).fit(pts).labels_
        assert np.array_equal(lab, d[f"{n}_labels"]), n


def test_fixture_centres_are_index_order_means():
    d = _load()
    for n in d["names"]:
        pts, lab, cen = d[f"{n}_points"], d[f"{n}_labels"], d[f"{n}_centres"]
        K = lab.max() + 1
        assert len(cen) == K, n
        for k in range(K):
            m = pts[lab == k]
            s = np.zeros(2)
            for p in m:                  # sequential, like numpy mean(axis=0)
                s = s + p
            assert np.array_equal(cen[k], s / len(m)), (n, k)


def _assert_ref_equals(d, n):
    lab, cen = ref_dbscan.dbscan(d[f"{n}_points"], float(d[f"{n}_eps"]), int(d[f"{n}_min_samples"]))
    assert lab.dtype == np.int32 and np.array_equal(lab, d[f"{n}_labels"]), n
    assert cen.shape == d[f"{n}_centres"].shape and np.array_equal(cen, d[f"{n}_centres"]), n


def test_ref_dbscan_equals_recorded_cases():
    d = _load()
    for n in d["names"]:
        _assert_ref_equals(d, n)
    cnt, lm = d["known_cnt"], d["known_lm"]
    pts = ref_dbscan.known_landmark_points(cnt, lm)
    assert len(pts) == cnt.sum()
    ms = ref_dbscan.min_samples_of(len(pts), len(cnt), 0.7)
    assert ms == int(len(pts) / len(cnt) * 0.7)
    assert np.array_equal(ref_dbscan.dbscan(pts, 0.5, ms)[1], d["known_centres"])


def test_ref_dbscan_equals_edge_cases(edges):
    d = edges
    for n in d["names"]:
        _assert_ref_equals(d, n)
    for e, eps in enumerate(d["tie_eps"]):
        for g in range(props.TIE_GROUPS):
            lab, cen = ref_dbscan.dbscan(d["tie_groups_points"][e, g], float(eps), 2)
            assert np.array_equal(lab, d["tie_groups_labels"][e, g]), (eps, g)
            assert len(cen) == d["tie_groups_k"][e, g], (eps, g)
            if len(cen):
                assert np.array_equal(cen[0], d["tie_groups_centres"][e, g]), (eps, g)
        for g in range(props.TIE_PAIRS):
            lab, _ = ref_dbscan.dbscan(d["tie_two_points"][e, g], float(eps), 2)
            assert np.array_equal(lab, d["tie_two_labels"][e, g]), (eps, g)


def test_edge_fixture_reaches_its_paths(edges):
    """The conditions gen_cluster_edges.py asserted when it wrote the fixture, from the
    committed file alone (near-ties that separate the predicate from its look-alikes,
    cell offsets 2 and 3 in each axis and sign, a first core point past a cell's first
    64, a component of thousands of cells, centres whose tree sum rounds differently)."""
    for k, v in props.check_all(edges).items():
        print(f"{k}: {v}")
    assert os.path.getsize(os.path.join(GOLDEN, "cluster_edges.npz")) < 500_000


def test_edge_fixture_labels_match_sklearn(edges):
    """sklearn run here equals every recorded label set; on the two-point near-ties it
    gives its own recorded answer, which is not the per-point predicate's."""
    sk = pytest.importorskip("sklearn.cluster")
    d = edges
    for n in d["names"]:
        lab = sk.DBSCAN(eps=float(d[f"{n}_eps"]), min_samples=int(d[f"{n}_min_samples"])).fit(
            d[f"{n}_points"]).labels_
        assert np.array_equal(lab, d[f"{n}_labels"]), n
    for e, eps in enumerate(d["tie_eps"]):
        for g in range(props.TIE_GROUPS):
            lab = sk.DBSCAN(eps=float(eps), min_samples=2).fit(d["tie_groups_points"][e, g]).labels_
            assert np.array_equal(lab, d["tie_groups_labels"][e, g]), (eps, g)
        for g in range(props.TIE_PAIRS):
            lab = sk.DBSCAN(eps=float(eps), min_samples=2).fit(d["tie_two_points"][e, g]).labels_
            assert np.array_equal(lab, d["tie_two_labels_sklearn"][e, g]), (eps, g)


def test_ref_dbscan_equals_sklearn_random():
    """6 blobs of 300 plus 600 uniform points, min_samples 3-19: no near-ties, so
    sklearn's tree shortcut cannot matter and the labels are equal."""
    sk = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(3)
    for trial in range(3):
        pts = np.concatenate([rng.normal(c, 0.2, (300, 2)) for c in rng.uniform(-5, 5, (6, 2))] +
                             [rng.uniform(-6, 6, (600, 2))])
        ms = int(rng.integers(3, 20))
        lab = sk.DBSCAN(eps=0.5, min_samples=ms).fit(pts).labels_
        assert np.array_equal(ref_dbscan.dbscan(pts, 0.5, ms)[0], lab), trial
