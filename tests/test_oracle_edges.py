"""The C oracle against the reference at the shape edges of the stand-alone GPU
primitives (tests/golden/ref_edges_*.npz, recorded from the reference by
tests/golden/gen_ref_edges.py): lists of 1..200 landmarks with the first match
and singular covariances on both sides of every 64-landmark boundary, best fits
of 1..2049 points, ICP with 1..1024 source and target points, line filters whose
radius is many times the number of points.

tests/test_gpu_primitives.py judges libfs2 by the oracle at these shapes (ICP
iteration counts) and by the same recorded results; this module pins the checker
there first.  Bars as in tests/test_oracle_vs_reference.py: association exact,
best fit 1e-12 / 1e-11, ICP 1e-10 / 1e-9, line filter 1e-13.
"""
import numpy as np
import pytest

import edge_cases
from oracle import oracle as orc


@pytest.fixture(scope="module")
def edges():
    return edge_cases.load()


def test_association_exact(edges):
    a, _ = edges
    for k in range(len(a["as_obs"])):
        assert orc.associate(a["as_obs"][k], a[f"as_lm_{k}"], a["as_gate"][k]) == a["assoc"][k], k


def test_association_covers_the_chunk_edges(edges):
    """The fixture holds what it was drawn for: per list length, the first match at
    0, 63, 64, 127, 128 and L - 1 where they exist, and both orders of a singular
    covariance and a match."""
    a, _ = edges
    seen = {}
    for k in range(len(a["as_obs"])):
        seen.setdefault(len(a[f"as_lm_{k}"]), set()).add(int(a["assoc"][k]))
    for L in edge_cases.AS_LENS:
        want = {p for p in (0, 63, 64, 127, 128, L - 1) if p < L} | {-1, -2}
        assert want <= seen[L], (L, sorted(want - seen[L]))
    assert 70 in seen[200]


def test_best_fit(edges):
    _, g = edges
    for k in range(int(g["bf_n"])):
        R, t = orc.best_fit(g[f"bf_src_{k}"], g[f"bf_tgt_{k}"])
        assert np.allclose(R, g["bf_R"][k], rtol=0, atol=1e-12), k
        assert np.allclose(t, g["bf_t"][k], rtol=0, atol=1e-11), k
        # the recorded long-double closed form is the same rotation
        assert np.allclose(g["bf_R_ld"][k], g["bf_R"][k], rtol=0, atol=1e-12), k
        assert np.allclose(g["bf_t_ld"][k], g["bf_t"][k], rtol=0, atol=1e-11), k


def test_icp(edges):
    _, g = edges
    for k in range(int(g["icp_n"])):
        R, t, it = orc.icp(g[f"icp_src_{k}"], g[f"icp_tgt_{k}"])
        assert 1 < it < 100, (k, it)
        assert np.allclose(R, g["icp_R"][k], rtol=0, atol=1e-10), k
        assert np.allclose(t, g["icp_t"][k], rtol=0, atol=1e-9), k


def test_line_filter(edges):
    _, g = edges
    for k, s in enumerate(g["lf_sigma"]):
        got = orc.line_filter(g[f"lf_pts_{k}"], s)
        assert np.allclose(got, g[f"lf_{k}"], rtol=1e-13, atol=1e-13), k
        assert np.allclose(g[f"lf_ld_{k}"], g[f"lf_{k}"], rtol=1e-13, atol=1e-13), k
