"""Loader of the shape-edge fixtures (tests/golden/ref_edges_assoc.npz and
ref_edges_geom.npz, recorded by tests/golden/gen_ref_edges.py), shared by
tests/test_oracle_edges.py (the C oracle, on the CPU) and
tests/test_gpu_primitives.py (libfs2, on the GPU)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

AS_LENS = (1, 63, 64, 65, 127, 128, 129, 200)
BF_N = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049)
ICP_SHAPES = ((1, 1), (1, 1024), (2, 3), (63, 64), (64, 64), (65, 63), (129, 1000), (1024, 7),
              (1024, 1024))
LF_N = (1, 2, 3, 127, 128, 129, 300)
LF_SIGMA = (0.1, 0.5, 2.5, 8.0)

_cache = None


def load():
    """(assoc, geom) as dicts; every primitive's cases are there in full (the
    counts and shapes the generator draws), so a truncated fixture fails."""
    global _cache
    if _cache is not None:
        return _cache
    a = dict(np.load(os.path.join(GOLDEN, "ref_edges_assoc.npz")))
    g = dict(np.load(os.path.join(GOLDEN, "ref_edges_geom.npz")))
    K = 133
    assert len(a["as_obs"]) == len(a["as_gate"]) == len(a["assoc"]) == K
    lens = [len(a[f"as_lm_{k}"]) for k in range(K)]
    assert sorted(set(lens)) == list(AS_LENS)
    assert set(a["as_gate"].tolist()) == {0.5, 2.0, 8.0}
    assert int((a["assoc"] == -2).sum()) == 52 and int((a["assoc"] == -1).sum()) == 8
    assert int(g["bf_n"]) == len(g["bf_R"]) == len(g["bf_t"]) == len(g["bf_R_ld"]) == len(g["bf_t_ld"]) == 10
    assert tuple(len(g[f"bf_src_{k}"]) for k in range(10)) == BF_N
    assert tuple(len(g[f"bf_tgt_{k}"]) for k in range(10)) == BF_N
    assert int(g["icp_n"]) == len(g["icp_R"]) == len(g["icp_t"]) == 9
    assert tuple((len(g[f"icp_src_{k}"]), len(g[f"icp_tgt_{k}"])) for k in range(9)) == ICP_SHAPES
    assert len(g["lf_sigma"]) == 28
    assert [(len(g[f"lf_pts_{k}"]), float(g["lf_sigma"][k])) for k in range(28)] == \
        [(n, s) for n in LF_N for s in LF_SIGMA]
    assert all(g[f"lf_{k}"].shape == g[f"lf_ld_{k}"].shape == g[f"lf_pts_{k}"].shape for k in range(28))
    _cache = (a, g)
    return _cache


def ref_bar(project_bar, ref, exact):
    """max(the project's bar, 4 x the reference's own distance from the recorded
    long-double result): as wrong as float64 numpy is and no more."""
    return max(project_bar, 4.0 * float(np.abs(np.asarray(ref) - np.asarray(exact)).max()))
