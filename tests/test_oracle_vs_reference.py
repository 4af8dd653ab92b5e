"""Property tests: the C oracle against the reference itself on random inputs.

SURVEY.md §4's build test plan: per primitive, random cases (including edge
cases: ill-conditioned covariances, weights below the 1e-5 floor, zero weights,
exact ties, resample start points at cumulative-weight boundaries) went
through the reference (tests/ref_primitives.py, in a process of its own because
the reference package is also named `fast_slam_2`) and go through the oracle
here.  The cases and the reference's outputs on them are fixtures
(tests/golden/ref_primitives_cases.npz, ref_primitives_out.npz, recorded by
tests/golden/gen_ref_primitives.py where the reference is installed), so the
comparison runs wherever the suite does.

Bars: Mahalanobis distance, association index, normalised weights, N_eff,
estimate index and resample sources bit-exact; best-fit / ICP / LineFilter
within 1e-12 (SVD / KDTree / scipy correlate vs closed forms).
"""
import os

import numpy as np
import pytest

from oracle import oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def both():
    cases = dict(np.load(os.path.join(GOLDEN, "ref_primitives_cases.npz")))
    ref = dict(np.load(os.path.join(GOLDEN, "ref_primitives_out.npz")))
    # every primitive's cases are there in full (the counts the generator draws)
    assert len(cases["maha_a"]) == len(ref["maha"]) == 1500
    assert len(cases["as_obs"]) == len(ref["assoc"]) == 300
    assert len(cases["w_len"]) == len(ref["norm_w"]) == len(ref["src"]) == 250
    assert len(cases["bf_src"]) == len(ref["bf_R"]) == 60 and len(cases["icp_src"]) == len(ref["icp_R"]) == 12
    assert len(cases["lf_pts"]) == len(ref["lf"]) == 40
    return cases, ref


def test_mahalanobis_bit_exact(both):
    c, r = both
    got = np.array([orc.mahalanobis(a, b, cv) for a, b, cv in zip(c["maha_a"], c["maha_b"], c["maha_cov"])])
    assert np.array_equal(got, r["maha"], equal_nan=True)


def test_association_exact(both):
    c, r = both
    for k in range(len(c["as_obs"])):
        L = c["as_len"][k]
        assert orc.associate(c["as_obs"][k], c["as_lm"][k, :L], c["as_gate"][k]) == r["assoc"][k], k


def test_weights_neff_estimate_resample(both):
    c, r = both
    hung = 0
    for k in range(len(c["w_len"])):
        N = c["w_len"][k]
        w = c["w"][k, :N]
        nw = orc.normalize(w)
        assert np.array_equal(nw, r["norm_w"][k, :N]), k
        assert orc.n_eff(nw) == r["n_eff"][k], k
        assert orc.argmax_first(nw) == int(r["est_x"][k]), k
        src = orc.resample_src(nw, c["u0"][k])
        if r["src"][k, 0] == -2:
            hung += 1                      # reference hangs (Q10); the oracle ends on N-1
            continue
        assert np.array_equal(src, r["src"][k, :N]), k
    assert hung < len(c["w_len"]) // 4


def test_best_fit_and_icp(both):
    c, r = both
    for k in range(len(c["bf_src"])):
        R, t = orc.best_fit(c["bf_src"][k], c["bf_tgt"][k])
        assert np.allclose(R, r["bf_R"][k], atol=1e-12) and np.allclose(t, r["bf_t"][k], atol=1e-11), k
    for k in range(len(c["icp_src"])):
        R, t, _ = orc.icp(c["icp_src"][k], c["icp_tgt"][k])
        assert np.allclose(R, r["icp_R"][k], atol=1e-10) and np.allclose(t, r["icp_t"][k], atol=1e-9), k


def test_line_filter(both):
    c, r = both
    for k in range(len(c["lf_pts"])):
        got = orc.line_filter(c["lf_pts"][k], c["lf_sigma"][k])
        assert np.allclose(got, r["lf"][k], rtol=1e-13, atol=1e-13), k
