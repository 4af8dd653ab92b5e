"""The stand-alone GPU primitives (fast-slam_amd/csrc/fs2_geometry.hip: k_icp,
k_best_fit, k_line_filter, k_mahalanobis, k_associate) and the small-N tail of the
filter against what the reference itself computed, at the shapes where the
kernels change path.  Every call goes through the shim and the C ABI (ctypes).

a. the whole of tests/golden/ref_primitives_{cases,out}.npz (recorded from the
   reference by gen_ref_primitives.py; so far only the C oracle saw it);
b. tests/golden/ref_edges_*.npz (gen_ref_edges.py): lists around k_associate's
   64-landmark trips with singular covariances on both sides of the first match,
   best fits around k_best_fit's 1024-point stride, ICP from 1 to 1024 points with
   P != n_tgt, line filters whose radius is many times n;
c. the entry points of one kernel agree with one another bit for bit, and refuse
   0 and 1025 points;
d. normalise / N_eff / estimate / resample for N <= 64 on the 250 recorded weight
   vectors (below the floor, zeros, ties, totals below 1e-5, boundary u0).

Bars.  Mahalanobis, association, the tail: bit-exact.  ICP: R 1e-10, t 1e-9 and
the oracle's iteration count (tests/test_oracle_edges.py pins the oracle at the
same cases).  Best fit and line filter on the edge fixture: against the recorded
long-double evaluation, within max(the project's bar -- 1e-12 / 1e-11 / 1e-13 --,
4 x the reference's own distance from it): the kernel may be as wrong as float64
numpy is and no more.  No bar comes from what the kernels give.
"""
import ctypes as C
import os
import time

import numpy as np
import pytest

import edge_cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fs():
    import torch  # noqa: F401  (loads the HIP runtime first)
    import fast_slam_2
    from gpu_util import configure
    yield fast_slam_2
    configure()


@pytest.fixture(scope="module")
def prim():
    c = dict(np.load(os.path.join(GOLDEN, "ref_primitives_cases.npz")))
    r = dict(np.load(os.path.join(GOLDEN, "ref_primitives_out.npz")))
    assert len(c["maha_a"]) == len(r["maha"]) == 1500
    assert len(c["as_obs"]) == len(r["assoc"]) == 300
    assert len(c["w_len"]) == len(r["norm_w"]) == len(r["src"]) == 250
    assert len(c["bf_src"]) == len(r["bf_R"]) == 60 and len(c["icp_src"]) == len(r["icp_R"]) == 12
    assert len(c["lf_pts"]) == len(r["lf"]) == 40
    return c, r


@pytest.fixture(scope="module")
def edges():
    return edge_cases.load()


def associate(fs, obs, lm, gate):
    """LandmarkUtils.associate_landmarks on rows (x, y, cov): the index, -1 for
    (None, None), -2 for numpy.linalg.LinAlgError."""
    from gpu_util import configure
    configure(gate=float(gate))
    lms = [fs.Landmark(r[0], r[1], r[2:6].reshape(2, 2)) for r in lm]
    try:
        got, idx = fs.LandmarkUtils.associate_landmarks(fs.Landmark(obs[0], obs[1]), lms)
    except np.linalg.LinAlgError:
        return -2
    if idx is None:
        assert got is None
        return -1
    assert got is lms[idx]
    return idx


# ------------------------------------------- a. the ref_primitives fixture ---

def test_mahalanobis_all_and_block_edges(fs, prim):
    """All 1500 distances bit-equal; prefixes around k_mahalanobis's 256-thread
    blocks; one zero covariance in the last element raises."""
    c, r = prim
    got = fs.GeometryUtils.mahalanobis_distances(c["maha_a"], c["maha_b"], c["maha_cov"])
    assert np.array_equal(got, r["maha"], equal_nan=True)
    for K in (1, 255, 256, 257, 513):
        got = fs.GeometryUtils.mahalanobis_distances(c["maha_a"][:K], c["maha_b"][:K], c["maha_cov"][:K])
        assert got.shape == (K,)
        assert np.array_equal(got, r["maha"][:K], equal_nan=True), K
        cov = c["maha_cov"][:K].copy()
        cov[K - 1] = 0.0
        with pytest.raises(np.linalg.LinAlgError):
            fs.GeometryUtils.mahalanobis_distances(c["maha_a"][:K], c["maha_b"][:K], cov)


def test_association_all(fs, prim):
    c, r = prim
    for k in range(len(c["as_obs"])):
        L = int(c["as_len"][k])
        assert associate(fs, c["as_obs"][k], c["as_lm"][k, :L], c["as_gate"][k]) == r["assoc"][k], k


def test_best_fit_all(fs, prim):
    c, r = prim
    for k in range(len(c["bf_src"])):
        R, t = fs.ICP.best_fit_transform(c["bf_src"][k], c["bf_tgt"][k])
        assert np.abs(R - r["bf_R"][k]).max() <= 1e-12, k
        assert np.abs(t - r["bf_t"][k]).max() <= 1e-11, k


def test_icp_all(fs, prim):
    from oracle import oracle as orc
    c, r = prim
    for k in range(len(c["icp_src"])):
        R, t, it = fs.ICP.get_transformation_ex(c["icp_src"][k], c["icp_tgt"][k])
        assert it == orc.icp(c["icp_src"][k], c["icp_tgt"][k])[2], k
        assert np.abs(R - r["icp_R"][k]).max() <= 1e-10, k
        assert np.abs(t - r["icp_t"][k]).max() <= 1e-9 * max(1.0, np.abs(r["icp_t"][k]).max()), k


def test_line_filter_all(fs, prim):
    c, r = prim
    for k in range(len(c["lf_pts"])):
        got = fs.LineFilter.filter(c["lf_pts"][k], c["lf_sigma"][k])
        assert np.all(np.abs(got - r["lf"][k]) <= 1e-13 + 1e-13 * np.abs(r["lf"][k])), k


# ---------------------------------------------------- b. the edge fixture ---

def test_association_edges(fs, edges):
    """Index exact; -2: LinAlgError; -1: (None, None)."""
    a, _ = edges
    for k in range(len(a["as_obs"])):
        lm = a[f"as_lm_{k}"]
        got = associate(fs, a["as_obs"][k], lm, a["as_gate"][k])
        assert got == a["assoc"][k], (k, len(lm), got, int(a["assoc"][k]))


def test_best_fit_edges(fs, edges):
    _, g = edges
    worst = [0.0, 0.0]
    for k, n in enumerate(edge_cases.BF_N):
        R, t = fs.ICP.best_fit_transform(g[f"bf_src_{k}"], g[f"bf_tgt_{k}"])
        eR, et = np.abs(R - g["bf_R_ld"][k]).max(), np.abs(t - g["bf_t_ld"][k]).max()
        bR = edge_cases.ref_bar(1e-12, g["bf_R"][k], g["bf_R_ld"][k])
        bt = edge_cases.ref_bar(1e-11, g["bf_t"][k], g["bf_t_ld"][k])
        print(f"best fit n={n}: |R - exact| {eR:.3g} (bar {bR:.3g}), |t - exact| {et:.3g} (bar {bt:.3g})")
        worst = [max(worst[0], eR), max(worst[1], et)]
        assert eR <= bR and et <= bt, (n, eR, bR, et, bt)
    print(f"best fit, largest deviation: R {worst[0]:.3g}, t {worst[1]:.3g}")


def test_icp_edges(fs, edges):
    from oracle import oracle as orc
    _, g = edges
    worst = [0.0, 0.0]
    for k, shape in enumerate(edge_cases.ICP_SHAPES):
        src, tgt = g[f"icp_src_{k}"], g[f"icp_tgt_{k}"]
        R, t, it = fs.ICP.get_transformation_ex(src, tgt)
        eR, et = np.abs(R - g["icp_R"][k]).max(), np.abs(t - g["icp_t"][k]).max()
        print(f"icp {shape}: {it} iterations, |R - ref| {eR:.3g}, |t - ref| {et:.3g}")
        worst = [max(worst[0], eR), max(worst[1], et)]
        assert it == orc.icp(src, tgt)[2], shape
        assert eR <= 1e-10, (shape, eR)
        assert et <= 1e-9 * max(1.0, np.abs(g["icp_t"][k]).max()), (shape, et)
    print(f"icp, largest deviation: R {worst[0]:.3g}, t {worst[1]:.3g}")


def test_line_filter_edges(fs, edges):
    _, g = edges
    worst = 0.0
    for k, s in enumerate(g["lf_sigma"]):
        pts, exact = g[f"lf_pts_{k}"], g[f"lf_ld_{k}"]
        got = fs.LineFilter.filter(pts, s)
        assert got.shape == pts.shape
        err = np.abs(got - exact)
        bar = np.maximum(1e-13 + 1e-13 * np.abs(exact), 4.0 * np.abs(g[f"lf_{k}"] - exact).max())
        print(f"line filter n={len(pts)} sigma={s}: |out - exact| {err.max():.3g} (bar {bar.min():.3g})")
        worst = max(worst, err.max())
        assert np.all(err <= bar), (len(pts), s, err.max())
    print(f"line filter, largest deviation: {worst:.3g}")


# ------------------------------------- c. consistency of the entry points ---

def _pairs(edges):
    """(src, tgt) with P = n_tgt in {1, 64, 1024} from the edge fixture, and a
    65-point pair (two waves, one lane of the second)."""
    _, g = edges
    out = []
    for k, (P, nt) in enumerate(edge_cases.ICP_SHAPES):
        if P == nt:
            out.append((g[f"icp_src_{k}"], g[f"icp_tgt_{k}"]))
    assert [len(s) for s, _ in out] == [1, 64, 1024]
    rng = np.random.default_rng(65)
    tgt = rng.normal(0, 4, (65, 2))
    out.append((tgt[rng.permutation(65)] * 1.01 + [0.2, -0.1], tgt))
    return out


def _triples(edges):
    """Three different alignments per point count: [3][P][2] sources, targets."""
    for src, tgt in _pairs(edges):
        yield np.stack([src + 0.01 * j for j in range(3)]), np.stack([np.roll(tgt, j, axis=0) for j in range(3)])


def test_icp_batched_is_three_single_calls(fs, edges):
    for src, tgt in _triples(edges):
        R, t, it = fs.ICP.get_transformation_batched(src, tgt)
        for b in range(3):
            R1, t1, it1 = fs.ICP.get_transformation_ex(src[b], tgt[b])
            assert it[b] == it1, (len(src[b]), b)
            assert np.array_equal(R[b], R1) and np.array_equal(t[b], t1), (len(src[b]), b)


def test_icp_batched_device_buffers(fs, edges):
    """fs2_icp_batched(where=FS2_DEVICE) on torch device buffers: bit-equal to FS2_HOST."""
    import torch
    from fast_slam_2 import _native as nat
    for src, tgt in _triples(edges):
        B, P = src.shape[:2]
        R, t, it = fs.ICP.get_transformation_batched(src, tgt)
        ds, dt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
        dR = torch.full((B, 4), float("nan"), dtype=torch.float64, device="cuda")
        dT = torch.full((B, 2), float("nan"), dtype=torch.float64, device="cuda")
        dI = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        nat.check(nat.load().fs2_icp_batched(0, B, P, C.c_void_p(ds.data_ptr()), C.c_void_p(dt.data_ptr()),
                                             100, 1e-5, C.c_void_p(dR.data_ptr()), C.c_void_p(dT.data_ptr()),
                                             C.c_void_p(dI.data_ptr()), nat.FS2_DEVICE))
        assert np.array_equal(dR.cpu().numpy().reshape(B, 2, 2), R), P
        assert np.array_equal(dT.cpu().numpy(), t), P
        assert np.array_equal(dI.cpu().numpy(), it), P
        # the inputs are left as they were
        assert np.array_equal(ds.cpu().numpy(), src) and np.array_equal(dt.cpu().numpy(), tgt)


def test_icp_submit_is_the_direct_call(fs, edges):
    pairs = _pairs(edges)
    tickets = [fs.ICP.submit(s, t) for s, t in pairs]
    for (s, t), tk in zip(pairs, tickets):
        R, tr, it = tk.result()
        R1, t1, it1 = fs.ICP.get_transformation_ex(s, t)
        assert it == it1 and np.array_equal(R, R1) and np.array_equal(tr, t1), len(s)


def test_icp_point_count_limits(fs):
    """0 and 1025 points are refused by every ICP entry point (FS2_ERR_ARG, before
    anything is launched: the outputs stay untouched); B = 0 is an empty batch."""
    from fast_slam_2 import _native as nat
    lib = nat.load()
    big = np.zeros((1025, 2))
    big[:, 0] = np.arange(1025)
    R, t = np.full(4, 7.0), np.full(2, 7.0)
    it = C.c_int32(-9)
    tk = C.c_int64(-9)
    for ns, ntg in ((0, 5), (5, 0), (1025, 5), (5, 1025), (1025, 1025)):
        assert lib.fs2_icp(0, nat.dptr(big), ns, nat.dptr(big), ntg, 100, 1e-5, nat.dptr(R), nat.dptr(t),
                           C.byref(it)) == nat.FS2_ERR_ARG, (ns, ntg)
        assert lib.fs2_icp_submit(0, nat.dptr(big), ns, nat.dptr(big), ntg, 100, 1e-5,
                                  C.byref(tk)) == nat.FS2_ERR_ARG, (ns, ntg)
    Ib = np.full(1, -9, np.int32)
    for P in (0, 1025):
        assert lib.fs2_icp_batched(0, 1, P, nat.ptr(big), nat.ptr(big), 100, 1e-5, nat.ptr(R), nat.ptr(t),
                                   nat.ptr(Ib), nat.FS2_HOST) == nat.FS2_ERR_ARG, P
    assert lib.fs2_icp_batched(0, 0, 8, nat.ptr(big), nat.ptr(big), 100, 1e-5, nat.ptr(R), nat.ptr(t),
                               nat.ptr(Ib), nat.FS2_HOST) == nat.FS2_OK
    assert np.all(R == 7.0) and np.all(t == 7.0) and it.value == -9 and tk.value == -9 and Ib[0] == -9
    for P in (0, 1025):
        with pytest.raises(ValueError):
            fs.ICP.get_transformation(big[:P], big[:5])
    # no ticket was taken: four submits still fit
    tickets = [fs.ICP.submit(big[:3] * 1.5, big[:4]) for _ in range(4)]
    for k in tickets:
        k.result()


def test_shim_refuses_mismatched_shapes(fs):
    """best_fit_transform pairs the points row by row and get_transformation_batched
    takes one [B][P][2] shape for both: a shorter target is a ValueError (as the
    reference's broadcast error), not a read past its end."""
    rng = np.random.default_rng(5)
    a, b = rng.normal(0, 1, (8, 2)), rng.normal(0, 1, (5, 2))
    for s, t in ((a, b), (b, a), (a, np.zeros((0, 2)))):
        with pytest.raises(ValueError):
            fs.ICP.best_fit_transform(s, t)
    for s, t in ((np.stack([a] * 3), np.stack([b] * 3)), (np.stack([a] * 3), np.stack([a] * 2)),
                 (np.stack([b] * 2), np.stack([a] * 2)), (a, a)):
        with pytest.raises(ValueError):
            fs.ICP.get_transformation_batched(s, t)
    R, t = fs.ICP.best_fit_transform(a, a)
    assert np.allclose(R, np.eye(2), rtol=0, atol=1e-12) and np.allclose(t, 0.0, rtol=0, atol=1e-12)


def test_line_filter_empty(fs):
    out = fs.LineFilter.filter(np.zeros((0, 2)), 0.5)
    assert out.shape == (0, 2) and out.dtype == np.float64


# ------------------------------------------------------ d. the small-N tail ---

def seq_sum(a):
    t = 0.0
    for v in a.tolist():
        t += v
    return t


def check_tail(fs, c, r, k, reduce):
    """One scan without measurements and without motion on weight vector k (as
    tests/test_gpu_exact.py's run_tail): x = the particle index reveals each
    output's source.  Everything bit-exact against the reference's record."""
    N = int(c["w_len"][k])
    w, u0 = c["w"][k, :N], float(c["u0"][k])
    nw, src = r["norm_w"][k, :N], r["src"][k, :N]
    assert src[0] != -2, k                       # the reference did not hang on any of them
    f = fs.FastSLAM2(N, reduce=reduce, verbose=False)
    f.set_state(np.arange(N, dtype=float), np.zeros(N), np.zeros(N), w)
    pose, st = f.step(0.0, 0.0, np.zeros((0, 2)), None, np.zeros(N), u0)
    x, _, _, wg, _, _ = f.get_state()
    f.close()
    tag = (k, N, reduce)
    assert st.error_flags == 0, tag
    assert st.total_weight == seq_sum(w), tag
    assert st.n_eff == r["n_eff"][k], tag
    resample = bool(r["n_eff"][k] < N / 2.0)
    assert bool(st.resampled) == resample, tag
    if resample:
        assert np.array_equal(x.astype(np.int64), src), tag
        assert np.array_equal(wg, nw[src]), tag
        assert pose[0] == float(src[int(np.argmax(nw[src]))]), tag
    else:
        assert np.array_equal(x, np.arange(N, dtype=float)), tag
        assert np.array_equal(wg, nw), tag
        assert pose[0] == float(r["est_x"][k]), tag
    return resample


@pytest.mark.parametrize("kind", range(5), ids=["skewed", "below_floor", "one_nonzero", "ties", "total_below_floor"])
def test_small_n_tail_auto(fs, prim, kind):
    """reduce="auto" (sequential sums at N <= 64) on the 50 recorded weight vectors
    of each kind (gen_ref_primitives.py draws kind k % 5)."""
    c, r = prim
    t0 = time.perf_counter()
    resampled = sum(check_tail(fs, c, r, k, "auto") for k in range(kind, 250, 5))
    print(f"tail kind {kind}: 50 handles, {resampled} resampled, {time.perf_counter() - t0:.2f} s")


def test_small_n_tail_fixture_resamples(prim):
    """From the fixture alone: 142 of the 250 vectors resample, 46 of them with u0
    on a cumulative boundary (k % 3 == 0), and the reference hung on none."""
    c, r = prim
    rs = [k for k in range(250) if r["n_eff"][k] < c["w_len"][k] / 2.0]
    assert len(rs) == 142 and sum(k % 3 == 0 for k in rs) == 46
    assert not np.any(r["src"][:, 0] == -2)


@pytest.mark.parametrize("reduce", ["sequential", "exact"])
def test_small_n_tail_other_modes(fs, prim, reduce):
    c, r = prim
    t0 = time.perf_counter()
    for k in range(50):
        check_tail(fs, c, r, k, reduce)
    print(f"tail {reduce}: 50 handles, {time.perf_counter() - t0:.2f} s")
