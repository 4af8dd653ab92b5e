#!/usr/bin/env python3
"""Golden fixtures of tests/test_oracle_edges.py and tests/test_gpu_primitives.py:
the stand-alone primitives at the shape edges of their kernels
(fast-slam_amd/csrc/fs2_geometry.hip), and what the reference computes there.

  association  L in {1, 63, 64, 65, 127, 128, 129, 200} (k_associate walks 64
               landmarks per trip): the first match at 0, 63, 64, 127, 128 and
               L - 1, further matches after it, no match at all, and singular
               covariances (the zero matrix and [[1, 2], [2, 4]]) before and
               after the first match, in its chunk of 64 and in another one.
               The reference raises numpy.linalg.LinAlgError at a singular
               covariance it reaches: recorded as -2.
  best fit     n in {1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049} (k_best_fit
               strides by 1024), angles over (-pi, pi), one next to pi.
  ICP          (P, n_tgt) from (1, 1) to (1024, 1024), P != n_tgt included.
  line filter  n in {1, 2, 3, 127, 128, 129, 300} x sigma in {0.1, 0.5, 2.5, 8.0}
               (radius up to 32: many times n, reflect_idx's repeated reflection).

Best fit and line filter also get a numpy.longdouble evaluation of the same
closed form (`bf_R_ld`, `bf_t_ld`, `lf_ld_<k>`, rounded to float64 once at the
end), which tells how far the reference's own float64 result is from the exact
one.  The reference runs in a process of its own (tests/ref_primitives.py
--ragged), where it is installed; nothing of it is copied, only its outputs on
the seeded inputs are saved.  Before anything is written the C oracle must
agree with the reference on every case within the bars of
tests/test_oracle_vs_reference.py.

Run:  python tests/golden/gen_ref_edges.py
      (writes tests/golden/ref_edges_assoc.npz and ref_edges_geom.npz)
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle import oracle as orc  # noqa: E402

SEED = 20261019
MAX_BYTES = 512 * 1024

AS_LENS = (1, 63, 64, 65, 127, 128, 129, 200)
AS_FIRST = (0, 63, 64, 127, 128)
AS_GATES = (0.5, 2.0, 8.0)
SINGULAR = (np.zeros(4), np.array([1.0, 2.0, 2.0, 4.0]))
BF_N = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049)
ICP_SHAPES = ((1, 1), (1, 1024), (2, 3), (63, 64), (64, 64), (65, 63), (129, 1000), (1024, 7),
              (1024, 1024))
LF_N = (1, 2, 3, 127, 128, 129, 300)
LF_SIGMA = (0.1, 0.5, 2.5, 8.0)


# ------------------------------------------------------------ association ---

def maha_ld(obs, row):
    """sqrt(delta^T inv(cov) delta) in long double (None: singular)."""
    ld = np.longdouble
    a, b, c, d = (ld(v) for v in row[2:6])
    det = a * d - b * c
    if det == 0:
        return None
    dx, dy = ld(obs[0]) - ld(row[0]), ld(obs[1]) - ld(row[1])
    q = (d * dx * dx - (b + c) * dx * dy + a * dy * dy) / det
    return np.sqrt(q)


def landmark(rng, obs, gate, match):
    """A landmark whose Mahalanobis distance to obs is 0.2..0.8 (match) or
    1.3..3 (no match) times the gate; well-conditioned covariance."""
    s = rng.uniform(0.01, 0.25)
    off = float(np.clip(rng.normal(0, 0.3), -0.6, 0.6)) * s      # positive definite: det >= 0.34 s^2
    cov = np.array([s * rng.uniform(0.7, 1.4), off, off, s])
    A = cov.reshape(2, 2)
    th = rng.uniform(0, 2 * np.pi)
    u = np.array([np.cos(th), np.sin(th)])
    unit = np.sqrt(u @ np.linalg.inv(A) @ u)             # Mahalanobis length of the unit step
    f = rng.uniform(0.2, 0.8) if match else rng.uniform(1.3, 3.0)
    return np.concatenate([obs - u * (f * gate / unit), cov])


def expected_assoc(obs, lm, gate):
    """First event in list order from the long-double distances; asserts the
    fixture's condition |sqrt(q) - gate| > 1e-9 gate up to and including it."""
    for j, row in enumerate(lm):
        dist = maha_ld(obs, row)
        if dist is None:
            return -2
        assert abs(dist - np.longdouble(gate)) > np.longdouble(1e-9) * np.longdouble(gate), (j, dist)
        if dist < gate:
            return j
    return -1


def assoc_case(rng, L, gate, matches=(), singular=()):
    """L landmarks around a random observation: matches at `matches`, singular
    covariances (index, kind) at `singular`, no match anywhere else."""
    obs = rng.normal(0, 3, 2)
    lm = np.stack([landmark(rng, obs, gate, j in matches) for j in range(L)])
    # values a float32 holds (as float64): the fixture compresses to half the size,
    # and the distances move by 1e-7 of themselves, far inside the 0.8 / 1.3 margins
    lm = lm.astype(np.float32).astype(np.float64)
    for j, kind in singular:
        lm[j, 2:6] = SINGULAR[kind]
    return obs, lm


def assoc_cases(rng):
    """[(obs, lm, gate, expected)].  The gates take turns over the cases of a
    length, so every length meets every gate."""
    out = []
    turn = [0]

    def add(L, matches=(), singular=(), want=None):
        gate = AS_GATES[turn[0] % 3]
        turn[0] += 1
        obs, lm = assoc_case(rng, L, gate, matches, singular)
        exp = expected_assoc(obs, lm, gate)      # asserts the band condition; a failure: redraw (new SEED)
        assert exp == want, (L, matches, singular, exp, want)
        out.append((obs, lm, gate, exp))

    for L in AS_LENS:
        later = lambda f: sorted({j for j in (f + 1, f + 2, (f // 64) * 64 + 63, f + 64, L - 1) if f < j < L})  # noqa: E731
        for f in sorted({p for p in AS_FIRST + (L - 1,) if p < L}):
            add(L, [f] + later(f), want=f)
        add(L, want=-1)
        if L > 64:
            add(L, [63, 64], want=63)            # last lane of chunk 0 before lane 0 of chunk 1
        if L > 130:
            add(L, [70, 130], want=70)           # chunk 1 before a lower lane of chunk 2
        last = (L - 1) // 64 * 64                # first index of the last chunk
        for kind in (0, 1):
            if L == 1:
                add(L, singular=[(0, kind)], want=-2)
                continue
            # same chunk: the singular one after / before the match
            add(L, [0], [(min(63, L - 1), kind)], want=0)
            add(L, [min(63, L - 1)], [(0, kind)], want=-2)
            if 0 < last < L - 1:
                add(L, [last, L - 1], [(last + 1, kind)], want=last)
                add(L, [L - 1], [(last, kind)], want=-2)
            if L > 64:
                # another chunk: the singular one in a later / an earlier chunk
                add(L, [63], [(64, kind), (L - 1, kind)], want=63)
                add(L, [5], [(last, kind)], want=5)
                add(L, [64], [(63, kind)], want=-2)
                add(L, [L - 1], [(0, kind)], want=-2)
                add(L, [], [(L - 1, kind)], want=-2)          # no match at all before it
    return out


# ---------------------------------------------------------- best fit, ICP ---

def rot(th):
    return np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])


def best_fit_cases(rng):
    # angles spread over (-pi, pi); one within 1e-3 of pi
    ang = np.linspace(-3.0, 3.0, len(BF_N))
    ang[3] = np.pi - 4e-4
    ang[6] = -np.pi + 7e-4
    out = []
    for n, th in zip(BF_N, ang):
        src = rng.normal(0, 3, (n, 2))
        tgt = src @ rot(th).T + rng.normal(0, 2, (1, 2)) + rng.normal(0, 0.01, (n, 2))
        out.append((src, tgt))
    return out


def best_fit_ld(src, tgt):
    """best_fit_transform's closed form (centroids, cross-covariance, the 2-D
    Kabsch angle) in long double, rounded to float64 at the end."""
    ld = np.longdouble
    s, t = src.astype(ld), tgt.astype(ld)
    n = ld(len(s))
    cs, ct = s.sum(0) / n, t.sum(0) / n
    a, b = s - cs, t - ct
    h00, h01 = (a[:, 0] * b[:, 0]).sum(), (a[:, 0] * b[:, 1]).sum()
    h10, h11 = (a[:, 1] * b[:, 0]).sum(), (a[:, 1] * b[:, 1]).sum()
    th = np.arctan2(h01 - h10, h00 + h11)
    c, sn = np.cos(th), np.sin(th)
    R = np.array([[c, -sn], [sn, c]], dtype=ld)
    tr = ct - R @ cs
    return R.astype(np.float64), tr.astype(np.float64)


def icp_cases(rng):
    out = []
    for P, nt in ICP_SHAPES:
        tgt = rng.normal(0, 4, (nt, 2))
        # KD-tree ties are not index-ordered: no duplicated target points
        assert len(np.unique(tgt, axis=0)) == nt
        pick = rng.permutation(nt)[:P] if P <= nt else rng.integers(0, nt, P)
        th = rng.uniform(-0.2, 0.2)
        # the source moved by the inverse: aligning it to the target finds (R(th), shift)
        shift = rng.normal(0, 0.3, 2)
        src = (tgt[pick] + rng.normal(0, 0.01, (P, 2)) - shift) @ rot(th)
        out.append((src, tgt))
    return out


# ------------------------------------------------------------ line filter ---

def line_filter_cases(rng):
    return [(rng.normal(0, 3, (n, 2)), s) for n in LF_N for s in LF_SIGMA]


def line_filter_ld(pts, sigma):
    """scipy's gaussian_filter1d(mode="reflect") as a symmetric pad and a dot
    product in long double; the taps are the float64 ones scipy builds."""
    w, r = orc.gaussian_weights(sigma)
    w = w.astype(np.longdouble)
    n = len(pts)
    out = np.empty((n, 2))
    for col in range(2):
        pad = np.pad(pts[:, col].astype(np.longdouble), r, mode="symmetric")
        out[:, col] = [np.dot(w, pad[i:i + 2 * r + 1]) for i in range(n)]
    return out


# ------------------------------------------------------------------ main ---

def main():
    rng = np.random.default_rng(SEED)
    asc = assoc_cases(rng)
    bf = best_fit_cases(rng)
    icp = icp_cases(rng)
    lf = line_filter_cases(rng)

    cases = {"as_obs": np.array([c[0] for c in asc]), "as_gate": np.array([c[2] for c in asc]),
             "bf_n": np.array(len(bf)), "icp_n": np.array(len(icp)),
             "lf_sigma": np.array([c[1] for c in lf])}
    for k, c in enumerate(asc):
        cases[f"as_lm_{k}"] = c[1]
    for k, (s, t) in enumerate(bf):
        cases[f"bf_src_{k}"], cases[f"bf_tgt_{k}"] = s, t
    for k, (s, t) in enumerate(icp):
        cases[f"icp_src_{k}"], cases[f"icp_tgt_{k}"] = s, t
    for k, (p, _) in enumerate(lf):
        cases[f"lf_pts_{k}"] = p

    with tempfile.TemporaryDirectory() as tmp:
        cpath, opath = os.path.join(tmp, "cases.npz"), os.path.join(tmp, "out.npz")
        np.savez(cpath, **cases)
        subprocess.run([sys.executable, os.path.join(REPO, "tests", "ref_primitives.py"), "--ragged",
                        cpath, opath], check=True)
        ref = dict(np.load(opath))

    # The C oracle agrees with the reference on every case within the project's
    # bars (tests/test_oracle_vs_reference.py).  A case that fails here is
    # ill-conditioned input, not a finding: change SEED and say so.  (None had to
    # be redrawn for the seed above.)
    worst = {"bf_R": 0.0, "bf_t": 0.0, "icp_R": 0.0, "icp_t": 0.0, "lf": 0.0}
    for k, (obs, lm, gate, exp) in enumerate(asc):
        assert ref["assoc"][k] == exp, (k, ref["assoc"][k], exp)       # the long-double prediction
        assert orc.associate(obs, lm, gate) == ref["assoc"][k], k
    for k, (s, t) in enumerate(bf):
        R, tr = orc.best_fit(s, t)
        worst["bf_R"] = max(worst["bf_R"], np.abs(R - ref["bf_R"][k]).max())
        worst["bf_t"] = max(worst["bf_t"], np.abs(tr - ref["bf_t"][k]).max())
        assert np.allclose(R, ref["bf_R"][k], atol=1e-12) and np.allclose(tr, ref["bf_t"][k], atol=1e-11), k
    iters = []
    for k, (s, t) in enumerate(icp):
        R, tr, it = orc.icp(s, t)
        iters.append(it)
        worst["icp_R"] = max(worst["icp_R"], np.abs(R - ref["icp_R"][k]).max())
        worst["icp_t"] = max(worst["icp_t"], np.abs(tr - ref["icp_t"][k]).max())
        assert np.allclose(R, ref["icp_R"][k], atol=1e-10) and np.allclose(tr, ref["icp_t"][k], atol=1e-9), k
    for k, (p, s) in enumerate(lf):
        got = orc.line_filter(p, s)
        worst["lf"] = max(worst["lf"], np.abs(got - ref[f"lf_{k}"]).max())
        assert np.allclose(got, ref[f"lf_{k}"], rtol=1e-13, atol=1e-13), k
    print("oracle vs reference, largest difference:", worst, "ICP iterations:", iters)

    ld = [best_fit_ld(s, t) for s, t in bf]
    assoc_file = {"as_obs": cases["as_obs"], "as_gate": cases["as_gate"], "assoc": ref["assoc"]}
    assoc_file.update({k: v for k, v in cases.items() if k.startswith("as_lm_")})
    geom_file = {k: v for k, v in cases.items() if not k.startswith("as_")}
    geom_file.update({k: v for k, v in ref.items() if k != "assoc"})
    geom_file["bf_R_ld"] = np.array([r for r, _ in ld])
    geom_file["bf_t_ld"] = np.array([t for _, t in ld])
    for k, (p, s) in enumerate(lf):
        geom_file[f"lf_ld_{k}"] = line_filter_ld(p, s)
    for name, content in (("ref_edges_assoc.npz", assoc_file), ("ref_edges_geom.npz", geom_file)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **content)
        size = os.path.getsize(path)
        print(path, size, "bytes;", len(content), "arrays")
        assert size < MAX_BYTES, (name, size)
    print("cases:", len(asc), "associations,", len(bf), "best fits,", len(icp), "ICPs,", len(lf), "line filters")


if __name__ == "__main__":
    main()
