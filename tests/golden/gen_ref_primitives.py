#!/usr/bin/env python3
"""Golden fixtures of tests/test_oracle_vs_reference.py: random cases per hot-path
primitive (SURVEY.md §4's build test plan) and what the reference computes on them.

The cases include the edge cases the plan names: ill-conditioned and slightly
asymmetric covariances, weights below the 1e-5 floor, zero weights, exact ties,
resample start points on cumulative-weight boundaries.  The reference runs in a
process of its own (tests/ref_primitives.py: its package is also named
`fast_slam_2`), where the reference is installed; nothing of it is copied, only
its outputs on the seeded inputs are saved.

Run:  python tests/golden/gen_ref_primitives.py
      (writes tests/golden/ref_primitives_cases.npz and ref_primitives_out.npz)
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle import oracle as orc  # noqa: E402

SEED = 20241015


def cases(rng):
    c = {}
    n = 1500
    a, b = rng.normal(0, 5, (n, 2)), rng.normal(0, 5, (n, 2))
    A = rng.normal(0, 1, (n, 2, 2))
    cov = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(2)
    cov[::7] *= 1e-6                                    # tiny / ill-conditioned
    cov[1::11, 0, 1] += rng.normal(0, 1e-2, len(cov[1::11]))   # slightly asymmetric
    c["maha_a"], c["maha_b"], c["maha_cov"] = a, b, cov
    K, Lmax = 300, 40
    lm = np.zeros((K, Lmax, 6))
    lens = rng.integers(0, Lmax + 1, K)
    obs = rng.normal(0, 3, (K, 2))
    for k in range(K):
        L = lens[k]
        lm[k, :L, 0:2] = obs[k] + rng.normal(0, 2.5, (L, 2))
        s = rng.uniform(0.01, 0.5, L)
        lm[k, :L, 2] = lm[k, :L, 5] = s
        lm[k, :L, 3] = lm[k, :L, 4] = rng.normal(0, 0.3, L) * s
    c["as_obs"], c["as_lm"], c["as_len"] = obs, lm, lens
    c["as_gate"] = rng.choice([8.0, 2.0, 0.5, 20.0], K)
    W, Nmax = 250, 64
    w = np.zeros((W, Nmax))
    wl = rng.integers(1, Nmax + 1, W)
    u0 = np.zeros(W)
    for k in range(W):
        N = wl[k]
        kind = k % 5
        if kind == 0:
            v = rng.random(N) ** 8
        elif kind == 1:
            v = np.where(rng.random(N) < 0.5, rng.random(N) * 1e-6, rng.random(N))   # below the floor
        elif kind == 2:
            v = np.zeros(N)
            v[rng.integers(0, N)] = rng.random()
        elif kind == 3:
            v = np.full(N, 1.0 / N)                                               # exact ties
        else:
            v = rng.random(N) * 1e-7                                              # total < 1e-5
        w[k, :N] = v
        nv = orc.normalize(v)
        cs = np.cumsum(nv)
        # u0 in (0, 1/N) or on a cumulative boundary reachable from it
        u0[k] = rng.uniform(0, 1.0 / N) if k % 3 else max(0.0, min(cs[0] % (1.0 / N), np.nextafter(1.0 / N, 0)))
    c["w"], c["w_len"], c["u0"] = w, wl, u0
    B, P = 60, 50
    src = rng.normal(0, 3, (B, P, 2))
    th = rng.uniform(-np.pi, np.pi, B)
    Rm = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], -2)
    tgt = np.einsum("bij,bpj->bpi", Rm, src) + rng.normal(0, 2, (B, 1, 2)) + rng.normal(0, 0.01, (B, P, 2))
    c["bf_src"], c["bf_tgt"] = src, tgt
    I, Q = 12, 120
    base = rng.normal(0, 4, (I, Q, 2))
    ang = rng.uniform(-0.2, 0.2, I)
    Ri = np.stack([np.stack([np.cos(ang), -np.sin(ang)], -1), np.stack([np.sin(ang), np.cos(ang)], -1)], -2)
    c["icp_src"] = base
    c["icp_tgt"] = np.einsum("bij,bpj->bpi", Ri, base) + rng.normal(0, 0.3, (I, 1, 2))
    F = 40
    c["lf_pts"] = rng.normal(0, 3, (F, 90, 2))
    c["lf_sigma"] = rng.choice([0.1, 0.3, 0.5, 1.0, 2.5], F)
    return c


def main():
    cpath = os.path.join(HERE, "ref_primitives_cases.npz")
    opath = os.path.join(HERE, "ref_primitives_out.npz")
    np.savez_compressed(cpath, **cases(np.random.default_rng(SEED)))
    tmp = opath + ".raw.npz"
    subprocess.run([sys.executable, os.path.join(REPO, "tests", "ref_primitives.py"), cpath, tmp], check=True)
    out = dict(np.load(tmp))
    os.remove(tmp)
    np.savez_compressed(opath, **out)
    for p in (cpath, opath):
        print(p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
