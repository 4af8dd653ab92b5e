#!/usr/bin/env python3
"""What the posterior readout on the device (FastSLAM2.pose_moments / pose_density;
csrc/fs2_posterior.hip) costs next to the only route there was before it:
downloading x, y, yaw, w (fs2_get_state) and reducing them with numpy on the host.

For each particle count (default 1e5 and 1e6; the config-3-like cloud of
fs2_synthetic.particle_poses, sigma 0.05 m, with random positive weights), on one GPU:
  (a) pose_moments(): host wall time of the call (it ends with the handle's stream
      drained) and the device time of its two passes (HIP events,
      fs2_debug_posterior_times);
  (b) pose_density((256, 256), weighted) on a fixed 1 cm window: the same two figures
      (weight pass; zeroing + histogram), and the wall time with the window fitted;
  (c) the host route: the download of x, y, yaw, w, then numpy for the same moments
      (two-pass covariance, circular mean) and for the same weighted histogram
      (np.bincount over the flattened cell index).
Wall times are median / min / max of --reps runs after one warm-up.  No ratio is a
target; the file records what one run measured.

  python scripts/posterior_probe.py [--n 100000 1000000] [--reps 5] [--out FILE]
  (profiles/posterior_probe.txt is one run's output)
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fast-slam_amd"))
sys.path.insert(0, REPO)


def _timed(fn, reps, after=None):
    fn()                                            # warm-up
    ms, extra = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
        if after:
            extra.append(after())
    return ms, extra


def _stats(v):
    return f"median {statistics.median(v):9.3f}  min {min(v):9.3f}  max {max(v):9.3f}"


def _host_moments(x, y, yaw, w):
    W = w.sum()
    mx, my = (w * x).sum() / W, (w * y).sum() / W
    myaw = math.atan2((w * np.sin(yaw)).sum(), (w * np.cos(yaw)).sum())
    dt = yaw - myaw
    d = np.stack((x - mx, y - my, dt - 2 * math.pi * np.floor((dt + math.pi) / (2 * math.pi))))
    return np.array([mx, my, myaw]), (w * d) @ d.T / W


def _host_density(x, y, w, x0, y0, cell, nx, ny):
    fx, fy = np.floor((x - x0) / cell), np.floor((y - y0) / cell)
    inside = (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny)
    flat = fy[inside].astype(np.int64) * nx + fx[inside].astype(np.int64)
    return np.bincount(flat, weights=w[inside], minlength=nx * ny).reshape(ny, nx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import build
    import fast_slam_2
    import fs2_synthetic as syn
    from fast_slam_2 import _native as nat
    lib = nat.load()
    lines = [f"scripts/posterior_probe.py on one MI355X, libfs2 build {build.source_id()}: the config-3-like cloud "
             f"(sigma 0.05 m), random positive weights; ms; wall = host wall time of the call, median / min / max of "
             f"{args.reps} runs after one warm-up; device = HIP events around the passes, median of the same runs.",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    dev = (C.c_double * 2)()

    def device_ms():
        lib.fs2_debug_posterior_times(-1, dev)
        return dev[0], dev[1]

    for N in args.n:
        f = fast_slam_2.FastSLAM2(N, rng="device", seed=3, reduce="auto", landmark_capacity=8, verbose=False)
        x, y, yaw = syn.particle_poses(N, 0)
        w = 10.0 ** np.random.default_rng(N).uniform(-6.0, 0.0, N)
        f.set_state(x, y, yaw, w)
        shape, x0, y0, cell = (256, 256), -1.28, -1.28, 0.01
        lib.fs2_debug_posterior_times(1, None)
        t_mom, d_mom = _timed(f.pose_moments, args.reps, device_ms)
        t_den, d_den = _timed(lambda: f.pose_density(shape, (x0, y0), cell, raw=True), args.reps, device_ms)
        lib.fs2_debug_posterior_times(0, None)
        t_fit, _ = _timed(lambda: f.pose_density(shape, raw=True), args.reps)
        med = statistics.median
        lines += [f"N = {N}",
                  f"(a) pose_moments()                 wall {_stats(t_mom)}   device: first pass "
                  f"{med(v[0] for v in d_mom):.4f}, second pass {med(v[1] for v in d_mom):.4f}",
                  f"(b) pose_density(256x256, window)  wall {_stats(t_den)}   device: weight pass "
                  f"{med(v[0] for v in d_den):.4f}, zeroing + histogram {med(v[1] for v in d_den):.4f}",
                  f"    pose_density(256x256, fitted)  wall {_stats(t_fit)}"]
        got = [None]

        def download():
            a = [np.empty(N) for _ in range(4)]
            nat.check(lib.fs2_get_state(f._h, 0, N, *(nat.ptr(v) for v in a), None, None, 0, nat.FS2_HOST), f._h)
            got[0] = a

        t_down, _ = _timed(download, args.reps)
        hx, hy, hyaw, hw = got[0]
        t_hm, _ = _timed(lambda: _host_moments(hx, hy, hyaw, hw), args.reps)
        t_hd, _ = _timed(lambda: _host_density(hx, hy, hw, x0, y0, cell, 256, 256), args.reps)
        pm = f.pose_moments()
        hmean, hcov = _host_moments(hx, hy, hyaw, hw)
        grid, outside, _, _, e = f.pose_density(shape, (x0, y0), cell, raw=True)
        hgrid = _host_density(hx, hy, hw, x0, y0, cell, 256, 256)
        lines += [f"(c) download of x, y, yaw, w       wall {_stats(t_down)}",
                  f"    numpy moments                  wall {_stats(t_hm)}",
                  f"    numpy histogram                wall {_stats(t_hd)}",
                  f"    agreement: max |mean - numpy| {np.abs(pm.mean - hmean).max():.2e}, max |cov - numpy| "
                  f"{np.abs(pm.cov - hcov).max():.2e}, max |grid 2^-e - numpy| "
                  f"{np.abs(np.ldexp(grid.astype(np.float64), -e) - hgrid).max():.2e} (scale_exp {e}, outside {outside})",
                  ""]
        f.close()
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
