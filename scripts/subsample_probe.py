#!/usr/bin/env python3
"""What the weighted subsample on the device (FastSLAM2.subsample; csrc/fs2_subsample.hip,
DESIGN.md §16) costs next to the only route there was before it: downloading the weights
and poses (fs2_get_state) and resampling on the host with numpy.

For each particle count (default 1e5 and 1e6; the config-3-like cloud of
fs2_synthetic.particle_poses with random positive weights over six decades) and for
k = 500 and k = N, on one GPU:
  (a) subsample(k): host wall time of the call (it ends with the handle's stream drained
      and idx, x, y, yaw, w, counts on the host) and the device time of its stages (HIP
      events, fs2_debug_subsample_times): scan -- the weight pass, the read-back of the
      largest weight and the three kernels of the prefix sum --, select, gather;
      the same for weighted=False (no scan);
  (b) the host route: the download of x, y, yaw, w, cnt, then the same integer draw with
      numpy (np.rint(np.ldexp), np.cumsum, the thresholds, np.searchsorted) and the fancy
      indexing of the five arrays.
The arrays of both routes are asserted equal.  Wall times are median / min / max of
--reps runs after one warm-up.  No ratio is a target; the file records what one run
measured.  FS2_LIB selects another build of the library (an A/B variant).

  python scripts/subsample_probe.py [--n 100000 1000000] [--reps 5] [--out FILE]
  (profiles/subsample_probe.txt is one run's output)
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fast-slam_amd"))
sys.path.insert(0, REPO)

OFFSET = 1 << 31


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


def _host_draw(w, e, k):
    """idx by the definition of fs2.h; the thresholds in uint64 through the same split the
    library uses when j Q would not fit (Python integers for 1e6 outputs would time the
    interpreter, not numpy)."""
    q = np.rint(np.ldexp(w, e)).astype(np.uint64)
    cum = np.cumsum(q, dtype=np.uint64)
    Q = int(cum[-1])
    s = (OFFSET * Q) >> 32
    a, b = divmod(Q, k)
    a_s, b_s = divmod(s, k)
    j = np.arange(k, dtype=np.uint64)
    t = j * np.uint64(a) + np.uint64(a_s) + (j * np.uint64(b) + np.uint64(b_s)) // np.uint64(k)
    return np.searchsorted(cum, t, side="right"), Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import fast_slam_2
    import fs2_synthetic as syn
    from fast_slam_2 import _native as nat
    lib = nat.load()
    lines = [f"scripts/subsample_probe.py on one MI355X, libfs2 build {lib.fs2_build_id().decode()} "
             f"({os.path.basename(nat.LIB_PATH)}): the config-3-like cloud, random positive weights over six decades, "
             f"offset 2^31; ms; wall = host wall time of the call, median / min / max of {args.reps} runs after one "
             f"warm-up; device = HIP events around the stages, median of the same runs.",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    dev = (C.c_double * 3)()
    med = statistics.median

    def device_ms():
        lib.fs2_debug_subsample_times(-1, dev)
        return dev[0], dev[1], dev[2]

    for N in args.n:
        f = fast_slam_2.FastSLAM2(N, rng="device", seed=3, reduce="auto", landmark_capacity=8, verbose=False)
        x, y, yaw = syn.particle_poses(N, 0)
        w = 10.0 ** np.random.default_rng(N).uniform(-6.0, 0.0, N)
        f.set_state(x, y, yaw, w)
        got = [None]

        def download():
            a = [np.empty(N) for _ in range(4)] + [np.empty(N, dtype=np.int32)]
            nat.check(lib.fs2_get_state(f._h, 0, N, *(nat.ptr(v) for v in a), None, 0, nat.FS2_HOST), f._h)
            got[0] = a

        t_down, _ = _timed(download, args.reps)
        lines += [f"N = {N}", f"    download of x, y, yaw, w, cnt         wall {_stats(t_down)}"]
        for k in (500, N):
            lib.fs2_debug_subsample_times(1, None)
            t_w, d_w = _timed(lambda: f.subsample(k), args.reps, device_ms)
            t_u, d_u = _timed(lambda: f.subsample(k, weighted=False), args.reps, device_ms)
            lib.fs2_debug_subsample_times(0, None)
            sub = f.subsample(k)
            hx, hy, hyaw, hw, hcnt = got[0]
            t_draw, _ = _timed(lambda: _host_draw(hw, sub.scale_exp, k), args.reps)
            hidx, Q = _host_draw(hw, sub.scale_exp, k)
            t_take, _ = _timed(lambda: [v[hidx] for v in got[0]], args.reps)
            assert Q == sub.total and np.array_equal(hidx, sub.idx)
            for dv, hv in ((sub.x, hx), (sub.y, hy), (sub.yaw, hyaw), (sub.w, hw), (sub.counts, hcnt)):
                assert np.array_equal(dv, hv[hidx])
            host = med(t_down) + med(t_draw) + med(t_take)
            lines += [f"  k = {k}",
                      f"(a) subsample(k)                          wall {_stats(t_w)}   device: scan "
                      f"{med(v[0] for v in d_w):.4f}, select {med(v[1] for v in d_w):.4f}, gather "
                      f"{med(v[2] for v in d_w):.4f}",
                      f"    subsample(k, weighted=False)          wall {_stats(t_u)}   device: scan "
                      f"{med(v[0] for v in d_u):.4f}, select {med(v[1] for v in d_u):.4f}, gather "
                      f"{med(v[2] for v in d_u):.4f}",
                      f"(b) numpy rint, cumsum, searchsorted      wall {_stats(t_draw)}",
                      f"    numpy fancy indexing of five arrays   wall {_stats(t_take)}",
                      f"    host route, download + draw + indexing (medians): {host:.3f}; device route / host route = "
                      f"{med(t_w) / host:.3f}; arrays equal (scale_exp {sub.scale_exp}, total {sub.total})"]
        lines.append("")
        f.close()
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
