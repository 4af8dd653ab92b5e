#!/usr/bin/env python3
"""What the map readout on the device (FastSLAM2.map_summary / map_density;
csrc/fs2_mapreadout.hip) costs, next to the route there was before it:
get_state()'s dense [N][cap][6] maps and np.add.at on the host.

For each shape (default BASELINE config 2, 1e5 x 200, and config 3, 1e6 x 500), on one GPU:
the synthetic maps of bench.py's populate, then scans of fs2_synthetic.scan_measurements
until one has resampled (and --more scans after it, so that siblings have appended into
shared pages), then on that state:
  (a) map_summary(): host wall time of the call and the device time of its three stages
      (HIP events, fs2_debug_map_times): the counts of cnt, the tally, the summary pass;
      T, R, U and U / R;
  (b) map_density((256, 256)) weighted, on the window fitted once to the summary's box:
      the same figures (weight pass + counts; tally; zeroing + bin pass), and the wall
      time with the window fitted by the call;
  (c) the host route (--host-limit: shapes of at most that many landmarks; config 3's
      download is 24 GB): get_state(), then the same weighted histogram with np.add.at,
      compared with (b)'s grid bit for bit; the ratio (c) / (b).
cluster_landmarks' gather stage is not timed: it has no hook and its first step from
outside (fs2_update_known_landmarks) sorts and clusters as well.

Two A/Bs, each the same run on a variant library named by FS2_LIB (--no-host skips (c),
--append adds the run to the file instead of replacing it):
  `python fast-slam_amd/build.py --variant mapdirect -DFS2_MAP_BIN_DIRECT=1`: the bin pass
      on plain global atomics, without the LDS table;
  `python fast-slam_amd/build.py --variant maptally -DFS2_MAP_TALLY_PER_ENTRY=1`: the tally
      with one atomic per shared entry, without the sum over runs of equal page ids.
Wall times are median / min / max of --reps runs after one warm-up.

  python scripts/map_probe.py [--shapes 100000x200 1000000x500] [--reps 5] [--out FILE] [--append]
  (writes profiles/map_probe.txt unless --out names another file; the committed file is
  three runs: libfs2.so, then the two variants appended)
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
    return f"median {statistics.median(v):10.3f}  min {min(v):10.3f}  max {max(v):10.3f}"


def _host_density(state, e, x0, y0, cell, nx, ny):
    w, cnt, lm = state[3], state[4], state[5]
    q = np.rint(np.ldexp(w, e)).astype(np.uint64)
    live = np.arange(lm.shape[1])[None, :] < cnt[:, None]
    pi = np.broadcast_to(np.arange(len(cnt))[:, None], live.shape)[live]
    fx, fy = np.floor((lm[:, :, 0][live] - x0) / cell), np.floor((lm[:, :, 1][live] - y0) / cell)
    inside = (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny)
    grid = np.zeros((ny, nx), dtype=np.uint64)
    np.add.at(grid, (fy[inside].astype(np.int64), fx[inside].astype(np.int64)), q[pi][inside])
    return grid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["100000x200", "1000000x500"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--more", type=int, default=2, help="scans after the first resample")
    ap.add_argument("--max-scans", type=int, default=40)
    ap.add_argument("--host-limit", type=int, default=50_000_000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "map_probe.txt"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()

    import torch
    import bench
    import build
    import fast_slam_2
    import fs2_synthetic as syn
    from fast_slam_2 import _native as nat
    from fast_slam_2.algorithms.fast_slam_2 import fit_density_window
    lib = nat.load()
    lines = [f"scripts/map_probe.py on one GPU, libfs2 build {build.source_id()} ({os.path.basename(nat.LIB_PATH)}): "
             f"filter-built maps after a resample; ms; wall = host wall time of the call, median / min / max of "
             f"{args.reps} runs after one warm-up; device = HIP events around the stages, median of the same runs.",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    dev = (C.c_double * 3)()
    med = statistics.median

    def device_ms():
        lib.fs2_debug_map_times(-1, dev)
        return dev[0], dev[1], dev[2]

    for shape_s in args.shapes:
        N, L = (int(v) for v in shape_s.split("x"))
        f = fast_slam_2.FastSLAM2(N, rng="device", seed=3, reduce="auto", landmark_capacity=L + args.max_scans + 8,
                                  verbose=False)
        bench.populate(f, N, L, 0, 0)
        scans, after = 0, None
        while scans < args.max_scans and (after is None or after < args.more):
            _, st = f.step(*syn.odometry(scans), np.ascontiguousarray(syn.scan_measurements(L, scans, 0)))
            scans += 1
            if after is not None:
                after += 1
            elif st.resampled:
                after = 0
        ms0 = f.map_summary()
        shape = (256, 256)
        (x0, y0), cell = fit_density_window(ms0.bbox, shape)
        lib.fs2_debug_map_times(1, None)
        t_sum, d_sum = _timed(f.map_summary, args.reps, device_ms)
        t_den, d_den = _timed(lambda: f.map_density(shape, (x0, y0), cell, raw=True), args.reps, device_ms)
        lib.fs2_debug_map_times(0, None)
        t_fit, _ = _timed(lambda: f.map_density(shape, raw=True), args.reps)
        grid, outside, _, _, e = f.map_density(shape, (x0, y0), cell, raw=True)
        lines += [f"N = {N}, L = {L}: {scans} scans, first resample {'none' if after is None else scans - after}; "
                  f"pool {int(st.pool_pages)} pages",
                  f"    T = {ms0.landmarks}, R = {ms0.page_refs}, U = {ms0.pages}, U / R = {ms0.pages / max(ms0.page_refs, 1):.4f}, "
                  f"max count {ms0.max_count}",
                  f"(a) map_summary()                  wall {_stats(t_sum)}   device: counts "
                  f"{med(v[0] for v in d_sum):.4f}, tally {med(v[1] for v in d_sum):.4f}, summary pass "
                  f"{med(v[2] for v in d_sum):.4f}",
                  f"(b) map_density(256x256, window)   wall {_stats(t_den)}   device: weight pass + counts "
                  f"{med(v[0] for v in d_den):.4f}, tally {med(v[1] for v in d_den):.4f}, zeroing + bin pass "
                  f"{med(v[2] for v in d_den):.4f}",
                  f"    map_density(256x256, fitted)   wall {_stats(t_fit)}",
                  f"    grid: {np.count_nonzero(grid)} nonzero cells, outside {outside}, scale_exp {e}"]
        if not args.no_host and N * L <= args.host_limit:
            got = [None]

            def download():
                got[0] = f.get_state()

            t_down, _ = _timed(download, min(args.reps, 3))
            t_add, _ = _timed(lambda: _host_density(got[0], e, x0, y0, cell, 256, 256), min(args.reps, 3))
            same = np.array_equal(_host_density(got[0], e, x0, y0, cell, 256, 256), grid)
            host = med(t_down) + med(t_add)
            lines += [f"(c) get_state()                    wall {_stats(t_down)}",
                      f"    np.add.at histogram            wall {_stats(t_add)}",
                      f"    host route / map_density (medians): {host:.1f} / {med(t_den):.3f} = {host / med(t_den):.0f}x; "
                      f"grids equal bit for bit: {same}"]
        lines.append("")
        f.close()
    text = "\n".join(lines)
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as fh:
        fh.write(("\n" if args.append else "") + text)


if __name__ == "__main__":
    main()
