#!/usr/bin/env python3
"""What a compact snapshot (FastSLAM2.snapshot / restore; csrc/fs2_snapshot.hip) costs
next to the dense path (get_state / set_state) on the same handle, on one GPU.

At config 2's shape (1e5 particles x 200 landmarks, the synthetic workload of
fs2_synthetic / bench.populate, rng="device"), after enough scans that resamples have
shared pages:
  (a) the snapshot's bytes against the dense maps' N * cap * 48 (cap = the longest map),
  (b) its distinct pages against the page-table entries sum(ceil(cnt / 8)), its records
      against the slots sum(cnt),
  (c) host wall time of snapshot() against get_state(), and of restore() against
      set_state(), median / min / max of --reps runs after one warm-up (every call
      ends with the handle's stream drained, so wall time covers the device work),
  (d) that the restored state equals the saved one.
set_state runs last: it gives every particle private pages again.

With --select-out, on the same handle and by the same method (before the restores):
snapshot(select=idx) for the identity, every 10th particle, the first half and one
particle -- bytes, pages, records, time -- each next to restore() into a handle of m
particles and to the dense route for the same selection (get_state + numpy indexing +
set_state into that handle).

  python scripts/snapshot_probe.py [--n 100000] [--l 200] [--scans 10] [--out FILE] [--select-out FILE]
  (profiles/snapshot_probe.txt and profiles/snapshot_select_probe.txt are one run's output)
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "fast-slam_amd"))
sys.path.insert(0, REPO)


def _timed(fn, reps):
    fn()                                            # warm-up
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def _stats(v):
    return f"median {statistics.median(v):10.3f}  min {min(v):10.3f}  max {max(v):10.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--l", type=int, default=200)
    ap.add_argument("--scans", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--select-out", default=None)
    args = ap.parse_args()

    import torch
    import bench
    import fast_slam_2
    import fs2_synthetic as syn
    N, L = args.n, args.l
    f = fast_slam_2.FastSLAM2(N, rng="device", seed=3, reduce="auto", landmark_capacity=L + 4 * args.scans + 8,
                              verbose=False)
    bench.populate(f, N, L, 0, 0)
    resamples = 0
    for s in range(args.scans):
        _, st = f.step(*syn.odometry(s), np.ascontiguousarray(syn.scan_measurements(L, s, 0)))
        resamples += st.resampled
    lines = [f"scripts/snapshot_probe.py on one MI355X: N = {N} particles x {L} landmarks, {args.scans} scans "
             f"({resamples} resampled), rng=\"device\"; wall ms, median / min / max of {args.reps} runs after one "
             f"warm-up.",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    state = f.get_state()
    cnt = state[4]
    snap = f.snapshot()
    info = f.snapshot_info(snap)
    cap = int(cnt.max())
    dense = N * cap * 48
    entries, slots = int(((cnt + 7) // 8).sum()), int(cnt.sum())
    lines += [f"(a) snapshot {snap.size} bytes; dense maps N * cap * 48 = {dense} bytes (cap {cap}): "
              f"{dense / snap.size:.2f}x the snapshot",
              f"(b) pages {info['pages']} of {entries} page-table entries ({info['pages'] / entries:.3f}); "
              f"records {info['records']} of {slots} slots ({info['records'] / slots:.3f}); rows {info['rows']}"]
    t_snap = _timed(f.snapshot, args.reps)
    t_get = _timed(f.get_state, args.reps)
    lines += [f"(c) snapshot()   [ms]  {_stats(t_snap)}",
              f"    get_state()  [ms]  {_stats(t_get)}   ratio of medians "
              f"{statistics.median(t_get) / statistics.median(t_snap):.2f}"]
    if args.select_out:
        _write(args.select_out, _selections(f, fast_slam_2, args, state, snap, t_snap, resamples,
                                            torch.cuda.get_device_name(0)))
    t_restore = _timed(lambda: f.restore(snap), args.reps)
    same = all(np.array_equal(u, v) for u, v in zip(f.get_state(), state))
    after = f.snapshot_info(f.snapshot())
    t_set = _timed(lambda: f.set_state(*state), args.reps)
    lines += [f"    restore()    [ms]  {_stats(t_restore)}",
              f"    set_state()  [ms]  {_stats(t_set)}   ratio of medians "
              f"{statistics.median(t_set) / statistics.median(t_restore):.2f}",
              f"(d) restored state equals the saved one: {same}; pages after restore {after['pages']}, after "
              f"set_state {f.snapshot_info(f.snapshot())['pages']}"]
    f.close()
    _write(args.out, lines)


def _write(path, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(text)


def _selections(f, fast_slam_2, args, state, snap, t_snap, resamples, device):
    """snapshot(select=idx) against the dense route for the same selection on the same
    handle (get_state + numpy indexing + set_state into a handle of m particles), for the
    identity, every 10th particle and the first half; one particle shows what a save
    costs before anything scales with m (the passes over the pools)."""
    N, L = args.n, args.l
    med = statistics.median
    full = f.snapshot_info(snap)
    lines = [f"scripts/snapshot_probe.py --select-out on one MI355X: N = {N} particles x {L} landmarks, {args.scans} "
             f"scans ({resamples} resampled), rng=\"device\"; wall ms, median / min / max of {args.reps} runs after "
             f"one warm-up, every call ending with the handle's stream drained.",
             f"device: {device}", "",
             f"full snapshot(): {snap.size} bytes, pages {full['pages']}, records {full['records']}, rows "
             f"{full['rows']};  [ms] {_stats(t_snap)}", ""]
    cases = [("identity", np.arange(N)), ("every 10th", np.arange(0, N, 10)), ("first half", np.arange(N // 2)),
             ("one particle", np.array([N // 2]))]
    for name, idx in cases:
        m = idx.size
        g = fast_slam_2.FastSLAM2(m, rng="device", seed=3, reduce="auto",
                                  landmark_capacity=L + 4 * args.scans + 8, verbose=False)

        def dense():
            st = f.get_state()
            g.set_state(*(a[idx] for a in st))

        t_sel = _timed(lambda: f.snapshot(select=idx), args.reps)
        sel = f.snapshot(select=idx)
        info = f.snapshot_info(sel)
        t_res = _timed(lambda: g.restore(sel), args.reps)
        want = tuple(a[idx] for a in state)
        cap = max(int(want[4].max()), 1)
        got = g.get_state()
        same = all(np.array_equal(u, v) for u, v in zip(got, want[:5] + (want[5][:, :cap],)))
        t_dense = _timed(dense, args.reps)
        lines += [f"{name}: m = {m}; snapshot {sel.size} bytes, pages {info['pages']}, records {info['records']}, "
                  f"rows {info['rows']}" + ("; equals snapshot(): " + str(bool(np.array_equal(sel, snap)))
                                            if name == "identity" else ""),
                  f"    snapshot(select)        [ms]  {_stats(t_sel)}   of snapshot(): "
                  f"{med(t_sel) / med(t_snap):.2f}",
                  f"    restore() into m        [ms]  {_stats(t_res)}   restored state equals the dense selection: "
                  f"{same}",
                  f"    get_state+index+set_state [ms]  {_stats(t_dense)}   ratio of medians to snapshot(select) + "
                  f"restore(): {med(t_dense) / (med(t_sel) + med(t_res)):.2f}"]
        g.close()
    return lines


if __name__ == "__main__":
    main()
