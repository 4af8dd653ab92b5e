#!/usr/bin/env python3
"""What the viewer snapshot costs with the particle block written on the device
(csrc/fs2_json.hip) and with the host emitter (serializer._poses_block, the path
before it), in one process on one GPU.

For N = 1e5 and 1e6 particles with normal(0, 3) poses (set_state), the median, minimum
and maximum of 5 runs after one warm-up of
  (a) Serializer.to_json through FastSLAM2.poses_json (device path),
  (b) Serializer.to_json through poses() + _poses_block (host emitter: the filter is
      wrapped so that it shows no poses_json),
  (c) the HIP-event times of the size pass, the offset scan, the write pass and the
      download (fs2_debug_json_times), the download once more into a pinned buffer,
      and a device-to-device copy of the same bytes for the write pass's rate,
  (d) the bytes produced,
and that (a) and (b) return the same text.

  python scripts/json_probe.py [--sizes 100000 1000000] [--out FILE]      (profiles/json_emit.txt is one run's output)
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


class _HostOnly:
    """A filter that offers only poses(): Serializer then takes the host emitter."""

    def __init__(self, f):
        self._f = f

    def poses(self):
        return self._f.poses()


class _View(list):
    pass


def _stats(v):
    return f"median {statistics.median(v):9.3f}  min {min(v):9.3f}  max {max(v):9.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import fast_slam_2
    from fast_slam_2 import DirectedPoint, EvaluationResults, Point, Serializer
    from fast_slam_2 import _native as nat
    if not torch.cuda.is_available():
        sys.exit("json_probe: no GPU (there is nothing to measure without one)")
    lib = nat.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    est, act = DirectedPoint(0.5, 0.25, 0.1), DirectedPoint(0.0, 0.0, 0.0)
    lms = [Point(float(k), float(-k)) for k in range(12)]
    res = EvaluationResults("t", 0.0, 0.0, 0.0, 0.0, 0.0)
    say(f"device: {torch.cuda.get_device_name(0)}")
    for N in args.sizes:
        rng = np.random.default_rng(N)
        f = fast_slam_2.FastSLAM2(N, rng="device", verbose=False)
        f.set_state(rng.normal(0, 3, N), rng.normal(0, 3, N), rng.normal(0, 3, N), np.full(N, 1.0 / N))
        host_view = _View()
        host_view._filter = _HostOnly(f)
        dev, host = [], []
        text_d = text_h = None
        for r in range(args.reps + 1):              # alternating, the first pair is the warm-up
            t0 = time.perf_counter()
            text_d = Serializer.to_json(est, act, f.particles, lms, res)
            t1 = time.perf_counter()
            text_h = Serializer.to_json(est, act, host_view, lms, res)
            t2 = time.perf_counter()
            if r:
                dev.append((t1 - t0) * 1e3)
                host.append((t2 - t1) * 1e3)
        same = text_d == text_h
        nbytes = len(text_d)
        del text_d, text_h
        # (c) device times of one emission into a pageable and into a pinned buffer
        size = C.c_int64()
        nat.check(lib.fs2_particles_json(f._h, 0, N, 1, None, 0, C.byref(size)), f._h)
        block = size.value
        pageable = np.empty(block, dtype=np.uint8)
        pinned = torch.empty(block, dtype=torch.uint8).pin_memory()
        ms = (C.c_double * 4)()
        lib.fs2_debug_json_times(1, None)
        parts = {"pageable": [], "pinned": []}
        for r in range(args.reps + 1):
            for name, p in (("pageable", pageable.ctypes.data), ("pinned", pinned.data_ptr())):
                nat.check(lib.fs2_particles_json(f._h, 0, N, 1, p, block, C.byref(size)), f._h)
                lib.fs2_debug_json_times(-1, ms)
                if r:
                    parts[name].append(list(ms))
        lib.fs2_debug_json_times(0, None)
        assert pageable.tobytes() == pinned.numpy().tobytes()
        t0 = time.perf_counter()
        pageable[:] = pinned.numpy()
        stage_copy = (time.perf_counter() - t0) * 1e3
        # a device-to-device copy of the block's bytes: the rate the write pass is compared with
        a = torch.empty(block, dtype=torch.uint8, device="cuda")
        b = torch.empty_like(a)
        d2d = []
        for r in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.copy_(a)
            e1.record()
            torch.cuda.synchronize()
            if r:
                d2d.append(e0.elapsed_time(e1))
        pg = np.array(parts["pageable"])
        pn = np.array(parts["pinned"])
        say()
        say(f"N = {N}: document {nbytes} bytes, particle block {block} bytes ({block / N:.1f} per particle); "
            f"device and host texts equal: {same}")
        say(f"  (a) to_json, device path   [ms]  {_stats(dev)}")
        say(f"  (b) to_json, host emitter  [ms]  {_stats(host)}")
        say(f"      ratio of medians (b) / (a): {statistics.median(host) / statistics.median(dev):.1f}; "
            f"(b) spread {max(host) - min(host):.3f} ms, (b) - (a) {statistics.median(host) - statistics.median(dev):.3f} ms")
        for k, nm in enumerate(["size pass", "offset scan", "write pass", "download (pageable)"]):
            say(f"  (c) {nm:20s} [ms]  {_stats(pg[:, k].tolist())}")
        say(f"  (c) {'download (pinned)':20s} [ms]  {_stats(pn[:, 3].tolist())}   + host copy out of it {stage_copy:.3f} ms")
        w = float(np.median(pg[:, 2]))
        c = statistics.median(d2d)
        say(f"  (c) {'device copy of block':20s} [ms]  {_stats(d2d)}")
        say(f"      write pass {block / w / 1e6:.1f} GB/s written, device copy {block / c / 1e6:.1f} GB/s "
            f"(each byte read and written): write pass at {c / w:.2f} of the copy's rate")
        del a, b, pinned
        f.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
