"""FastSLAM2: drop-in for the reference's fast_slam_2.algorithms.FastSLAM2.

The per-scan hot path -- motion sample, association, EKF, likelihood,
normalisation, N_eff, low-variance resample, estimate
(reference fast_slam_2/algorithms/fast_slam_2.py:33-223) -- runs in libfs2.so on
the GPU; particle state stays resident in HBM between scans.

Randomness.  By default the motion noise and the resample starting point are
drawn from numpy's global legacy RandomState exactly as the reference draws
them (N normals in particle order, then one uniform only if resampling fires,
SURVEY.md Q4/Q5), so a seeded run reproduces the reference's stream.  The
draws are made on the GPU from np.random.get_state() (fs2_mt_draw: MT19937 and
the polar method bit for bit, a few logs near a rounding midpoint recomputed
with the host's libm) and numpy's state is advanced to where the reference's
draws leave it: past the normals, and past the uniform only when resampling
fired.  rng="numpy-host" draws them with numpy on the host instead (the same
values, ~10 ms per 1e6 particles); rng="device" draws both with Philox on the
GPU (not numpy's stream; used by bench.py).
"""
from __future__ import annotations

import ctypes as C
import math
from collections.abc import Sequence
from typing import NamedTuple

import numpy as np

from .. import _native as nat
from .. import _npstate
from .. import config
from ..models.landmark import Landmark
from ..models.measurement import Measurement
from ..models.particle import Particle

_REDUCE = {"auto": nat.FS2_REDUCE_AUTO, "sequential": nat.FS2_REDUCE_SEQUENTIAL,
           "parallel": nat.FS2_REDUCE_PARALLEL, "exact": nat.FS2_REDUCE_EXACT}

# A bytes object of a given size that the library fills in place (poses_json): the
# C API's own way to build one, without a second copy of a 134 MB text.
_new_bytes = C.pythonapi.PyBytes_FromStringAndSize
_new_bytes.restype = C.py_object
_new_bytes.argtypes = [C.c_char_p, C.c_ssize_t]
_bytes_addr = C.pythonapi.PyBytes_AsString
_bytes_addr.restype = C.c_void_p
_bytes_addr.argtypes = [C.py_object]


class PoseMoments(NamedTuple):
    """FastSLAM2.pose_moments' result."""
    mean: np.ndarray            # (3,): x, y, circular mean of yaw
    cov: np.ndarray             # (3, 3) weighted population covariance
    weight_sum: float           # W
    weight_sq_sum: float        # sum of w^2
    resultant: float            # mean resultant length of the yaws
    bbox: np.ndarray            # (4,): min x, min y, max x, max y


class MapSummary(NamedTuple):
    """FastSLAM2.map_summary's result."""
    landmarks: int              # T: sum of the particles' landmark counts
    page_refs: int              # R: live page-table entries
    pages: int                  # U: distinct pages they name
    max_count: int              # largest landmark count of a particle
    bbox: np.ndarray            # (4,): min x, min y, max x, max y of the landmark means


class Subsample(NamedTuple):
    """FastSLAM2.subsample's result (k drawn particles)."""
    idx: np.ndarray             # (k,) int64, non-decreasing particle indices
    x: np.ndarray               # (k,) the drawn particles' x, y, yaw, weights ...
    y: np.ndarray
    yaw: np.ndarray
    w: np.ndarray
    counts: np.ndarray          # ... and landmark counts (int32)
    scale_exp: int              # e of the amounts q = rint(w 2^e) (0 when not weighted)
    total: int                  # Q, the sum of the amounts


def fit_density_window(bbox, shape, origin=None, cell=None):
    """FastSLAM2.pose_density's window rule (documented there): (origin, cell) for a grid
    of shape (ny, nx) over bbox = (xmin, ymin, xmax, ymax), given neither, or one, of them."""
    ny, nx = shape
    lo, hi, n = (float(bbox[0]), float(bbox[1])), (float(bbox[2]), float(bbox[3])), (nx, ny)
    if not all(math.isfinite(v) for v in lo + hi):
        raise ValueError(f"pose_density: cannot fit a window to the bounding box {lo + hi}")
    fitted = origin is None

    def snap(c):
        return tuple(math.floor(lo[a] / c) * c if n[a] > 1 else lo[a] for a in range(2))

    if cell is not None:
        return snap(float(cell)), float(cell)
    org = lo if fitted else (float(origin[0]), float(origin[1]))
    c = max((hi[a] - org[a]) / (max(n[a] - 1, 1) if fitted else n[a]) for a in range(2))
    if not c > 0.0:
        c = 1.0
    for _ in range(256):
        if fitted:
            org = snap(c)
        if all(math.floor((hi[a] - org[a]) / c) <= n[a] - 1 for a in range(2)):
            return org, c
        c *= 1.0625
    raise ValueError(f"pose_density: no cell covers the bounding box {lo + hi} in shape {shape}")


class FastSLAM2:
    """FastSLAM 2.0 particle filter (reference fast_slam_2.py:15-31)."""

    def __init__(self, num_particles: int | None = None, *, device: int = 0, rng: str = "numpy",
                 seed: int | None = None, reduce: str = "auto", record_assoc: bool = False,
                 landmark_capacity: int = 64, rank: int = 0, world_size: int = 1,
                 comm_id: bytes | None = None, verbose: bool = True, gate_filter: bool = True,
                 comm_mode: str = "rccl", sharded_path: bool = False, page_pool: int = 0,
                 record_pool: int = 0, page_refs: str = "auto", max_landmark_capacity: int = 0):
        lib = nat.load()
        cfg = nat.default_config()
        cfg.num_particles = int(config.NUM_PARTICLES if num_particles is None else num_particles)
        cfg.translation_noise = float(config.TRANSLATION_NOISE)
        cfg.rotation_noise = float(config.ROTATION_NOISE)
        R = np.asarray(config.MEASUREMENT_NOISE, dtype=np.float64).reshape(4)
        for k in range(4):
            cfg.measurement_noise[k] = R[k]
        cfg.max_landmark_distance = float(config.MAXIMUM_LANDMARK_DISTANCE)
        cfg.landmark_capacity = int(landmark_capacity)
        cfg.max_landmark_capacity = int(max_landmark_capacity)   # hard limit on map slots (0: 4096)
        cfg.device = int(device)
        cfg.reduce_mode = _REDUCE[reduce]
        if seed is not None:
            cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        cfg.record_assoc = 1 if record_assoc else 0
        cfg.gate_filter = 1 if gate_filter else 0
        cfg.rank = int(rank)
        cfg.world_size = int(world_size)
        if comm_id is not None:
            C.memmove(cfg.comm_id, comm_id, 128)
        cfg.comm_mode = {"rccl": nat.FS2_COMM_RCCL, "local": nat.FS2_COMM_LOCAL,
                         "shm": nat.FS2_COMM_SHM}[comm_mode]
        cfg.sharded_path = 1 if sharded_path else 0
        cfg.page_pool = int(page_pool)          # initial pool sizes (0: defaults; fs2.h)
        cfg.record_pool = int(record_pool)
        # sharded resample: pages by reference ("on"), by content ("off"); fs2.h page_refs
        cfg.page_refs = {"auto": 0, "on": 1, "off": -1}[page_refs]
        if rng not in ("numpy", "numpy-host", "device"):
            raise ValueError("rng must be 'numpy', 'numpy-host' or 'device'")
        self._rng = rng
        self._verbose = verbose
        h = C.c_void_p()
        nat.check(lib.fs2_create(C.byref(cfg), C.byref(h)))
        self._lib = lib
        self._h = h
        self._cfg = cfg
        n_local, first, cap = C.c_int64(), C.c_int64(), C.c_int32()
        nat.check(lib.fs2_shard_info(h, C.byref(n_local), C.byref(first), C.byref(cap)), h)
        self.num_particles = int(cfg.num_particles)
        self.n_local = int(n_local.value)
        self._particles = None
        self.last_stats = None
        # step(): fs2_iterate through a prototype of plain addresses and buffers
        # made once (ndarray.ctypes conversions cost ~3 us each, a scan ~500 us)
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int32,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
        self._iterate_raw = proto(C.cast(lib.fs2_iterate, C.c_void_p).value)
        sproto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int32,
                             C.c_void_p, C.c_void_p)
        self._submit_raw = sproto(C.cast(lib.fs2_iterate_submit, C.c_void_p).value)
        wproto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
        self._wait_raw = wproto(C.cast(lib.fs2_iterate_wait, C.c_void_p).value)
        self._hv = h.value
        self._mcap = 0
        self._grow_meas(8)                      # measurement / observed-point buffers
        self._pose = np.empty(3)
        self._pose_addr = self._pose.ctypes.data
        self._st = nat.fs2_iter_stats()
        self._st_addr = C.addressof(self._st)
        self._u0 = np.empty(1)
        self._u0_addr = self._u0.ctypes.data
        self._mt = [nat.fs2_mt_state() for _ in range(3)]     # in, after the normals, after u0
        self._mt_addr = [C.addressof(m) for m in self._mt]
        dproto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p)
        self._draw_raw = dproto(C.cast(lib.fs2_mt_draw_deferred, C.c_void_p).value)

    @property
    def first_global(self) -> int:
        """Global index of local particle 0.  Sharded handles with equal shards may
        take another shard at a resample (the one their sources fill most; DESIGN.md
        §5), so this is read from libfs2 each time."""
        if self._h is None:
            raise nat.FS2Error(nat.FS2_ERR_ARG, "first_global of a closed FastSLAM2 handle")
        n_local, first, cap = C.c_int64(), C.c_int64(), C.c_int32()
        nat.check(self._lib.fs2_shard_info(self._h, C.byref(n_local), C.byref(first), C.byref(cap)), self._h)
        return int(first.value)

    # ------------------------------------------------------------------ core
    def iterate(self, rotation: float, translation: float,
                measurements: list[Measurement]) -> tuple[float, float, float]:
        """One FastSLAM step (reference fast_slam_2.py:33-67); returns the estimate pose."""
        if not getattr(self, "_h", None) or not self._hv:
            raise nat.FS2Error(nat.FS2_ERR_ARG, "iterate on a closed FastSLAM2 handle")
        M = len(measurements)
        if M > self._mcap:
            self._grow_meas(M)
        mb, ob = self._mbuf, self._obuf
        for k, m in enumerate(measurements):
            d, b = m.distance, m.yaw
            mb[k, 0] = d
            mb[k, 1] = b
            # observed robot-frame point, computed as the reference does (:100-103)
            ob[k, 0] = d * np.cos(b)
            ob[k, 1] = d * np.sin(b)
        noise = u0 = None
        state = None
        sigma = config.ROTATION_NOISE if rotation != 0 else config.TRANSLATION_NOISE
        if self._rng == "numpy":
            mt_in = self._mt[0]
            npv = _npstate.view()                # numpy's state in place (get_state: ~40-70 us)
            if npv is not None:
                npv.read(mt_in)
            else:
                C.pointer(mt_in)[0] = nat.fs2_mt_state.from_numpy(np.random.get_state())
            # ended by fs2_iterate below, while its candidate pass runs (mt_after / mt_u0 written then)
            rc = self._draw_raw(self._hv, self._mt_addr[0], float(sigma), self._mt_addr[1], self._mt_addr[2], None)
            if rc == nat.FS2_ERR_STATE and "libm" in nat.last_error(self._h):
                self._rng = "numpy-host"        # another libm: numpy draws on the host, still exact
            else:
                nat.check(rc, self._h)
        if self._rng == "numpy-host":
            noise = np.random.normal(0, sigma, size=self.num_particles)
            noise = np.ascontiguousarray(noise[self.first_global:self.first_global + self.n_local])
            state = np.random.get_state()
            self._u0[0] = np.random.uniform(0, 1 / self.num_particles)
            u0 = self._u0_addr
        rc = self._iterate_raw(self._hv, float(rotation), float(translation), self._mbuf_addr if M else None,
                               self._obuf_addr if M else None, M, None if noise is None else noise.ctypes.data, u0,
                               self._pose_addr, self._st_addr)
        self._particles = None
        st = nat.fs2_iter_stats.from_buffer_copy(self._st)
        self.last_stats = st
        if self._rng == "numpy":
            # the normals are drawn by the move, u0 only when resampling (fast_slam_2.py:79,81,183)
            chosen = self._mt[2] if (rc == 0 and st.resampled) else self._mt[1]
            npv = _npstate.view()
            if npv is not None:
                npv.write(chosen)
            else:
                np.random.set_state(chosen.to_numpy())
        elif state is not None and not st.resampled:
            np.random.set_state(state)          # the reference draws u0 only when resampling
        nat.check(rc, self._h)
        if st.resampled and self._verbose:
            print("\nRESAMPLING")               # reference fast_slam_2.py:63
        pose = self._pose
        return float(pose[0]), float(pose[1]), float(pose[2])

    def _grow_meas(self, M):
        self._mcap = max(M, 2 * self._mcap, 8)
        self._mbuf = np.empty((self._mcap, 2))
        self._obuf = np.empty((self._mcap, 2))
        self._mbuf_addr = self._mbuf.ctypes.data
        self._obuf_addr = self._obuf.ctypes.data

    def step(self, rotation: float, translation: float, meas, observed=None, noise=None,
             u0=None):
        """iterate() with explicit inputs: meas [M][2] (distance, yaw); observed [M][2]
        robot-frame points (None: computed in libfs2); noise [N_local] motion draws and
        u0 the resample start (None: Philox on the device).  Returns (pose, stats)."""
        return self._step(rotation, translation, meas, observed, noise, u0, split=False)

    def step_submit(self, rotation: float, translation: float, meas, observed=None, noise=None, u0=None):
        """The first half of step(): enqueue the scan and return while the GPU works
        (libfs2 fs2_iterate_submit).  Finish it with step_wait()."""
        self._step(rotation, translation, meas, observed, noise, u0, split=True)

    def step_wait(self):
        """Complete the scan step_submit() enqueued; returns (pose, stats) like step()."""
        if not getattr(self, "_h", None) or not self._hv:
            raise nat.FS2Error(nat.FS2_ERR_ARG, "step_wait() on a closed FastSLAM2 handle")
        rc = self._wait_raw(self._hv, self._pose_addr, self._st_addr)
        self._particles = None
        st = nat.fs2_iter_stats.from_buffer_copy(self._st)
        self.last_stats = st
        nat.check(rc, self._h)
        return self._pose.copy(), st

    def _step(self, rotation, translation, meas, observed, noise, u0, split):
        if not getattr(self, "_h", None) or not self._hv:
            raise nat.FS2Error(nat.FS2_ERR_ARG, "step() on a closed FastSLAM2 handle")
        meas = nat.f64(meas).reshape(-1, 2)
        M = meas.shape[0]
        obs = None
        if observed is not None:
            obs = nat.f64(observed).reshape(-1, 2)
            if obs.shape[0] != M:
                raise ValueError(f"observed has {obs.shape[0]} points for {M} measurements")
        if M > self._mcap:
            self._grow_meas(M)
        oa = None
        if M:
            self._mbuf[:M] = meas
            if obs is not None:
                self._obuf[:M] = obs
                oa = self._obuf_addr
        nz = None
        if noise is not None:
            nz = nat.f64(noise)
            if nz.size != self.n_local:
                raise ValueError(f"noise must have {self.n_local} values")
        ua = None
        if u0 is not None:
            self._u0[0] = float(u0)
            ua = self._u0_addr
        if split:
            rc = self._submit_raw(self._hv, float(rotation), float(translation), self._mbuf_addr if M else None, oa,
                                  M, None if nz is None else nz.ctypes.data, ua)
            self._particles = None
            nat.check(rc, self._h)
            return None
        rc = self._iterate_raw(self._hv, float(rotation), float(translation), self._mbuf_addr if M else None, oa,
                               M, None if nz is None else nz.ctypes.data, ua, self._pose_addr, self._st_addr)
        self._particles = None
        st = nat.fs2_iter_stats.from_buffer_copy(self._st)
        self.last_stats = st
        nat.check(rc, self._h)
        return self._pose.copy(), st

    # ------------------------------------------------------------ particles
    def get_state(self, first: int = 0, count: int | None = None, lm_cap: int | None = None):
        """Local particles [first, first+count) as arrays (x, y, yaw, w, cnt, lm[count][cap][6])."""
        count = self.n_local - first if count is None else count
        x, y, yaw, w = (np.empty(count) for _ in range(4))
        cnt = np.empty(count, dtype=np.int32)
        nat.check(self._lib.fs2_get_state(self._h, first, count, nat.ptr(x), nat.ptr(y),
                                          nat.ptr(yaw), nat.ptr(w), nat.ptr(cnt), None, 0,
                                          nat.FS2_HOST), self._h)
        cap = int(cnt.max()) if (lm_cap is None and count) else (lm_cap or 0)
        lm = np.zeros((count, max(cap, 1), 6))
        if cap:
            nat.check(self._lib.fs2_get_state(self._h, first, count, None, None, None, None,
                                              None, nat.ptr(lm), max(cap, 1), nat.FS2_HOST),
                      self._h)
        return x, y, yaw, w, cnt, lm

    def set_state(self, x=None, y=None, yaw=None, w=None, cnt=None, lm=None, first: int = 0):
        """Upload local particles starting at `first`; lm is [count][cap][6] with cnt."""
        arrs = [None if a is None else nat.f64(a) for a in (x, y, yaw, w)]
        count = next((len(a) for a in arrs + [cnt] if a is not None), 0)
        lmh = None
        cap = 0
        cnth = None
        if cnt is not None:
            cnth = np.ascontiguousarray(cnt, dtype=np.int32)
            lmh = nat.f64(lm)
            cap = lmh.shape[1]
        nat.check(self._lib.fs2_set_state(self._h, first, count, *(nat.ptr(a) for a in arrs),
                                          nat.ptr(cnth), nat.ptr(lmh), cap, nat.FS2_HOST),
                  self._h)
        self._particles = None

    # ------------------------------------------------------------ snapshots
    def snapshot(self, select=None) -> np.ndarray:
        """The filter as one uint8 array (fs2_snapshot_save): particles, maps and the scan
        counter in the device's own compact form -- every distinct page and record once, so
        maps that resampled siblings share are stored once -- for `restore` to resume the run
        bit for bit.  One sizing call, then one save into a single allocation.

        select: an integer array-like of particle indices in [0, N) (negative ones are
        refused, not wrapped; repeats allowed; it may be longer than N).  The result is
        then the snapshot of those particles in that order (fs2_snapshot_save_select), for
        a filter of len(select) particles to `restore`: a thinned filter, a slice, a
        permutation.  Poses, weights and maps are copied verbatim and only the pages and
        records they reach are stored; a particle taken more than once shares its pages
        between the copies.  Weights are not renormalised: set_state(w=...) on the
        restored filter sets others and leaves the maps alone.

        With rng="numpy" or rng="numpy-host" the generator's state belongs to the caller:
        keep np.random.get_state() next to the snapshot and np.random.set_state() it before
        resuming.  rng="device" draws from (seed, scan counter), which the snapshot holds."""
        size = C.c_int64()
        if select is None:
            def save(addr, cap):
                return self._lib.fs2_snapshot_save(self._h, addr, cap, C.byref(size))
        else:
            idx = np.asarray(select)
            if idx.dtype.kind not in "iu":
                raise TypeError(f"select must hold integers, not {idx.dtype}")
            if idx.dtype.kind == "u" and idx.size and int(idx.max()) > np.iinfo(np.int64).max:
                raise ValueError("select holds an index above the int64 range")
            idx = np.ascontiguousarray(idx.reshape(-1), dtype=np.int64)

            def save(addr, cap):
                return self._lib.fs2_snapshot_save_select(self._h, idx.ctypes.data, idx.size, addr, cap,
                                                          C.byref(size))
        nat.check(save(None, 0), self._h)
        out = np.empty(size.value, dtype=np.uint8)
        nat.check(save(out.ctypes.data, out.size), self._h)
        return out

    def restore(self, buf) -> None:
        """Replace this filter's particles, maps and scan counter with a snapshot's
        (fs2_snapshot_load; any object with the buffer protocol).  The snapshot must be of
        the same particle count; it is validated completely first and an invalid one leaves
        the filter unchanged.  This filter keeps its own configuration (noise, gate, seed,
        reduce mode): resume with the arguments the snapshot's filter was made with.

        With rng="numpy" or rng="numpy-host" restore np.random's state yourself
        (np.random.set_state(saved)); see `snapshot`."""
        a = np.frombuffer(buf, dtype=np.uint8)
        nat.check(self._lib.fs2_snapshot_load(self._h, a.ctypes.data, a.size), self._h)
        self._particles = None

    @staticmethod
    def snapshot_info(buf) -> dict:
        """Validate a snapshot on the host (no device) and describe it: bytes,
        num_particles, rows, pages, records, max_count, scan, version.  Raises FS2Error
        (FS2_ERR_ARG) naming the first violated rule."""
        a = np.frombuffer(buf, dtype=np.uint8)
        info = nat.fs2_snapshot_info()
        nat.check(nat.load().fs2_snapshot_check(a.ctypes.data, a.size, C.byref(info)))
        return info.as_dict()

    @property
    def particles(self) -> "ParticleView":
        """This rank's particles (reference attribute `particles`), materialised lazily in
        chunks; LandmarkUtils.update_known_landmarks given this view clusters on the device."""
        if self._particles is None:
            self._particles = ParticleView(self)
        return self._particles

    def poses(self):
        """(x, y, yaw) arrays of this rank's particles (one structure-of-arrays download)."""
        x, y, yaw = (np.empty(self.n_local) for _ in range(3))
        nat.check(self._lib.fs2_get_state(self._h, 0, self.n_local, nat.ptr(x), nat.ptr(y), nat.ptr(yaw),
                                          None, None, None, 0, nat.FS2_HOST), self._h)
        return x, y, yaw

    def poses_json(self, depth: int = 1, head: bytes = b"", tail: bytes = b"") -> bytes:
        """The JSON list of this rank's {"x", "y", "yaw"} objects exactly as
        json.dump(..., indent=4) writes it at nesting depth `depth`, formatted on the
        device from the resident poses (fs2_particles_json): one sizing call, then one
        that fills a bytes object of that size in place.  head / tail: bytes to put
        before / after the list in the same object (the Serializer's document around
        it), so the large text is never copied to be joined."""
        size = C.c_int64()
        nat.check(self._lib.fs2_particles_json(self._h, 0, self.n_local, int(depth), None, 0,
                                               C.byref(size)), self._h)
        n = size.value
        out = _new_bytes(None, len(head) + n + len(tail))   # uninitialised, ours alone until returned
        addr = _bytes_addr(out)
        C.memmove(addr, head, len(head))
        nat.check(self._lib.fs2_particles_json(self._h, 0, self.n_local, int(depth),
                                               addr + len(head), n, C.byref(size)), self._h)
        C.memmove(addr + len(head) + n, tail, len(tail))
        return out

    # ------------------------------------------------------ posterior readout
    def _moments_raw(self, weighted, what, cov=True):
        if not getattr(self, "_h", None):
            raise nat.FS2Error(nat.FS2_ERR_ARG, f"{what}() on a closed FastSLAM2 handle")
        mean, cv, sums, bbox = np.empty(3), (np.empty((3, 3)) if cov else None), np.empty(4), np.empty(4)
        nat.check(self._lib.fs2_pose_moments(self._h, 1 if weighted else 0, nat.ptr(mean), nat.ptr(cv),
                                             nat.ptr(sums), nat.ptr(bbox)), self._h)
        return mean, cv, sums, bbox

    def pose_moments(self, weighted: bool = True) -> "PoseMoments":
        """Moments of the particle cloud, reduced on the device (fs2_pose_moments; DESIGN.md
        §14): `mean` (x, y and the circular mean of yaw, in [-pi, pi)), `cov` the 3x3 weighted
        population covariance of (x, y, yaw wrapped about its mean), `weight_sum` W,
        `weight_sq_sum`, `resultant` (the mean resultant length of the yaws, 1 = all equal)
        and `bbox` (min x, min y, max x, max y).

        weighted=True weighs each particle by its weight as it stands and divides by W (the
        weights need not sum to 1); weighted=False counts each particle once.  The reference
        does not reset the weights at a resample, so right after a
        resampling scan the weights still are those of the particles' sources while the
        cloud itself already is the resampled posterior: there the unweighted form is the
        cloud's own posterior.  FS2Error (FS2_ERR_STATE) for a negative or non-finite weight
        or W = 0 when weighted, and on a sharded handle.  Two calls on the same state
        return the same bits."""
        mean, cov, sums, bbox = self._moments_raw(weighted, "pose_moments")
        return PoseMoments(mean, cov, float(sums[0]), float(sums[1]), float(sums[2]), bbox)

    def pose_density(self, shape, origin=None, cell=None, weighted: bool = True, raw: bool = False):
        """A 2-D histogram of the particle positions, accumulated on the device in integers
        (fs2_pose_density; exact, independent of summation order).  shape = (ny, nx); the
        particle at (x, y) counts in grid[iy, ix], ix = floor((x - origin[0]) / cell),
        iy = floor((y - origin[1]) / cell), when that lies in the grid; every other particle
        (a non-finite pose too) counts in `outside`.  Amounts: 1 per particle when not
        weighted, else q = rint(w 2^e) with the exponent e the library chooses from the
        largest weight and the particle count (fs2_density_scale).

        Returns (grid, outside, origin, cell): grid float64 [ny, nx], the counts times
        2^-e (sums of weights up to the rounding of each q), outside likewise, origin a
        tuple (x0, y0).  raw=True returns the uint64 counts and the int outside instead,
        and appends e: (grid, outside, origin, cell, scale_exp).

        The window.  With origin and cell both given it is used as it is.  Otherwise it is
        fitted to pose_moments' bbox = (xmin, ymin, xmax, ymax), which must be finite:
          * cell given, origin None: origin = (floor(xmin / cell) cell, floor(ymin / cell) cell)
            (on an axis of one cell: the bbox minimum itself, see below).
          * cell None: the spans are sx = xmax - x_lo, sy = ymax - y_lo with (x_lo, y_lo) the
            given origin, or (xmin, ymin) when origin is None; the divisors are dx = nx,
            dy = ny for a given origin and dx = max(nx - 1, 1), dy = max(ny - 1, 1) for a
            fitted one (snapping the origin down can cost up to one cell);
            cell = max(sx / dx, sy / dy), or 1.0 if that is not positive.  A fitted origin is
            snapped down to a multiple of the cell as above, except on an axis of one cell,
            where it is the bbox minimum itself (one cell at a multiple of its size cannot
            cover a cloud that straddles one).  Then, while floor((xmax - x0) / cell) > nx - 1
            or floor((ymax - y0) / cell) > ny - 1 (the device's own index arithmetic), cell
            is multiplied by 1.0625 and a fitted origin snapped again.
        With a fitted origin and cell no particle of a finite cloud is outside.
        `fit_density_window` is this rule as a function."""
        if not getattr(self, "_h", None):
            raise nat.FS2Error(nat.FS2_ERR_ARG, "pose_density() on a closed FastSLAM2 handle")
        ny, nx = (int(v) for v in shape)
        if origin is None or cell is None:
            if nx < 1 or ny < 1:
                raise ValueError("pose_density: shape must be (ny >= 1, nx >= 1)")
            origin, cell = fit_density_window(self._moments_raw(False, "pose_density", cov=False)[3], (ny, nx),
                                              origin, cell)
        x0, y0, cell = float(origin[0]), float(origin[1]), float(cell)
        counts = np.empty((max(ny, 0), max(nx, 0)), dtype=np.uint64)
        e, out = C.c_int32(), C.c_uint64()
        nat.check(self._lib.fs2_pose_density(self._h, 1 if weighted else 0, x0, y0, cell, nx, ny,
                                             nat.ptr(counts) if counts.size else None, C.byref(e), C.byref(out)),
                  self._h)
        if raw:
            return counts, int(out.value), (x0, y0), cell, int(e.value)
        return (np.ldexp(counts.astype(np.float64), -e.value), float(np.ldexp(float(out.value), -e.value)),
                (x0, y0), cell)

    # ------------------------------------------------------------ map readout
    def map_summary(self) -> "MapSummary":
        """Counts and bounding box of the map posterior -- every live landmark of every
        particle -- from the page pool on the device (fs2_map_summary), without
        forming a dense map: `landmarks` T = sum of the particles' landmark counts,
        `page_refs` R = the live page-table entries (sum of ceil(count / 8)), `pages` U = the
        distinct pages they name (U / R is the share of the maps the particles do not have in
        common: 1 with nothing shared, small after resamples), `max_count`, and `bbox` (min x,
        min y, max x, max y of the landmarks' fp64 means; (inf, inf, -inf, -inf) when there is
        no landmark).  FS2Error (FS2_ERR_STATE) on a sharded handle and while a scan is
        pending."""
        if not getattr(self, "_h", None):
            raise nat.FS2Error(nat.FS2_ERR_ARG, "map_summary() on a closed FastSLAM2 handle")
        bbox, counts = np.empty(4), np.empty(4, dtype=np.int64)
        nat.check(self._lib.fs2_map_summary(self._h, nat.ptr(bbox), nat.ptr(counts)), self._h)
        return MapSummary(int(counts[0]), int(counts[1]), int(counts[2]), int(counts[3]), bbox)

    def map_density(self, shape, origin=None, cell=None, weighted: bool = True, raw: bool = False):
        """A 2-D histogram of every live landmark of every particle, accumulated on the device
        in integers (fs2_map_density; exact, independent of summation order).
        A landmark of particle i with fp64 mean (mx, my) counts in grid[iy, ix] by
        pose_density's rule and adds the particle's amount: 1 when not weighted, else
        q_i = rint(w_i 2^e), e chosen from the largest weight and the landmark total
        (fs2_density_scale(wmax, max(T, 1))).  Each distinct page of the pool is opened once,
        however many particles share it.

        shape, origin, cell, raw and the return forms are pose_density's: (grid, outside,
        origin, cell), or with raw=True the uint64 counts, the int outside and scale_exp
        appended.  Without origin or cell the window is fitted to map_summary().bbox by
        `fit_density_window`; with no landmark at all that is a ValueError."""
        if not getattr(self, "_h", None):
            raise nat.FS2Error(nat.FS2_ERR_ARG, "map_density() on a closed FastSLAM2 handle")
        ny, nx = (int(v) for v in shape)
        if origin is None or cell is None:
            if nx < 1 or ny < 1:
                raise ValueError("map_density: shape must be (ny >= 1, nx >= 1)")
            ms = self.map_summary()
            if ms.landmarks == 0:
                raise ValueError("map_density: no landmark to fit a window to (give origin and cell)")
            origin, cell = fit_density_window(ms.bbox, (ny, nx), origin, cell)
        x0, y0, cell = float(origin[0]), float(origin[1]), float(cell)
        counts = np.empty((max(ny, 0), max(nx, 0)), dtype=np.uint64)
        e, out = C.c_int32(), C.c_uint64()
        nat.check(self._lib.fs2_map_density(self._h, 1 if weighted else 0, x0, y0, cell, nx, ny,
                                            nat.ptr(counts) if counts.size else None, C.byref(e), C.byref(out)),
                  self._h)
        if raw:
            return counts, int(out.value), (x0, y0), cell, int(e.value)
        return (np.ldexp(counts.astype(np.float64), -e.value), float(np.ldexp(float(out.value), -e.value)),
                (x0, y0), cell)

    # ------------------------------------------------------- weighted subsample
    def subsample(self, k: int, offset: int | None = None, weighted: bool = True) -> "Subsample":
        """k particles drawn in proportion to their weights by the systematic sampler, on
        the device and in integers (fs2_subsample): `idx` (int64,
        non-decreasing), the drawn particles' `x`, `y`, `yaw`, `w` and landmark `counts`
        gathered on the device (x[j] is particle idx[j]'s x bit for bit), and `scale_exp`,
        `total`: the e and Q of the amounts q_i = rint(w_i 2^e) the draw is exact for.
        Particle i is drawn floor(k q_i / Q) or ceil(k q_i / Q) times and never when
        q_i = 0; numpy reproduces idx bit for bit (np.cumsum of q, np.searchsorted of the
        thresholds floor((j Q + floor(offset Q / 2^32)) / k), side="right").

        offset: the sampler's one uniform as a 32-bit integer, u = offset / 2^32.  None
        means 2^31, the mid-stratum draw, so the call is deterministic.  np.random is
        never consumed (the drop-in replays depend on numpy's stream being left alone); for
        a random draw pass offset=int(rng.integers(2**32)) from a generator of your own.

        weighted=True uses the weights as they stand (they need not sum to 1);
        weighted=False draws every particle equally (idx[j] = floor((j N + s) / k)) and
        does not read the weights.  The reference does not reset the weights at a resample
        (DESIGN.md §2, Q8), so right after a resampling scan the unweighted form is the
        cloud's own posterior.

        snapshot(select=sub.idx) is the thinned filter of the drawn particles, maps
        included; `restore` it into a FastSLAM2 of k particles.  FS2Error (FS2_ERR_STATE)
        for a negative or non-finite weight or no positive weight when weighted, on a
        sharded handle and while a scan is pending; ValueError for k outside [1, 2^30]."""
        if not getattr(self, "_h", None):
            raise nat.FS2Error(nat.FS2_ERR_ARG, "subsample() on a closed FastSLAM2 handle")
        k = int(k)
        offset = 1 << 31 if offset is None else int(offset)
        if not 0 <= offset < 1 << 32:
            raise ValueError("subsample: offset must be an integer in [0, 2^32)")
        m = k if 1 <= k <= 1 << 30 else 0            # (the library refuses k before it touches an array)
        idx = np.empty(m, dtype=np.int64)
        x, y, yaw, w = (np.empty(m) for _ in range(4))
        cnt = np.empty(m, dtype=np.int32)
        e, total = C.c_int32(), C.c_uint64()
        nat.check(self._lib.fs2_subsample(self._h, 1 if weighted else 0, k, offset, nat.ptr(idx), nat.ptr(x),
                                          nat.ptr(y), nat.ptr(yaw), nat.ptr(w), nat.ptr(cnt), C.byref(e),
                                          C.byref(total)), self._h)
        return Subsample(idx, x, y, yaw, w, cnt, int(e.value), int(total.value))

    def cluster_landmarks(self, eps: float = 0.5, min_fraction: float = 0.7):
        """Centres [K][2] of DBSCAN over every particle's landmarks, on the device
        (update_known_landmarks, landmark_utils.py:120-144); None when min_samples < 1."""
        cap = 256
        while True:
            cen = np.empty((cap, 2))
            k = C.c_int64()
            rc = self._lib.fs2_update_known_landmarks(self._h, float(eps), float(min_fraction),
                                                      nat.dptr(cen), cap, C.byref(k))
            if rc == nat.FS2_ERR_ARG and k.value > cap:
                cap = int(k.value)
                continue
            nat.check(rc, self._h)
            return None if k.value < 0 else cen[:k.value].copy()

    @particles.setter
    def particles(self, plist: list[Particle]):
        if len(plist) != self.n_local:
            raise ValueError(f"expected {self.n_local} particles, got {len(plist)}")
        cnt = np.array([len(p.landmarks) for p in plist], dtype=np.int32)
        cap = max(int(cnt.max()) if len(cnt) else 0, 1)
        lm = np.zeros((len(plist), cap, 6))
        for i, p in enumerate(plist):
            for j, l in enumerate(p.landmarks):
                c = np.asarray(l.cov, dtype=np.float64).reshape(4)
                lm[i, j] = (l.x, l.y, c[0], c[1], c[2], c[3])
        self.set_state([p.x for p in plist], [p.y for p in plist], [p.yaw for p in plist],
                       [p.weight for p in plist], cnt, lm)

    # ------------------------------------------------------------ extras
    def associations(self) -> np.ndarray:
        """[M][N_local] association indices of the last scan (-1 = appended)."""
        m = C.c_int32()
        buf = np.empty(max(self.n_local * 64, 1), dtype=np.int32)
        nat.check(self._lib.fs2_get_assoc(self._h, buf.ctypes.data_as(C.POINTER(C.c_int32)),
                                          buf.size, C.byref(m)), self._h)
        return buf[:m.value * self.n_local].reshape(m.value, self.n_local).copy()

    def set_profiling(self, enable: bool = True, every: int = 1):
        """Device-event timing of the update kernels on every `every`-th scan (libfs2
        fs2_set_profiling; resets the profile)."""
        nat.check(self._lib.fs2_set_profiling(self._h, max(1, int(every)) if enable else 0), self._h)

    def profile(self) -> dict:
        p = nat.fs2_profile()
        nat.check(self._lib.fs2_get_profile(self._h, C.byref(p)), self._h)
        return p.as_dict()

    def synchronize(self):
        nat.check(self._lib.fs2_synchronize(self._h), self._h)

    def close(self):
        self._hv = None                         # step()'s raw address: never reused once freed
        if getattr(self, "_h", None):
            self._lib.fs2_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ParticleView(Sequence):
    """Lazy, read-only sequence of Particle objects over a FastSLAM2's device state
    (downloaded 4096 particles at a time on first access)."""

    _CHUNK = 4096

    def __init__(self, filt: FastSLAM2):
        self._filter = filt
        self._n = filt.n_local
        self._chunks: dict[int, list[Particle]] = {}

    def __len__(self):
        return self._n

    def _chunk(self, c: int) -> list[Particle]:
        if c not in self._chunks:
            first = c * self._CHUNK
            count = min(self._CHUNK, self._n - first)
            x, y, yaw, w, cnt, lm = self._filter.get_state(first, count)
            out = []
            for i in range(count):
                p = Particle.__new__(Particle)
                p.x, p.y, p.yaw, p.weight = float(x[i]), float(y[i]), float(yaw[i]), float(w[i])
                p.landmarks = [Landmark(float(lm[i, j, 0]), float(lm[i, j, 1]),
                                        lm[i, j, 2:6].reshape(2, 2).copy())
                               for j in range(int(cnt[i]))]
                out.append(p)
            self._chunks[c] = out
        return self._chunks[c]

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError("particle index out of range")
        return self._chunk(i // self._CHUNK)[i % self._CHUNK]
