"""Host side of the spectrum C-ABI (include/go1spectrum.h): ctypes mirrors, library loading, the twiddle tables, and `Go1Spectrum`, which
owns the ring of the open segment, the per-environment accumulators and density sums and the result tables of one simulator instance.

libgo1spectrum.so is a library of its own whose device code shares csrc/go1_tables.h with the other table libraries, and the host side
shares as much: `load_library` is `go1eval_host._load` with this module's path, cache, error class and entry points, and `Go1Spectrum`
subclasses `go1eval_host._Table`.  The device computes no trigonometric function: `twiddle_tables` forms the tapered DFT matrix, the
one-sided density scale and the bin frequencies in fp64, rounds them to fp32, and arm() uploads them.  The host counts its own record
calls, so it knows the slot of every step and when a segment closes: `accumulate()` enqueues one launch, and after slot W - 1 the fold.
"""
import ctypes
import os

import numpy as np
import torch

from go1eval_host import _ACCUMULATORS, _Table, _load

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1spectrum.so")

NUM_SIGNALS, NUM_SPECTRUM_METRICS, MIN_SEGMENT, MAX_SEGMENT, FOLD_THREADS = 40, 5, 8, 128, 64
SPECTRUM_NAMES = ["power", "peak_freq", "peak_share", "high_share", "centroid"]                                     # enum Go1SpectrumMetric
SPECTRUM_GROUP_FIELDS = ["envs", "steps", "resets", "segments", "segments_dropped"]                                 # enum Go1SpectrumGroupField
DOF_NAMES = [f"{leg}_{part}" for leg in ("FL", "FR", "RL", "RR") for part in ("hip", "thigh", "calf")]              # the simulator's joint order
QUANTITIES = ["action", "torque", "dof_vel"]                                                                        # signals 0..11, 12..23, 24..35
TRUNK_SIGNALS = ["roll_rate", "pitch_rate", "yaw_rate", "vertical_vel"]                                             # signals 36..39
SIGNAL_NAMES = [f"{q}_{j}" for q in QUANTITIES for j in DOF_NAMES] + TRUNK_SIGNALS
TAPERS = ("hann", "boxcar")


class Go1SpectrumConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("segment_steps", ctypes.c_int32),
                ("high_bin", ctypes.c_int32), ("bin_width", ctypes.c_float)]


_SPECTRUM_INPUTS = ["actions", "torques", "dof_vel", "base_ang_vel", "base_lin_vel", "reset_buf", "episode_length_buf"]
_SPECTRUM_TABLES = ["tw_re", "tw_im", "scale", "freq"]
_SPECTRUM_STATE = ["ring", "valid", "steps", "resets", "segments", "segments_dropped", "psd_sum", "psd_segments"]


class Go1SpectrumBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _SPECTRUM_INPUTS + _SPECTRUM_TABLES + _ACCUMULATORS + _SPECTRUM_STATE +
                ["group", "results", "psd_results", "psd_counts"]]


EXPORTED_SYMBOLS = ["go1spectrum_clear", "go1spectrum_record", "go1spectrum_fold", "go1spectrum_reduce", "go1spectrum_version"]

_lib = None


class Go1SpectrumLibraryMissing(RuntimeError):
    pass


def load_library(path=None):
    """Load libgo1spectrum.so (HIP, gfx950).  Fails loudly: the spectrum kernels have no CPU fallback."""
    lib = _load(globals(), path, Go1SpectrumLibraryMissing, "spectrum metrics", [(EXPORTED_SYMBOLS[:4], Go1SpectrumConfig, Go1SpectrumBuffers)],
                "go1spectrum_version")
    lib.go1spectrum_record.argtypes = [ctypes.POINTER(Go1SpectrumConfig), ctypes.POINTER(Go1SpectrumBuffers), ctypes.c_int32, ctypes.c_void_p]   # the slot
    return lib


def check_segment(segment_steps):
    """W as an int, refused unless it is even and in [8, 128]"""
    W = int(segment_steps)
    if W != segment_steps or W % 2 or not MIN_SEGMENT <= W <= MAX_SEGMENT:
        raise ValueError(f"spectrum: segment_steps has to be even and in [{MIN_SEGMENT}, {MAX_SEGMENT}], not {segment_steps}")
    return W


def taper_weights(W, taper="hann"):
    """the taper w[t], fp64: periodic Hann, 0.5 - 0.5 cos(2 pi t / W), or boxcar"""
    if taper not in TAPERS:
        raise ValueError(f"spectrum: taper has to be one of {TAPERS}, not {taper!r}")
    t = np.arange(W, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * t / W) if taper == "hann" else np.ones(W)


def twiddle_tables(segment_steps, dt, taper="hann"):
    """{"tw_re": (F, W), "tw_im": (F, W), "scale": (F,), "freq": (F,)} as fp32 arrays, computed in fp64 and rounded once
    (include/go1spectrum.h).  The angle is 2 pi ((k t) mod W) / W: the same angle, with an argument that stays below 2 pi."""
    W = check_segment(segment_steps)
    F, fs = W // 2 + 1, 1.0 / float(dt)
    w = taper_weights(W, taper)
    k, t = np.arange(F, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    angle = 2.0 * np.pi * ((k * t) % W).astype(np.float64) / W
    scale = np.full(F, 2.0 / (fs * (w * w).sum()))
    scale[0] *= 0.5
    scale[F - 1] *= 0.5
    return dict(tw_re=(w * np.cos(angle)).astype(np.float32), tw_im=(-w * np.sin(angle)).astype(np.float32), scale=scale.astype(np.float32),
                freq=(np.arange(F, dtype=np.float64) * fs / W).astype(np.float32))


def first_high_bin(freq, high_freq):
    """the first bin with freq >= high_freq, refused unless it is in [1, F - 1]"""
    at = np.nonzero(np.asarray(freq, np.float64) >= float(high_freq))[0]
    if at.size == 0 or at[0] < 1:
        raise ValueError(f"spectrum: high_freq has to lie in ({0.0}, {float(freq[-1])}] Hz, not {high_freq}")
    return int(at[0])


class Go1Spectrum(_Table):
    """The spectra of one simulator instance: it owns its accumulators ([40 * 5][N]), the ring of the open segment ([W][40][N]), the
    density sums ([40][F][N]) and the counters.  S: the simulator's Go1SimConfig, buffers: its SimBuffers (device tensors), dt: the policy
    step in seconds.  The ring, the density sums and the twiddle tables are sized by arm()."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1spectrum", Go1SpectrumConfig, Go1SpectrumBuffers, _SPECTRUM_INPUTS
    ROWS, TABLE_ROWS = NUM_SIGNALS * NUM_SPECTRUM_METRICS, NUM_SIGNALS * NUM_SPECTRUM_METRICS + 1
    STATE = {"valid": (torch.uint8, ()), "steps": (torch.int32, ()), "resets": (torch.int32, ()), "segments": (torch.int32, ()),
             "segments_dropped": (torch.int32, ()), "psd_segments": (torch.int32, (NUM_SIGNALS,))}   # (uint32 on the device; torch reads the same bits as int32)

    def __init__(self, S, buffers, dt, lib=None):
        super().__init__(S, buffers, lib if lib is not None else load_library())
        self.dt = float(dt)
        self.ring = self.psd_sum = self.psd_table = self.count_table = None
        self.tables, self.device_tables = None, {}
        self.calls = 0
        self._refresh()

    def _refresh(self):
        super()._refresh()
        b = self.buf
        for n in _SPECTRUM_TABLES:
            setattr(b, n, self.device_tables[n].data_ptr() if n in self.device_tables else None)
        b.ring = self.ring.data_ptr() if self.ring is not None else None
        b.psd_sum = self.psd_sum.data_ptr() if self.psd_sum is not None else None
        b.psd_results = self.psd_table.data_ptr() if self.psd_table is not None else None
        b.psd_counts = self.count_table.data_ptr() if self.count_table is not None else None

    def _size_tables(self, G):
        super()._size_tables(G)
        F = self.cfg.segment_steps // 2 + 1
        self.psd_table = torch.zeros(G, NUM_SIGNALS, F, dtype=torch.float64, device=self.device)
        self.count_table = torch.zeros(G, NUM_SIGNALS, dtype=torch.float64, device=self.device)

    def arm(self, groups, warmup_steps=0, segment_steps=100, high_freq=10.0, taper="hann"):
        """as _Table.arm(); sizes the ring and the density sums for segments of `segment_steps` steps and uploads the tables of `taper`;
        high_share counts the bins from the first with freq >= high_freq on.  The segment clock starts at slot 0."""
        W = check_segment(segment_steps)
        F, N = W // 2 + 1, self.num_envs
        self.tables = twiddle_tables(W, self.dt, taper)
        self.high_freq, self.taper = float(high_freq), taper
        c = self.cfg
        c.segment_steps, c.high_bin, c.bin_width = W, first_high_bin(self.tables["freq"], high_freq), float(np.float32(1.0 / self.dt / W))
        self.device_tables = {n: torch.from_numpy(a).to(self.device) for n, a in self.tables.items()}
        if self.ring is None or tuple(self.ring.shape) != (W, NUM_SIGNALS, N):
            self.ring = torch.zeros(W, NUM_SIGNALS, N, dtype=torch.float32, device=self.device)
            self.psd_sum = torch.zeros(NUM_SIGNALS, F, N, dtype=torch.float64, device=self.device)
        self.calls = 0
        super().arm(groups, warmup_steps)

    def accumulate(self):
        """after a step: its forty samples into the ring (one launch, no sync), and after the segment's last slot the fold (one more)"""
        W = self.cfg.segment_steps
        slot = self.calls % W
        self._launch("go1spectrum_record", self.cfg, self.buf, ctypes.c_int32(slot))
        self.calls += 1
        if slot == W - 1:
            self.fold()

    def fold(self):
        """transform and fold the segment the ring holds (accumulate() calls it after slot W - 1)"""
        self._call("go1spectrum_fold")

    def reduce(self):
        """(the result table [G][200 + 1][NUM_FIELDS], the density sums [G][40][F], their segment counts [G][40]) as device tensors
        (one launch, no sync)"""
        return super().reduce(), self.psd_table, self.count_table

    def read(self):
        """{"metrics": {row: (G, 40, 6) array with the columns go1eval_host.FIELD_NAMES}, "groups": (G, 5) array with the columns
        SPECTRUM_GROUP_FIELDS, "psd": (G, 40, F) the mean density (units^2 / Hz; NaN where no segment was folded), "psd_sum": (G, 40, F)
        and "psd_segments": (G, 40) what it is the quotient of, "freq": (F,) Hz, "signals": the forty names, "high_bin", "segment_steps",
        "bin_width", the per-environment state: "valid", "steps", "resets", "segments", "segments_dropped": (N,), "env_psd_segments":
        (40, N), "env_psd_sum": (40, F, N)}: one launch and the device-to-host copies of the tables and the state arrays"""
        table, psd, counts = (t.cpu().numpy() for t in self.reduce())
        rows = table[:, :self.ROWS].reshape(table.shape[0], NUM_SIGNALS, NUM_SPECTRUM_METRICS, table.shape[2])
        with np.errstate(all="ignore"):
            mean = np.where(counts[:, :, None] > 0, psd / counts[:, :, None], np.nan)
        out = dict(metrics={name: rows[:, :, m, :].copy() for m, name in enumerate(SPECTRUM_NAMES)},
                   groups=table[:, self.ROWS, :len(SPECTRUM_GROUP_FIELDS)].copy(), psd=mean, psd_sum=psd.copy(), psd_segments=counts.copy(),
                   freq=self.tables["freq"].astype(np.float64), signals=list(SIGNAL_NAMES), high_bin=int(self.cfg.high_bin),
                   segment_steps=int(self.cfg.segment_steps), bin_width=float(self.cfg.bin_width), env_psd_sum=self.psd_sum.cpu().numpy())
        out.update({("env_" + n if n == "psd_segments" else n): t.cpu().numpy() for n, t in self.state.items()})
        return out
