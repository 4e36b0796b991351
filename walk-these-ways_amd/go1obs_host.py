"""Host side of the observation C-ABI (include/go1obs.h): ctypes mirrors, library loading, and `Go1Observations`, which owns the
`value` and `delta` accumulators, the previous values, the bins and tails and the three result tables of one simulator instance.

libgo1obs.so is a library of its own (the other table libraries' surfaces stay as they are) whose device code shares
csrc/go1_tables.h with them, and the host side shares as much: `load_library` is `go1eval_host._load` with this module's path, cache,
error class and entry points, and `Go1Observations` subclasses `go1eval_host._Table` and hands it its own library, so arm / accumulate /
disarm / reduce, the group validation and the launch check are the tables'.  The number of channels is the configuration's, so the
accumulators and the state are sized by arm().  `accumulate()` enqueues one launch; the host reads the tables when it asks for `read()`.
"""
import ctypes
import math
import os

import numpy as np
import torch

from go1eval_host import _ACC_DTYPES, _ACCUMULATORS, _Table, _load

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1obs.so")

MAX_CHANNELS, BINS, NUM_TAILS = 160, 16, 3
TAILS = ["below", "above", "at_clip"]                                         # enum Go1ObsTail
OBS_GROUP_FIELDS = ["envs", "launches", "measured", "resets"]                 # enum Go1ObsGroupField


class Go1ObsConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("num_obs", ctypes.c_int32),
                ("num_privileged_obs", ctypes.c_int32), ("privileged", ctypes.c_int32), ("num_break", ctypes.c_int32), ("clip", ctypes.c_float),
                ("lo", ctypes.c_float * MAX_CHANNELS), ("scale", ctypes.c_float * MAX_CHANNELS)]


_OBS_INPUTS = ["obs_buf", "privileged_obs_buf", "reset_buf"]
_OBS_STATE = ["prev", "age", "hist", "below", "above", "at_clip", "launches", "resets"]
_OBS_TABLES = ["results", "hist_results", "tails"]


class Go1ObsBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _OBS_INPUTS + _ACCUMULATORS + _OBS_STATE + ["break_ids", "group"] + _OBS_TABLES]


EXPORTED_SYMBOLS = ["go1obs_clear", "go1obs_break", "go1obs_accumulate", "go1obs_reduce", "go1obs_version"]

_lib = None


class Go1ObsLibraryMissing(RuntimeError):
    pass


def load_library(path=None):
    """Load libgo1obs.so (HIP, gfx950).  Fails loudly: the observation kernels have no CPU fallback."""
    return _load(globals(), path, Go1ObsLibraryMissing, "observation metrics", [(EXPORTED_SYMBOLS[:4], Go1ObsConfig, Go1ObsBuffers)], "go1obs_version")


def checked_spans(spans):
    """[(lo, hi)] as fp32 pairs; ValueError for a bound that is not finite or a span with hi <= lo (in fp32)"""
    out = []
    for c, (lo, hi) in enumerate(spans):
        lo, hi = np.float32(lo), np.float32(hi)
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f"observations: the range of channel {c} has to be finite, not ({lo}, {hi})")
        if not hi > lo or not math.isfinite(np.float32(BINS) / (hi - lo)):
            raise ValueError(f"observations: the range of channel {c} needs hi > lo, not ({lo}, {hi})")
        out.append((lo, hi))
    return out


def bin_edges(spans):
    """(C, 17): the edges of every channel's sixteen bins.  Bin k holds edges[k] <= v < edges[k + 1] up to the rounding of the kernel's
    fp32 (v - lo) * scale; what lies outside [lo, hi) is in the tails"""
    return np.stack([np.linspace(float(lo), float(hi), BINS + 1) for lo, hi in spans]) if len(spans) else np.zeros((0, BINS + 1))


class Go1Observations(_Table):
    """The observation tables of one simulator instance: it owns the `value` and `delta` rows ([2 C][N]), the previous values and ages
    ([C][N]), the bins ([C][16][N]) and the tails.  S: the simulator's Go1SimConfig, buffers: its SimBuffers (device tensors)."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1obs", Go1ObsConfig, Go1ObsBuffers, _OBS_INPUTS
    _I = torch.int32                                                         # (uint32 on the device; torch reads the same bits as int32)
    PER_CHANNEL = {"prev": (torch.float32, ()), "age": (_I, ()), "hist": (_I, (BINS,)), "below": (_I, ()), "above": (_I, ()), "at_clip": (_I, ())}
    PER_ENV = {"launches": (_I, ()), "resets": (_I, ())}

    def __init__(self, S, buffers, lib=None):
        super().__init__(S, buffers, lib if lib is not None else load_library())       # (ROWS = 0: arm() sizes what depends on C)
        self.num_obs, self.num_privileged_obs = int(S.num_obs), int(S.num_privileged_obs)
        self.cfg.num_obs, self.cfg.num_privileged_obs, self.cfg.clip = self.num_obs, self.num_privileged_obs, float(S.clip_observations)
        self.channels, self.spans, self.privileged = 0, [], False
        self.hist_table = self.tails_table = self._ids = None
        self._size_state(0)
        self._refresh()

    def _size_state(self, C):
        N = self.num_envs
        self.acc = {n: torch.zeros(2 * C, N, dtype=dt, device=self.device) for n, dt in _ACC_DTYPES.items()}
        self.state = {n: torch.zeros(C, *lead, N, dtype=dt, device=self.device) for n, (dt, lead) in self.PER_CHANNEL.items()}
        self.state.update({n: torch.zeros(N, dtype=dt, device=self.device) for n, (dt, _) in self.PER_ENV.items()})

    def _refresh(self):
        super()._refresh()
        for field, table in (("hist_results", self.hist_table), ("tails", self.tails_table)):
            setattr(self.buf, field, table.data_ptr() if table is not None else None)
        self.buf.break_ids = None

    def _size_tables(self, G):
        C = self.channels
        self.table = torch.zeros(G, 2 * C + 1, 6, dtype=torch.float64, device=self.device)
        self.hist_table = torch.zeros(G, C, BINS, dtype=torch.float64, device=self.device)
        self.tails_table = torch.zeros(G, C, NUM_TAILS, dtype=torch.float64, device=self.device)

    def arm(self, groups, warmup_steps=0, spans=None, privileged=True):
        """as _Table.arm().  spans: [(lo, hi)] per channel, the span of its sixteen bins, num_obs of them and, with `privileged`,
        num_privileged_obs more"""
        C = self.num_obs + (self.num_privileged_obs if privileged else 0)
        if not 1 <= C <= MAX_CHANNELS:
            raise ValueError(f"observations: {C} channels, the library takes 1 to {MAX_CHANNELS}")
        spans = checked_spans(spans or [])
        if len(spans) != C:
            raise ValueError(f"observations: {len(spans)} ranges for {C} channels")
        c = self.cfg
        c.privileged = int(bool(privileged))
        for k, (lo, hi) in enumerate(spans):
            c.lo[k], c.scale[k] = lo, np.float32(BINS) / (hi - lo)            # (fp32 throughout, as the header says)
        self.channels, self.spans, self.privileged = C, spans, bool(privileged)
        self._size_state(C)
        super().arm(groups, warmup_steps)

    def note_reset(self, env_ids=None):
        """the environments `env_ids` (None: all) were put elsewhere between two launches: their next launch folds no change (one
        launch, no sync)"""
        if env_ids is None:
            self.buf.break_ids, self.cfg.num_break = None, 0
        else:
            self._ids = torch.as_tensor(env_ids, device=self.device).to(torch.int64).reshape(-1).contiguous()       # (kept until the next call)
            if self._ids.numel() == 0:
                return
            self.buf.break_ids, self.cfg.num_break = self._ids.data_ptr(), int(self._ids.numel())
        self._call(self.PREFIX + "_break")
        self.buf.break_ids, self.cfg.num_break = None, 0

    def reduce(self):
        """(the result table [G][2 C + 1][6], the bins [G][C][16], the tails [G][C][3]) as device tensors (one launch, no sync)"""
        return super().reduce(), self.hist_table, self.tails_table

    def read(self):
        """{"edges": (C, 17), "clip", "privileged", "value", "delta": (G, C, 6) arrays with the columns go1eval_host.FIELD_NAMES, "hist":
        (G, C, 16), "tails": (G, C, 3) below, above, at_clip, "groups": (G, 4) environments, launches, measured env-steps, reset steps,
        and the per-environment state under "env_" + its name}: one launch and the device-to-host copies"""
        C = self.channels
        table, hist, tails = (t.cpu().numpy() for t in self.reduce())
        out = dict(edges=bin_edges(self.spans), clip=float(self.cfg.clip), privileged=self.privileged, value=table[:, :C].copy(),
                   delta=table[:, C:2 * C].copy(), hist=hist.copy(), tails=tails.copy(), groups=table[:, 2 * C, :len(OBS_GROUP_FIELDS)].copy())
        out.update({"env_" + n: t.cpu().numpy() for n, t in self.state.items()})
        return out
