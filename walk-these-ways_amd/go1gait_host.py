"""Host side of the gait C-ABI (include/go1gait.h): ctypes mirrors, library loading, and `Go1Gait`, which owns the per-environment
accumulators, the stride state, the support-pattern and touchdown-phase histograms and the two result tables of one simulator instance.

libgo1gait.so is a library of its own (the evaluation, foot and trunk libraries' surfaces stay as they are) whose device code shares
csrc/go1_tables.h with those three, and the host side shares as much: `load_library` is `go1eval_host._load` with this module's path,
cache, error class and entry points, and `Go1Gait` subclasses `go1eval_host._Table` and hands it its own library, so arm / accumulate /
disarm / reduce, the group validation and the launch check are the tables'.  `accumulate()` enqueues one launch; the host reads the
tables when it asks for `read()`.
"""
import ctypes
import os

import numpy as np
import torch

from go1eval_host import _ACCUMULATORS, _Table, _load

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1gait.so")

FEET = ["FL", "FR", "RL", "RR"]                                                                                      # the simulator's foot order
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]                                                             # the order of the sync rows
GAIT_NAMES = [f"sync_{FEET[i]}_{FEET[j]}" for i, j in PAIRS] + [f"{kind}_{foot}" for kind in ("phase_err", "phase_abs_err", "touchdowns")
                                                                for foot in FEET[1:]]                              # enum Go1GaitMetric
GAIT_GROUP_FIELDS = ["envs", "steps", "resets", "strides", "strides_dropped"]                                        # enum Go1GaitGroupField
NUM_GAIT_METRICS, BINS, NUM_HISTS, CONTACT_FORCE = 15, 16, 4, 1.0
# the sixteen support patterns, bin = mask = sum of c_f << f: "-" for flight, else the feet on the ground
SUPPORT_PATTERNS = ["+".join(FEET[f] for f in range(4) if mask >> f & 1) or "-" for mask in range(BINS)]


class Go1GaitConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("min_stride_steps", ctypes.c_int32),
                ("max_stride_steps", ctypes.c_int32)]


_GAIT_INPUTS = ["contact_forces", "foot_indices", "reset_buf", "episode_length_buf"]
_GAIT_STATE = ["prev_contact", "ref_steps", "last_td", "td_count", "steps", "resets", "strides", "strides_dropped", "support_hist", "phase_hist"]


class Go1GaitBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _GAIT_INPUTS + _ACCUMULATORS + _GAIT_STATE + ["group", "results", "hist_results"]]


EXPORTED_SYMBOLS = ["go1gait_clear", "go1gait_accumulate", "go1gait_reduce", "go1gait_version"]

_lib = None


class Go1GaitLibraryMissing(RuntimeError):
    pass


def load_library(path=None):
    """Load libgo1gait.so (HIP, gfx950).  Fails loudly: the gait kernels have no CPU fallback."""
    return _load(globals(), path, Go1GaitLibraryMissing, "gait metrics", [(EXPORTED_SYMBOLS[:3], Go1GaitConfig, Go1GaitBuffers)],
                 "go1gait_version")


def phase_centres():
    """the centres of the sixteen touchdown-phase bins (cycles): bin k is centred on k / 16; bin 0 covers [31/32, 1) and [0, 1/32)"""
    return np.arange(BINS) / float(BINS)


class Go1Gait(_Table):
    """Inter-leg coordination of one simulator instance: it owns its accumulators ([15][N]), the previous contacts and the open reference
    stride of every environment, and the per-environment support-pattern ([16][N]) and touchdown-phase ([3][16][N]) histograms.  S: the
    simulator's Go1SimConfig, buffers: its SimBuffers (device tensors).  clear() forgets the contacts and the open strides."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1gait", Go1GaitConfig, Go1GaitBuffers, _GAIT_INPUTS
    ROWS, TABLE_ROWS = NUM_GAIT_METRICS, NUM_GAIT_METRICS + 1
    STATE = {"prev_contact": (torch.uint8, (4,)), "ref_steps": (torch.int32, ()), "last_td": (torch.int32, (3,)), "td_count": (torch.int32, (3,)),
             "steps": (torch.int32, ()), "resets": (torch.int32, ()), "strides": (torch.int32, ()), "strides_dropped": (torch.int32, ()),
             "support_hist": (torch.int32, (BINS,)), "phase_hist": (torch.int32, (3, BINS))}     # (uint32 on the device; torch reads the same bits as int32)

    def __init__(self, S, buffers, min_stride_steps=1, max_stride_steps=100, lib=None):
        super().__init__(S, buffers, lib if lib is not None else load_library())
        self.cfg.min_stride_steps, self.cfg.max_stride_steps = int(min_stride_steps), int(max_stride_steps)
        self.hist_table = None
        self._refresh()

    def _refresh(self):
        super()._refresh()
        self.buf.hist_results = self.hist_table.data_ptr() if self.hist_table is not None else None

    def _size_tables(self, G):
        super()._size_tables(G)
        self.hist_table = torch.zeros(G, NUM_HISTS, BINS, dtype=torch.float64, device=self.device)

    def arm(self, groups, warmup_steps=0, min_stride_steps=None, max_stride_steps=None):
        """as _Table.arm(); stride limits given here replace the config's"""
        if min_stride_steps is not None:
            self.cfg.min_stride_steps = int(min_stride_steps)
        if max_stride_steps is not None:
            self.cfg.max_stride_steps = int(max_stride_steps)
        super().arm(groups, warmup_steps)

    def reduce(self):
        """(the result table [G][15 + 1][NUM_FIELDS], the histogram table [G][4][16]) as device tensors (one launch, no sync)"""
        return super().reduce(), self.hist_table

    def read(self):
        """{"metrics": {name: (G, 6) array with the columns go1eval_host.FIELD_NAMES}, "groups": (G, 5) array with the columns
        GAIT_GROUP_FIELDS, "support_hist": (G, 16) steps per support pattern (SUPPORT_PATTERNS), "phase_hist": (G, 3, 16) closed strides
        per touchdown-phase bin of FR, RL, RR, "phase_centres": (16,), "support_patterns", the per-environment state: "ref_steps", "steps",
        "resets", "strides", "strides_dropped": (N,), "prev_contact": (4, N), "last_td", "td_count": (3, N), "env_support_hist": (16, N),
        "env_phase_hist": (3, 16, N)}: one launch and the device-to-host copies of the tables and the state arrays"""
        table, hist = self.reduce()
        table, hist = table.cpu().numpy(), hist.cpu().numpy()
        out = dict(metrics={name: table[:, m, :].copy() for m, name in enumerate(GAIT_NAMES)},
                   groups=table[:, self.ROWS, :len(GAIT_GROUP_FIELDS)].copy(), support_hist=hist[:, 0].copy(), phase_hist=hist[:, 1:].copy(),
                   phase_centres=phase_centres(), support_patterns=list(SUPPORT_PATTERNS))
        out.update({("env_" + n if n.endswith("_hist") else n): t.cpu().numpy() for n, t in self.state.items()})
        return out
