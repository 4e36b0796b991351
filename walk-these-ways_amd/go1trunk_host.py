"""Host side of the trunk C-ABI (include/go1trunk.h): ctypes mirrors, library loading, and `Go1Trunk`, which owns the per-environment
accumulators, the velocity and segment state, the tilt histogram and the two result tables of one simulator instance.

libgo1trunk.so is a library of its own (the evaluation library's and the foot library's surfaces stay as they are) whose device code
shares csrc/go1_tables.h with those two, and the host side shares as much: `load_library` is `go1eval_host._load` with this module's
path, cache, error class and entry points, and `Go1Trunk` subclasses `go1eval_host._Table` and hands it its own library, so arm /
accumulate / disarm / reduce, the group validation and the launch check are the tables'.  `accumulate()` enqueues one launch; the host
reads the tables when it asks for `read()`.
"""
import ctypes
import os

import numpy as np
import torch

from go1eval_host import _ACCUMULATORS, _Table, _load

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1trunk.so")

TRUNK_NAMES = ["roll_sin", "pitch_sin", "tilt", "tilt_exceeded", "roll_rate", "pitch_rate", "vertical_vel", "accel_horizontal", "accel_vertical",
               "ang_accel", "support_feet", "support_margin", "margin_negative", "support_line_dist", "lateral_drift", "heading_drift",
               "progress_err"]                                                                                       # enum Go1TrunkMetric
TRUNK_GROUP_FIELDS = ["envs", "steps", "resets", "segments_dropped"]                                                 # enum Go1TrunkGroupField
NUM_TRUNK_METRICS, TILT_BINS, TILT_BIN_WIDTH, CONTACT_FORCE = 17, 16, 1.0 / 32.0, 1.0


class Go1TrunkConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("segment_steps", ctypes.c_int32),
                ("dt", ctypes.c_float), ("tilt_limit", ctypes.c_float)]


_TRUNK_INPUTS = ["root_states", "base_lin_vel", "base_ang_vel", "projected_gravity", "commands", "contact_forces", "foot_positions", "reset_buf",
                 "episode_length_buf"]
_TRUNK_STATE = ["prev_valid", "prev_lin_vel", "prev_ang_vel", "seg_valid", "seg_steps", "seg_anchor", "seg_command", "segments_dropped", "steps",
                "resets", "tilt_hist"]


class Go1TrunkBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _TRUNK_INPUTS + _ACCUMULATORS + _TRUNK_STATE + ["group", "results", "hist_results"]]


EXPORTED_SYMBOLS = ["go1trunk_clear", "go1trunk_accumulate", "go1trunk_reduce", "go1trunk_version"]

_lib = None


class Go1TrunkLibraryMissing(RuntimeError):
    pass


def load_library(path=None):
    """Load libgo1trunk.so (HIP, gfx950).  Fails loudly: the trunk kernels have no CPU fallback."""
    return _load(globals(), path, Go1TrunkLibraryMissing, "trunk metrics", [(EXPORTED_SYMBOLS[:3], Go1TrunkConfig, Go1TrunkBuffers)],
                 "go1trunk_version")


def tilt_edges():
    """the seventeen edges of the sixteen tilt bins (sines): bin k covers [k / 32, (k + 1) / 32); the last one has no upper edge"""
    edges = np.arange(TILT_BINS + 1) * TILT_BIN_WIDTH
    edges[-1] = np.inf
    return edges


class Go1Trunk(_Table):
    """Trunk motion of one simulator instance: it owns its accumulators ([17][N]), the previous velocities and the open drift segment of
    every environment, and the per-environment tilt histogram ([16][N]).  S: the simulator's Go1SimConfig, buffers: its SimBuffers
    (device tensors), dt: the policy step in seconds.  clear() forgets the previous velocities and the open segments."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1trunk", Go1TrunkConfig, Go1TrunkBuffers, _TRUNK_INPUTS
    ROWS, TABLE_ROWS = NUM_TRUNK_METRICS, NUM_TRUNK_METRICS + 1
    STATE = {"prev_valid": (torch.uint8, ()), "prev_lin_vel": (torch.float32, (3,)), "prev_ang_vel": (torch.float32, (3,)),
             "seg_valid": (torch.uint8, ()), "seg_steps": (torch.int32, ()), "seg_anchor": (torch.float32, (4,)),
             "seg_command": (torch.float32, (2,)), "segments_dropped": (torch.int32, ()), "steps": (torch.int32, ()), "resets": (torch.int32, ()),
             "tilt_hist": (torch.int32, (TILT_BINS,))}                        # (uint32 on the device; torch reads the same bits as int32)

    def __init__(self, S, buffers, dt, segment_steps=50, tilt_limit=0.25, lib=None):
        super().__init__(S, buffers, lib if lib is not None else load_library())
        c = self.cfg
        c.dt, c.segment_steps, c.tilt_limit = float(dt), int(segment_steps), float(tilt_limit)
        self.hist_table = None
        self._refresh()

    def _refresh(self):
        super()._refresh()
        self.buf.hist_results = self.hist_table.data_ptr() if self.hist_table is not None else None

    def _size_tables(self, G):
        super()._size_tables(G)
        self.hist_table = torch.zeros(G, TILT_BINS, dtype=torch.float64, device=self.device)

    def arm(self, groups, warmup_steps=0, segment_steps=None, tilt_limit=None):
        """as _Table.arm(); a segment length or a tilt limit given here replaces the config's"""
        if segment_steps is not None:
            self.cfg.segment_steps = int(segment_steps)
        if tilt_limit is not None:
            self.cfg.tilt_limit = float(tilt_limit)
        super().arm(groups, warmup_steps)

    def reduce(self):
        """(the result table [G][17 + 1][NUM_FIELDS], the histogram table [G][16]) as device tensors (one launch, no sync)"""
        return super().reduce(), self.hist_table

    def read(self):
        """{"metrics": {name: (G, 6) array with the columns go1eval_host.FIELD_NAMES}, "groups": (G, 4) array with the columns
        TRUNK_GROUP_FIELDS, "tilt_hist": (G, 16) counts, "tilt_edges": (17,), the per-environment state: "prev_valid", "seg_valid",
        "seg_steps", "segments_dropped", "steps", "resets": (N,), "prev_lin_vel", "prev_ang_vel": (3, N), "seg_anchor": (4, N),
        "seg_command": (2, N), "env_tilt_hist": (16, N), and "env_max_tilt": (N,) the largest tilt every environment folded (-inf where it
        folded none)}: one launch and the device-to-host copies of the tables and the state arrays"""
        table, hist = self.reduce()
        table, hist = table.cpu().numpy(), hist.cpu().numpy()
        out = dict(metrics={name: table[:, m, :].copy() for m, name in enumerate(TRUNK_NAMES)},
                   groups=table[:, self.ROWS, :len(TRUNK_GROUP_FIELDS)].copy(), tilt_hist=hist.copy(), tilt_edges=tilt_edges())
        out.update({("env_" + n if n == "tilt_hist" else n): t.cpu().numpy() for n, t in self.state.items()})
        out["env_max_tilt"] = self.acc["max"][TRUNK_NAMES.index("tilt")].cpu().numpy()
        return out
