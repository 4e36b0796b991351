"""Host side of the foot-loading C-ABI (include/go1feet.h): ctypes mirrors, library loading, and `Go1Feet`, which owns the
per-(foot, environment) accumulators, the stance state, the GRF profile and the three result tables of one simulator instance.

libgo1feet.so is a library of its own (the evaluation library's surface stays as it is) whose device code shares
csrc/go1_tables.h with the evaluation and trunk libraries, and the host side shares as much: `load_library` is
`go1eval_host._load` with this module's path, cache, error class and entry points, and `Go1Feet` subclasses `go1eval_host._Table`
and hands it its own library, so arm / accumulate / disarm / reduce, the group validation and the launch check are the tables'.
`accumulate()` enqueues one launch; the host reads the tables when it asks for `read()`.
"""
import ctypes
import os

import numpy as np
import torch

from go1eval_host import NUM_FIELDS, _ACCUMULATORS, _Table, _load

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1feet.so")

FEET_NAMES = ["contact", "force_normal", "force_tangent", "friction_use", "force_excess", "impact_vel_sq", "touchdown_speed",
              "touchdown_force", "stance_peak_force", "stance_impulse", "stance_slip", "stance_time"]                 # enum Go1FeetMetric
STEP_NAMES, TOUCHDOWN_NAMES, STANCE_NAMES = FEET_NAMES[:6], FEET_NAMES[6:8], FEET_NAMES[8:]     # folded per step / at a touchdown / at a lift-off
FEET_GROUP_FIELDS = ["envs", "steps", "resets"]                                                                      # enum Go1FeetGroupField
FOOT_NAMES = ["FL", "FR", "RL", "RR"]                                                                                # the simulator's foot order
NUM_FEET, NUM_FEET_METRICS, PHASE_BINS, CONTACT_FORCE = 4, 12, 16, 1.0


class Go1FeetConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("dt", ctypes.c_float),
                ("terrain_friction", ctypes.c_float), ("max_contact_force", ctypes.c_float)]


_FEET_INPUTS = ["contact_forces", "foot_velocities", "prev_foot_velocities", "foot_indices", "friction_coeffs", "reset_buf", "episode_length_buf"]
_FEET_STATE = ["prev_contact", "stance_valid", "stance_steps", "stance_peak", "stance_impulse", "stance_slip", "steps", "resets",
               "profile_sum", "profile_count"]


class Go1FeetBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _FEET_INPUTS + _ACCUMULATORS + _FEET_STATE + ["group", "results", "profile_results"]]


EXPORTED_SYMBOLS = ["go1feet_clear", "go1feet_accumulate", "go1feet_reduce", "go1feet_version"]

_lib = None


class Go1FeetLibraryMissing(RuntimeError):
    pass


def load_library(path=None):
    """Load libgo1feet.so (HIP, gfx950).  Fails loudly: the foot-loading kernels have no CPU fallback."""
    return _load(globals(), path, Go1FeetLibraryMissing, "foot-loading metrics", [(EXPORTED_SYMBOLS[:3], Go1FeetConfig, Go1FeetBuffers)],
                 "go1feet_version")


def phase_edges():
    """the seventeen edges of the sixteen phase bins: bin k covers [k / 16, (k + 1) / 16)"""
    return np.arange(PHASE_BINS + 1) / float(PHASE_BINS)


class Go1Feet(_Table):
    """Foot loading of one simulator instance: it owns its accumulators ([4 * 12][N]), the stance state of every foot ([4][N]) and the
    per-environment GRF profile ([4][16][N]).  S: the simulator's Go1SimConfig (its terrain_friction and max_contact_force are the
    config's), buffers: its SimBuffers (device tensors), dt: the policy step in seconds.  clear() leaves every foot's state unknown."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1feet", Go1FeetConfig, Go1FeetBuffers, _FEET_INPUTS
    ROWS, TABLE_ROWS = NUM_FEET * NUM_FEET_METRICS, NUM_FEET * NUM_FEET_METRICS + 1
    STATE = {"prev_contact": (torch.uint8, (NUM_FEET,)), "stance_valid": (torch.uint8, (NUM_FEET,)), "stance_steps": (torch.int32, (NUM_FEET,)),
             "stance_peak": (torch.float32, (NUM_FEET,)), "stance_impulse": (torch.float32, (NUM_FEET,)), "stance_slip": (torch.float32, (NUM_FEET,)),
             "steps": (torch.int32, ()), "resets": (torch.int32, ()), "profile_sum": (torch.float64, (NUM_FEET, PHASE_BINS)),
             "profile_count": (torch.int32, (NUM_FEET, PHASE_BINS))}          # (uint32 on the device; torch reads the same bits as int32)

    def __init__(self, S, buffers, dt, lib=None):
        super().__init__(S, buffers, lib if lib is not None else load_library())
        c = self.cfg
        c.dt, c.terrain_friction, c.max_contact_force = float(dt), float(S.terrain_friction), float(S.max_contact_force)
        self.profile_table = None
        self._refresh()

    def _refresh(self):
        super()._refresh()
        self.buf.profile_results = self.profile_table.data_ptr() if self.profile_table is not None else None

    def _size_tables(self, G):
        super()._size_tables(G)
        self.profile_table = torch.zeros(G, NUM_FEET, PHASE_BINS, 2, dtype=torch.float64, device=self.device)

    def reduce(self):
        """(the result table [G][4 * 12 + 1][NUM_FIELDS], the profile table [G][4][16][2]: sum, count) as device tensors (one launch, no sync)"""
        return super().reduce(), self.profile_table

    def read(self):
        """{"metrics": {name: (G, 4, 6) array with the columns go1eval_host.FIELD_NAMES, one row per foot of FOOT_NAMES}, "groups": (G, 3) array with the
        columns FEET_GROUP_FIELDS, "profile": (G, 4, 16) mean vertical force per phase bin (NaN where nothing was sampled),
        "profile_sum", "profile_count": (G, 4, 16), "phase_edges": (17,), and the per-environment state: "prev_contact", "stance_valid",
        "stance_steps", "stance_peak", "stance_impulse", "stance_slip": (4, N), "steps", "resets": (N,), "env_profile_sum",
        "env_profile_count": (4, 16, N)}: one launch and the device-to-host copies of the tables and the state arrays"""
        table, profile = self.reduce()
        table, profile = table.cpu().numpy(), profile.cpu().numpy()
        rows = table[:, :self.ROWS, :].reshape(-1, NUM_FEET, NUM_FEET_METRICS, NUM_FIELDS)
        total, count = profile[..., 0].copy(), profile[..., 1].copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(count > 0, total / count, np.nan)
        out = dict(metrics={name: rows[:, :, m, :].copy() for m, name in enumerate(FEET_NAMES)},
                   groups=table[:, self.ROWS, :len(FEET_GROUP_FIELDS)].copy(), profile=mean, profile_sum=total, profile_count=count,
                   phase_edges=phase_edges())
        out.update({("env_" + n if n.startswith("profile") else n): t.cpu().numpy() for n, t in self.state.items()})
        return out
