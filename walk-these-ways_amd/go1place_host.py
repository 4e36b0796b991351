"""Host side of the foot-placement C-ABI (include/go1place.h): ctypes mirrors, library loading, and `Go1Place`, which owns the
per-(foot, environment) accumulators, the stance and stride state, the footprint maps and the two result tables of one simulator
instance.

libgo1place.so is a library of its own (the other libraries' surfaces stay as they are) whose device code shares csrc/go1_tables.h
with the other table libraries, and the host side shares as much: `load_library` is `go1eval_host._load` with this module's path,
cache, error class and entry points, and `Go1Place` subclasses `go1eval_host._Table` and hands it its own library, so arm / accumulate /
disarm / reduce, the group validation and the launch check are the tables'.  `accumulate()` enqueues one launch; the host reads the
tables when it asks for `read()`.
"""
import ctypes
import os

import numpy as np
import torch

from go1eval_host import NUM_FIELDS, _ACCUMULATORS, _Table, _load

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1place.so")

PLACE_NAMES = ["stance_err_x", "stance_err_y", "swing_err_x", "swing_err_y", "touchdown_x", "touchdown_y", "touchdown_err_x", "touchdown_err_y",
               "track_width_err", "stride_length", "stride_length_err", "liftoff_x", "liftoff_y", "stance_sweep"]     # enum Go1PlaceMetric
PLACE_GROUP_FIELDS = ["envs", "steps", "resets", "touchdowns", "strides", "map_outside"]                             # enum Go1PlaceGroupField
FOOT_NAMES = ["FL", "FR", "RL", "RR"]                                                                                # the simulator's foot order
NUM_FEET, NUM_PLACE_METRICS, MAP_SIDE, MAP_CELLS, CONTACT_FORCE = 4, 14, 8, 64, 1.0
DEFAULT_MAP_CELL = 0.03        # m: a placeholder, nothing measured stands behind it


class Go1PlaceConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("num_commands", ctypes.c_int32),
                ("map_cell", ctypes.c_float)]


_PLACE_INPUTS = ["commands", "root_states", "foot_positions", "contact_forces", "foot_indices", "reset_buf", "episode_length_buf"]
_PLACE_STATE = ["prev_contact", "stance_open", "stride_open", "td_x", "last_x", "last_y", "td_world_x", "td_world_y", "touchdowns", "liftoffs",
                "strides", "map_outside", "map", "steps", "resets"]


class Go1PlaceBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _PLACE_INPUTS + _ACCUMULATORS + _PLACE_STATE + ["group", "results", "map_results"]]


EXPORTED_SYMBOLS = ["go1place_clear", "go1place_accumulate", "go1place_reduce", "go1place_version"]

_lib = None


class Go1PlaceLibraryMissing(RuntimeError):
    pass


def load_library(path=None):
    """Load libgo1place.so (HIP, gfx950).  Fails loudly: the foot-placement kernels have no CPU fallback."""
    return _load(globals(), path, Go1PlaceLibraryMissing, "foot-placement metrics", [(EXPORTED_SYMBOLS[:3], Go1PlaceConfig, Go1PlaceBuffers)],
                 "go1place_version")


def map_edges(map_cell):
    """the nine edges of the map's eight cells per axis (m from the nominal stance point): cell k covers [(k - 4) cell, (k - 3) cell)"""
    return (np.arange(MAP_SIDE + 1) - MAP_SIDE // 2) * float(np.float32(map_cell))


class Go1Place(_Table):
    """Foot placement of one simulator instance: it owns its accumulators ([4 * 14][N]), the stance and stride state of every foot
    ([4][N]) and the per-environment footprint maps ([4][64][N]).  S: the simulator's Go1SimConfig (its num_commands is the config's),
    buffers: its SimBuffers (device tensors), map_cell: the side of a map cell in metres.  clear() leaves every foot's state unknown."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1place", Go1PlaceConfig, Go1PlaceBuffers, _PLACE_INPUTS
    ROWS, TABLE_ROWS = NUM_FEET * NUM_PLACE_METRICS, NUM_FEET * NUM_PLACE_METRICS + 1
    STATE = {"prev_contact": (torch.uint8, (NUM_FEET,)), "stance_open": (torch.uint8, (NUM_FEET,)), "stride_open": (torch.uint8, (NUM_FEET,)),
             "td_x": (torch.float32, (NUM_FEET,)), "last_x": (torch.float32, (NUM_FEET,)), "last_y": (torch.float32, (NUM_FEET,)),
             "td_world_x": (torch.float32, (NUM_FEET,)), "td_world_y": (torch.float32, (NUM_FEET,)), "touchdowns": (torch.int32, (NUM_FEET,)),
             "liftoffs": (torch.int32, (NUM_FEET,)), "strides": (torch.int32, (NUM_FEET,)), "map_outside": (torch.int32, (NUM_FEET,)),
             "map": (torch.int32, (NUM_FEET, MAP_CELLS)), "steps": (torch.int32, ()),
             "resets": (torch.int32, ())}                                     # (uint32 on the device; torch reads the same bits as int32)

    def __init__(self, S, buffers, map_cell=DEFAULT_MAP_CELL, lib=None):
        super().__init__(S, buffers, lib if lib is not None else load_library())
        self.cfg.num_commands, self.cfg.map_cell = int(S.num_commands), float(map_cell)
        self.map_table = None
        self._refresh()

    def _refresh(self):
        super()._refresh()
        self.buf.map_results = self.map_table.data_ptr() if self.map_table is not None else None

    def _size_tables(self, G):
        super()._size_tables(G)
        self.map_table = torch.zeros(G, NUM_FEET, MAP_CELLS, dtype=torch.float64, device=self.device)

    def arm(self, groups, warmup_steps=0, map_cell=None):
        """as _Table.arm(); a map_cell given here replaces the config's"""
        if map_cell is not None:
            self.cfg.map_cell = float(map_cell)
        super().arm(groups, warmup_steps)

    def reduce(self):
        """(the result table [G][4 * 14 + 1][NUM_FIELDS], the map table [G][4][64]) as device tensors (one launch, no sync)"""
        return super().reduce(), self.map_table

    def read(self):
        """{"metrics": {name: (G, 4, 6) array with the columns go1eval_host.FIELD_NAMES, one row per foot of FOOT_NAMES}, "groups": (G, 6)
        array with the columns PLACE_GROUP_FIELDS, "map": (G, 4, 8, 8) touchdowns per cell, [v][u]: v along y, u along x, "map_edges":
        (9,) metres from the nominal stance point, and the per-environment state: "prev_contact", "stance_open", "stride_open", "td_x",
        "last_x", "last_y", "td_world_x", "td_world_y", "touchdowns", "liftoffs", "strides", "map_outside": (4, N), "steps", "resets":
        (N,), "env_map": (4, 64, N)}: one launch and the device-to-host copies of the tables and the state arrays"""
        table, cells = self.reduce()
        table, cells = table.cpu().numpy(), cells.cpu().numpy()
        rows = table[:, :self.ROWS, :].reshape(-1, NUM_FEET, NUM_PLACE_METRICS, NUM_FIELDS)
        out = dict(metrics={name: rows[:, :, m, :].copy() for m, name in enumerate(PLACE_NAMES)},
                   groups=table[:, self.ROWS, :len(PLACE_GROUP_FIELDS)].copy(), map=cells.reshape(-1, NUM_FEET, MAP_SIDE, MAP_SIDE).copy(),
                   map_edges=map_edges(self.cfg.map_cell))
        out.update({("env_map" if n == "map" else n): t.cpu().numpy() for n, t in self.state.items()})
        return out
