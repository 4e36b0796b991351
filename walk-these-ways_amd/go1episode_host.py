"""Host side of the episode C-ABI (include/go1episode.h): ctypes mirrors, library loading, and `Go1Episodes`, which owns the
per-environment accumulators, the state of every environment's open episode, the two length histograms and the two result tables of one
simulator instance.

libgo1episode.so is a library of its own (the other table libraries' surfaces stay as they are) whose device code shares
csrc/go1_tables.h with them, and the host side shares as much: `load_library` is `go1eval_host._load` with this module's path, cache,
error class and entry points, and `Go1Episodes` subclasses `go1eval_host._Table` and hands it its own library, so arm / accumulate /
disarm / reduce, the group validation and the launch check are the tables'.  `accumulate()` enqueues one launch; the host reads the
tables when it asks for `read()`.
"""
import ctypes
import math
import os

import numpy as np
import torch

from go1eval_host import _ACCUMULATORS, _Table, _load

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1episode.so")

EPISODE_NAMES = ["step_reward", "length", "fell", "length_fell", "return", "reward_rate", "lin_vel_err", "yaw_vel_err", "discounted_return",
                 "displacement", "path_length"]                                                                      # enum Go1EpisodeMetric
# the columns of "groups": enum Go1EpisodeGroupField, then the first three of enum Go1EpisodeGroupField2
EPISODE_GROUP_FIELDS = ["envs", "steps", "closed", "fell", "timed_out", "open", "cut", "unseen", "open_steps"]
NUM_EPISODE_METRICS, BINS, NUM_HISTS = 11, 16, 3


class Go1EpisodeConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("return_row", ctypes.c_int32),
                ("gamma", ctypes.c_float), ("bin_steps", ctypes.c_int32)]


_EPISODE_INPUTS = ["rew_buf", "reset_buf", "time_out_buf", "episode_length_buf", "root_states", "base_lin_vel", "base_ang_vel", "commands",
                   "episode_sums"]
_EPISODE_STATE = ["age", "whole", "ret", "disc_ret", "disc_w", "first_pos", "prev_pos", "path", "lin_err", "yaw_err", "track_steps", "steps",
                  "closed", "fell", "timed_out", "cut", "unseen", "fall_hist", "timeout_hist"]


class Go1EpisodeBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _EPISODE_INPUTS + _ACCUMULATORS + _EPISODE_STATE + ["group", "results", "hist_results"]]


EXPORTED_SYMBOLS = ["go1episode_clear", "go1episode_accumulate", "go1episode_reduce", "go1episode_version"]

_lib = None


class Go1EpisodeLibraryMissing(RuntimeError):
    pass


def load_library(path=None):
    """Load libgo1episode.so (HIP, gfx950).  Fails loudly: the episode kernels have no CPU fallback."""
    return _load(globals(), path, Go1EpisodeLibraryMissing, "episode metrics", [(EXPORTED_SYMBOLS[:3], Go1EpisodeConfig, Go1EpisodeBuffers)],
                 "go1episode_version")


def bin_edges(bin_steps):
    """the seventeen edges of the sixteen length bins, in steps: bin k holds the episodes of edges[k] < L <= edges[k + 1] steps; the last
    bin is open-ended, its upper edge infinite"""
    return np.concatenate([np.arange(BINS, dtype=np.float64) * int(bin_steps), [np.inf]])


class Go1Episodes(_Table):
    """Whole episodes of one simulator instance: it owns its accumulators ([11][N]), the running state of every environment's open
    episode, and the per-environment length histograms of the episodes that fell and that timed out ([16][N] each).  S: the simulator's
    Go1SimConfig, buffers: its SimBuffers (device tensors).  clear() forgets every open episode: its age is unknown until it is seen
    again."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1episode", Go1EpisodeConfig, Go1EpisodeBuffers, _EPISODE_INPUTS
    ROWS, TABLE_ROWS = NUM_EPISODE_METRICS, NUM_EPISODE_METRICS + 2
    _F, _I = (torch.float32, ()), (torch.int32, ())                          # (uint32 on the device; torch reads the same bits as int32)
    STATE = {"age": _I, "whole": (torch.uint8, ()), "ret": _F, "disc_ret": _F, "disc_w": _F, "first_pos": (torch.float32, (2,)),
             "prev_pos": (torch.float32, (2,)), "path": _F, "lin_err": _F, "yaw_err": _F, "track_steps": _I, "steps": _I, "closed": _I, "fell": _I,
             "timed_out": _I, "cut": _I, "unseen": _I, "fall_hist": (torch.int32, (BINS,)), "timeout_hist": (torch.int32, (BINS,))}

    def __init__(self, S, buffers, gamma=0.99, bin_steps=63, lib=None):
        super().__init__(S, buffers, lib if lib is not None else load_library())
        self.cfg.return_row = int(S.num_rewards)
        self.cfg.gamma, self.cfg.bin_steps = float(gamma), int(bin_steps)
        self.hist_table = None
        self._refresh()

    def _refresh(self):
        super()._refresh()
        self.buf.hist_results = self.hist_table.data_ptr() if self.hist_table is not None else None

    def _size_tables(self, G):
        super()._size_tables(G)
        self.hist_table = torch.zeros(G, NUM_HISTS, BINS, dtype=torch.float64, device=self.device)

    def arm(self, groups, warmup_steps=0, gamma=None, bin_steps=None):
        """as _Table.arm(); a discount in (0, 1] and a bin width of at least one step given here replace the config's"""
        gamma = self.cfg.gamma if gamma is None else float(gamma)
        bin_steps = self.cfg.bin_steps if bin_steps is None else int(bin_steps)
        if not (math.isfinite(gamma) and 0.0 < gamma <= 1.0):
            raise ValueError(f"episodes: gamma has to lie in (0, 1], not {gamma}")
        if bin_steps < 1:
            raise ValueError(f"episodes: bin_steps has to be at least 1, not {bin_steps}")
        self.cfg.gamma, self.cfg.bin_steps = gamma, bin_steps
        super().arm(groups, warmup_steps)

    def reduce(self):
        """(the result table [G][11 + 2][NUM_FIELDS], the histogram table [G][3][16]) as device tensors (one launch, no sync)"""
        return super().reduce(), self.hist_table

    def read(self):
        """{"metrics": {name: (G, 6) array with the columns go1eval_host.FIELD_NAMES}, "groups": (G, 9) array with the columns
        EPISODE_GROUP_FIELDS, "fall_hist", "timeout_hist", "open_hist": (G, 16) episodes per length bin (the open ones by their age: the
        right-censored observations), "bin_edges": (17,) in steps, "gamma", "bin_steps", the per-environment state: "age", "whole", "ret",
        "disc_ret", "disc_w", "path", "lin_err", "yaw_err", "track_steps", "steps", "closed", "fell", "timed_out", "cut", "unseen": (N,),
        "first_pos", "prev_pos": (2, N), "env_fall_hist", "env_timeout_hist": (16, N)}: one launch and the device-to-host copies of the
        tables and the state arrays"""
        table, hist = self.reduce()
        table, hist = table.cpu().numpy(), hist.cpu().numpy()
        groups = np.concatenate([table[:, self.ROWS, :], table[:, self.ROWS + 1, :3]], axis=1)
        out = dict(metrics={name: table[:, m, :].copy() for m, name in enumerate(EPISODE_NAMES)}, groups=groups, fall_hist=hist[:, 0].copy(),
                   timeout_hist=hist[:, 1].copy(), open_hist=hist[:, 2].copy(), bin_edges=bin_edges(self.cfg.bin_steps), gamma=float(self.cfg.gamma),
                   bin_steps=int(self.cfg.bin_steps))
        out.update({("env_" + n if n.endswith("_hist") else n): t.cpu().numpy() for n, t in self.state.items()})
        return out
