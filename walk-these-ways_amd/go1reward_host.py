"""Host side of the reward C-ABI (include/go1reward.h): ctypes mirrors, library loading, and `Go1Reward`, which owns the per-environment
accumulators ([K + 4][N]), the snapshot of the four histories the step's roll destroys, the last step's term table and the two result
tables of one simulator instance.

libgo1reward.so is a library of its own: nothing imports this module until an environment calls start_reward_metrics().  Its device code
is the step kernel's own reward functions (csrc/go1_maps.h) under the step kernel's flags plus csrc/go1_tables.h; the host side is
`go1eval_host._Table` with a handle in front of the calls (the device functions read a configuration block in device memory, which the
handle owns): arm / accumulate / disarm / reduce, the group validation and the launch check are the tables'.
"""
import ctypes
import os

import numpy as np
import torch

import go1sim_abi as abi
from go1eval_host import _ACCUMULATORS, FIELD_NAMES, _Table
from go1sim_host import release

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1reward.so")

REWARD_EXTRA_ROWS = ("sum", "positive", "negative", "total")                       # enum Go1RewardExtraRow
REWARD_GROUP_FIELDS = ["envs", "measured", "reset", "teleported"]                  # enum Go1RewardGroupField
ENVS_PER_BLOCK, TELEPORT_DISTANCE = 64, 1.0


class Go1RewardConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("num_rewards", ctypes.c_int32)]


_REWARD_SNAPSHOT = ["snap_last_last_actions", "snap_last_last_joint_pos_target", "snap_last_dof_vel", "snap_last_contacts"]
_REWARD_LAST = ["last_raw", "last_scaled", "last_valid"]
_REWARD_COUNTS = ["measured", "resets", "teleported"]
_REWARD_STATE = _REWARD_SNAPSHOT + _REWARD_LAST + _REWARD_COUNTS
# what go1reward_accumulate reads of the simulator's buffer table (measured_heights and height_samples may be NULL)
SIM_INPUTS = ["root_states", "base_lin_vel", "base_ang_vel", "projected_gravity", "commands", "torques", "dof_pos", "dof_vel", "actions",
              "joint_pos_target", "contact_forces", "foot_positions", "foot_velocities", "prev_foot_velocities", "foot_indices",
              "desired_contact_states", "last_last_actions", "last_last_joint_pos_target", "last_dof_vel", "last_contacts", "reset_buf",
              "episode_length_buf"]


class Go1RewardBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _ACCUMULATORS + _REWARD_STATE + ["group", "results", "group_results"]]


EXPORTED_SYMBOLS = ["go1reward_create", "go1reward_destroy", "go1reward_arm", "go1reward_snapshot", "go1reward_accumulate", "go1reward_reduce",
                    "go1reward_version"]

_lib = None


class Go1RewardLibraryMissing(RuntimeError):
    pass


def load_library(path=None):
    """Load libgo1reward.so (HIP, gfx950).  Fails loudly: the reward kernels have no CPU fallback.  A library loaded from another path
    is not cached."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise Go1RewardLibraryMissing(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                      f"(hipcc --offload-arch=gfx950). Device-side reward metrics have no CPU fallback.")
    lib = ctypes.CDLL(p)
    vp, ip = ctypes.c_void_p, ctypes.c_int
    lib.go1reward_create.argtypes = [ctypes.POINTER(abi.Go1SimConfig), ctypes.POINTER(abi.Go1SimBuffers), ip, ctypes.POINTER(vp)]
    lib.go1reward_destroy.argtypes = [vp]
    lib.go1reward_arm.argtypes = [vp, ctypes.POINTER(Go1RewardConfig), ctypes.POINTER(Go1RewardBuffers), vp]
    lib.go1reward_snapshot.argtypes = [vp, vp]
    lib.go1reward_accumulate.argtypes = [vp, ctypes.POINTER(ctypes.c_float), vp]
    lib.go1reward_reduce.argtypes = [vp, vp]
    for fn in EXPORTED_SYMBOLS[:-1]:
        getattr(lib, fn).restype = ctypes.c_int
    lib.go1reward_version.restype = ctypes.c_char_p
    if path is None:
        _lib = lib
    return lib


class Go1Reward(_Table):
    """The reward table of one simulator instance.  S: the simulator's Go1SimConfig, buffers: its SimBuffers (device tensors; their
    `struct` is the Go1SimBuffers the handle copies), names: the K term names in the configuration's order (env.reward_names)."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1reward", Go1RewardConfig, Go1RewardBuffers, ()

    def __init__(self, S, buffers, names=None, lib=None):
        K = self.K = int(S.num_rewards)
        self.names = list(names) if names is not None else [f"term_{k}" for k in range(K)]
        assert len(self.names) == K, (len(self.names), K)
        self.scales = np.array([S.reward_scales[k] for k in range(K)], dtype=np.float32)
        self.ROWS = self.TABLE_ROWS = K + len(REWARD_EXTRA_ROWS)
        f, u8, i32 = torch.float32, torch.uint8, torch.int32
        self.STATE = {"snap_last_last_actions": (f, (12,)), "snap_last_last_joint_pos_target": (f, (12,)), "snap_last_dof_vel": (f, (12,)),
                      "snap_last_contacts": (u8, (4,)), "last_raw": (f, (K,)), "last_scaled": (f, (self.ROWS,)), "last_valid": (u8, ()),
                      "measured": (i32, ()), "resets": (i32, ()), "teleported": (i32, ())}   # (uint32 on the device; the same bits)
        super().__init__(S, buffers, lib if lib is not None else load_library())
        self.S = S
        self.cfg.num_rewards = K
        self.group_table = None
        self.accumulated = 0                                                   # accumulate launches since arm()
        self.handle = ctypes.c_void_p()
        # the handle's device block lives where the simulator's buffers live: the index is theirs, not an argument a caller could get wrong
        # (a CPU tensor, under the tests' emulator, has none: 0); the library leaves the thread's current device as it found it
        index = self.device.index if self.device.type == "cuda" else 0
        if index is None:
            index = torch.cuda.current_device()
        self._check(self.lib.go1reward_create(ctypes.byref(S), ctypes.byref(buffers.struct), int(index), ctypes.byref(self.handle)),
                    "go1reward_create")
        self.device_index = int(index)
        self._refresh()

    def _refresh(self):
        super()._refresh()
        self.buf.group_results = self.group_table.data_ptr() if self.group_table is not None else None

    def _size_tables(self, G):
        super()._size_tables(G)
        self.group_table = torch.zeros(G, len(REWARD_GROUP_FIELDS), dtype=torch.float64, device=self.device)

    def clear(self):
        """snapshot, empty accumulators and counts (one launch, no sync); the handle keeps this config and these buffers"""
        self._check(self.lib.go1reward_arm(self.handle, ctypes.byref(self.cfg), ctypes.byref(self.buf), self._stream()), "go1reward_arm")
        self.accumulated = 0

    def snapshot(self):
        """take the snapshot again: after a reset of environments from the host between two steps (one launch, no sync)"""
        self._check(self.lib.go1reward_snapshot(self.handle, self._stream()), "go1reward_snapshot")

    def accumulate(self, gravity):
        """after a step: its terms.  gravity: the three floats of the gravity vector that was in force during the step
        (go1sim_host.gravity_at(S, counter before the step)); one launch, no sync"""
        g = (ctypes.c_float * 3)(*[float(x) for x in gravity])
        self._check(self.lib.go1reward_accumulate(self.handle, g, self._stream()), "go1reward_accumulate")
        self.accumulated += 1

    def reduce(self):
        """(the result table [G][K + 4][NUM_FIELDS], the counts [G][4]) as device tensors (one launch, no sync)"""
        assert self.table is not None, "arm() first"
        self._check(self.lib.go1reward_reduce(self.handle, self._stream()), "go1reward_reduce")
        return self.table, self.group_table

    def last(self):
        """((K + 4, N) scaled terms and sums of the last accumulated step, (N,) uint8 valid): views of the device tensors, no copy"""
        return self.state["last_scaled"], self.state["last_valid"]

    def raw_functions(self):
        """K callables in the names' order, each returning the last step's raw (unscaled) term as an (N,) device tensor: a view, NaN for
        an environment whose last step was not measured"""
        raw = self.state["last_raw"]
        return [(lambda k=k: raw[k]) for k in range(self.K)]

    def read(self):
        """{"names": [K], "scales": (K,), "terms": {name: (G, 6) with the columns go1eval_host.FIELD_NAMES}, "sum", "positive", "negative",
        "total": (G, 6), "share": {name: (G,)} = mean_k / sum_j |mean_j|, "groups": (G, 4) with the columns REWARD_GROUP_FIELDS, and the
        per-environment state ("measured", "resets", "teleported", "last_valid": (N,), "last_raw": (K, N), "last_scaled": (K + 4, N))}:
        one reduction launch and the device-to-host copies"""
        table, groups = self.reduce()
        table, groups = table.cpu().numpy(), groups.cpu().numpy()
        K = self.K
        out = dict(names=list(self.names), scales=self.scales.copy(), terms={n: table[:, k, :].copy() for k, n in enumerate(self.names)},
                   groups=groups.copy())
        for x, n in enumerate(REWARD_EXTRA_ROWS):
            out[n] = table[:, K + x, :].copy()
        means = table[:, :K, FIELD_NAMES.index("mean")]
        out["share"] = shares(means, self.names)
        out.update({n: self.state[n].cpu().numpy() for n in _REWARD_LAST + _REWARD_COUNTS})
        return out

    def __del__(self):
        try:
            if self.handle:
                release(self.lib.go1reward_destroy, self.handle)       # (not inside a stream capture: go1sim_host.release)
                self.handle = None
        except Exception:
            pass


def shares(means, names):
    """{name: (G,)} mean_k / sum_j |mean_j| of a (G, K) table of means; a term without a mean (nothing measured) counts as 0 in the
    denominator and has a NaN share, and a group whose means are all 0 has NaN shares"""
    means = np.asarray(means, dtype=np.float64)
    denom = np.nansum(np.abs(means), axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return {n: np.where(denom > 0, means[:, k] / denom, np.nan) for k, n in enumerate(names)}
