"""Host side of the evaluation-metrics C-ABI (include/go1eval.h): ctypes mirror, library loading, and `Go1Eval`, which owns
the per-environment accumulators and the result table of one simulator instance.

Replaces calling the reference's go1_gym_learn/eval_metrics/metrics.py functions (each ends in `.cpu()`) after every step:
`accumulate()` enqueues one launch and the host reads one small table when it asks for `results()`.  `Go1Behaviour` is the
second table (gait and behaviour tracking); `Go1Trace` records a per-step time series of chosen environments on the device and
analyses the step response to a command switch there (what the reference's scripts/play.py reads to the host step by step).
`Go1Push` adds a chosen velocity step to the base of chosen environments with one launch, and `Go1Trace.recovery` analyses the
trace that follows it (fall, peak velocity error, recovery time, ...).  `Go1Terrain` is the fifth family: whether a robot leaves the
terrain tile it was placed on, falls or times out first, and its height, foot clearance, stumbles and collisions above the ground
it is over, from the simulator's own height field.  `Go1Joints` is the sixth: ten values per joint and step (torque, speed,
acceleration, driving and braking power, soft-limit excess, saturation at the torque clip and at the URDF's speed limit) and a
torque-speed histogram per joint.

What the families share is written once: `load_library` declares the entry points from one table (`_ENTRY_POINTS`); `_Host` holds
the library, the simulator's buffers and how a launch is made and checked; `_Table` is the accumulating family (accumulators,
per-environment state, groups and result table, arm / accumulate / disarm / reduce), which `Go1Eval`, `Go1Behaviour`, `Go1Terrain`
and `Go1Joints` describe with a few class attributes; `_groups` and `_env_ids` are the two host-side validations; and
`Go1Trace._analysis` is the shared back half of the response and the recovery.
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1eval.so")

METRIC_NAMES = ["lin_vel_rmsd", "ang_vel_rmsd", "lin_vel_x", "ang_vel_yaw", "base_height", "max_torques", "power_consumption",
                "CoT", "froude_number", "termination"]                                        # enum Go1EvalMetric
FIELD_NAMES = ["count", "mean", "std", "min", "max", "nonfinite"]                             # enum Go1EvalField
GROUP_FIELD_NAMES = ["envs", "steps", "episodes_terminated", "episodes_timed_out", "fall_rate"]   # enum Go1EvalGroupField
NUM_METRICS, NUM_FIELDS, REDUCE_THREADS = 10, 6, 256
DEFAULT_BODY_MASS = 4.801          # LeggedRobot.default_body_mass


class Go1EvalConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("num_height_points", ctypes.c_int32), ("warmup_steps", ctypes.c_int32),
                ("num_groups", ctypes.c_int32), ("default_body_mass", ctypes.c_float)]


_INPUTS = ["base_lin_vel", "base_ang_vel", "commands", "root_states", "measured_heights", "torques", "dof_vel", "payloads",
           "reset_buf", "time_out_buf", "episode_length_buf"]
_ACCUMULATORS = ["count", "sum", "sumsq", "min", "max", "nonfinite"]
_PER_ENV = ["steps", "episodes_terminated", "episodes_timed_out"]


class Go1EvalBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _INPUTS + _ACCUMULATORS + _PER_ENV + ["group", "results"]]


# ---- the behaviour table (gait and behaviour tracking; include/go1eval.h, second kernel family)
BEHAVIOUR_NAMES = ["contact_match", "body_height_err", "orientation_err", "feet_clearance", "raibert_heuristic", "feet_slip",
                   "action_rate", "step_frequency_err", "duty_factor_err", "swing_height_err"]       # enum Go1BehaviourMetric
STRIDE_NAMES = BEHAVIOUR_NAMES[7:]            # folded at a touchdown, not every step
NUM_BEHAVIOUR = 10


class Go1BehaviourConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("num_commands", ctypes.c_int32), ("num_height_points", ctypes.c_int32),
                ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("dt", ctypes.c_float),
                ("base_height_target", ctypes.c_float)]


_BEHAVIOUR_INPUTS = ["commands", "root_states", "measured_heights", "contact_forces", "foot_positions", "foot_velocities",
                     "desired_contact_states", "foot_indices", "last_actions", "last_last_actions", "reset_buf", "episode_length_buf"]
_STRIDE_STATE = ["prev_contact", "stride_steps", "stance_steps", "swing_peak"]


class Go1BehaviourBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _BEHAVIOUR_INPUTS + _ACCUMULATORS + _STRIDE_STATE + ["group", "results"]]


# ---- the trace and the step response (include/go1eval.h, third kernel family)
TRACE_CHANNELS = ["lin_vel_x", "lin_vel_y", "ang_vel_yaw", "base_height", "contact_match", "power_consumption", "cmd_lin_vel_x",
                  "cmd_lin_vel_y", "cmd_ang_vel_yaw", "cmd_base_height", "max_torques", "reset"] + [f"dof_pos_{j}" for j in range(12)]   # enum Go1TraceChannel
RESPONSE_METRICS = ["reached", "rise_time", "overshoot", "settled", "settling_time", "steady_state_err", "iae"]       # enum Go1ResponseMetric
RESPONSE_GROUP_FIELDS = ["envs", "ok", "reset", "not_held"]                                                          # enum Go1ResponseGroupField
NUM_TRACE, NUM_RESPONSE, MAX_SIGNALS = 24, 7, 8


class Go1TraceConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("num_traced", ctypes.c_int32), ("capacity", ctypes.c_int32),
                ("num_height_points", ctypes.c_int32), ("base_height_target", ctypes.c_float)]


_TRACE_INPUTS = ["base_lin_vel", "base_ang_vel", "commands", "root_states", "measured_heights", "contact_forces", "desired_contact_states",
                 "torques", "dof_vel", "dof_pos", "reset_buf"]


class Go1TraceBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _TRACE_INPUTS + ["env_ids", "trace"]]


class Go1ResponseSignal(ctypes.Structure):
    _fields_ = [("y_channel", ctypes.c_int32), ("r_channel", ctypes.c_int32), ("fixed_target", ctypes.c_float), ("fixed_scale", ctypes.c_float)]


class Go1ResponseConfig(ctypes.Structure):
    _fields_ = [("num_traced", ctypes.c_int32), ("rows", ctypes.c_int32), ("switch_row", ctypes.c_int32), ("pre", ctypes.c_int32),
                ("smooth", ctypes.c_int32), ("hold", ctypes.c_int32), ("tail", ctypes.c_int32), ("band", ctypes.c_float),
                ("dt", ctypes.c_float), ("num_signals", ctypes.c_int32), ("num_groups", ctypes.c_int32),
                ("signal", Go1ResponseSignal * MAX_SIGNALS)]


class Go1ResponseBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ["trace", "values", "status", "group", "results"]]


# ---- the push and the disturbance recovery (include/go1eval.h, fourth kernel family)
PUSH_ROWS = ["forward", "left", "up", "yaw_rate"]                                                                    # enum Go1PushRow
RECOVERY_METRICS = ["fell", "peak_vel_err", "peak_time", "recovered", "recovery_time", "height_drop", "yaw_rate_dev", "iae_excess"]   # enum Go1RecoveryMetric
RECOVERY_STATUS = ["ok", "baseline_reset", "not_held", "fell"]                                                       # enum Go1RecoveryStatus
RECOVERY_GROUP_FIELDS = ["envs", "ok", "baseline_reset", "not_held", "fell"]                                         # enum Go1RecoveryGroupField
NUM_PUSH, NUM_RECOVERY = 4, 8


class Go1PushConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("num_pushed", ctypes.c_int32)]


class Go1PushBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ["root_states", "env_ids", "push"]]


class Go1RecoveryConfig(ctypes.Structure):
    _fields_ = [("num_traced", ctypes.c_int32), ("rows", ctypes.c_int32), ("push_row", ctypes.c_int32), ("pre", ctypes.c_int32),
                ("smooth", ctypes.c_int32), ("hold", ctypes.c_int32), ("band", ctypes.c_float), ("dt", ctypes.c_float),
                ("num_groups", ctypes.c_int32)]


class Go1RecoveryBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ["trace", "values", "status", "group", "results"]]


# ---- terrain traversal (include/go1eval.h, fifth kernel family)
TERRAIN_NAMES = ["base_height_terrain", "feet_clearance_terrain", "swing_foot_height", "stumble", "collision"]         # enum Go1TerrainMetric
TERRAIN_STATUS = ["running", "traversed", "fell", "timed_out"]                                                       # enum Go1TerrainStatus
TERRAIN_OUTCOMES = ["traversed", "fell", "distance", "end_time"]                                                     # enum Go1TerrainOutcome
TERRAIN_GROUP_FIELDS = ["envs", "running", "traversed", "fell", "timed_out", "success_rate"]                         # enum Go1TerrainGroupField
NUM_TERRAIN, NUM_OUTCOME = 5, 4


class Go1TerrainConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("hf_rows", ctypes.c_int32),
                ("hf_cols", ctypes.c_int32), ("penalised_body_mask", ctypes.c_uint32), ("dt", ctypes.c_float), ("hf_hscale", ctypes.c_float),
                ("hf_vscale", ctypes.c_float), ("hf_border", ctypes.c_float), ("tile_length", ctypes.c_float), ("tile_width", ctypes.c_float)]


_TERRAIN_INPUTS = ["root_states", "commands", "contact_forces", "foot_positions", "desired_contact_states", "foot_indices", "env_origins",
                   "height_samples", "reset_buf", "time_out_buf", "episode_length_buf"]
_TERRAIN_STATE = ["status", "steps", "end_step", "max_dist"]


class Go1TerrainBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _TERRAIN_INPUTS + _ACCUMULATORS + _TERRAIN_STATE + ["group", "results"]]


# ---- per-joint actuator usage (include/go1eval.h, sixth kernel family)
JOINT_NAMES = ["torque_abs", "torque_sq", "vel_abs", "vel_sq", "acc_sq", "power_pos", "power_neg", "pos_limit_excess", "torque_saturated",
               "vel_saturated"]                                                                                      # enum Go1JointMetric
JOINT_GROUP_FIELDS = ["envs", "steps", "resets"]                                                                     # enum Go1JointGroupField
DOF_NAMES = [f"{leg}_{part}_joint" for leg in ("FL", "FR", "RL", "RR") for part in ("hip", "thigh", "calf")]         # the simulator's joint order
NUM_DOF, NUM_JOINT, JOINT_TAU_BINS, JOINT_VEL_BINS = 12, 10, 8, 8


class Go1JointConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("dt", ctypes.c_float),
                ("soft_torque_limit", ctypes.c_float), ("soft_vel_limit", ctypes.c_float), ("torque_limit", ctypes.c_float * 12),
                ("vel_limit", ctypes.c_float * 12), ("pos_lower", ctypes.c_float * 12), ("pos_upper", ctypes.c_float * 12)]


_JOINT_INPUTS = ["torques", "dof_vel", "dof_pos", "reset_buf", "episode_length_buf"]
_JOINT_STATE = ["prev_dof_vel", "steps", "resets", "hist"]


class Go1JointBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _JOINT_INPUTS + _ACCUMULATORS + _JOINT_STATE + ["group", "results", "hist_results"]]


EXPORTED_SYMBOLS = ["go1eval_clear", "go1eval_accumulate", "go1eval_reduce", "go1eval_version",
                    "go1eval_behaviour_clear", "go1eval_behaviour_accumulate", "go1eval_behaviour_reduce",
                    "go1eval_trace_record", "go1eval_response", "go1eval_response_reduce",
                    "go1eval_push", "go1eval_recovery", "go1eval_recovery_reduce",
                    "go1eval_terrain_clear", "go1eval_terrain_accumulate", "go1eval_terrain_reduce",
                    "go1eval_joint_clear", "go1eval_joint_accumulate", "go1eval_joint_reduce"]

# (entry points, config, buffers): each is f(const config*, const buffers*, void* stream) -> int; go1eval_trace_record alone takes
# the row (int32) in front of the stream
_ENTRY_POINTS = [(("go1eval_clear", "go1eval_accumulate", "go1eval_reduce"), Go1EvalConfig, Go1EvalBuffers),
                 (("go1eval_behaviour_clear", "go1eval_behaviour_accumulate", "go1eval_behaviour_reduce"), Go1BehaviourConfig, Go1BehaviourBuffers),
                 (("go1eval_trace_record",), Go1TraceConfig, Go1TraceBuffers),
                 (("go1eval_response", "go1eval_response_reduce"), Go1ResponseConfig, Go1ResponseBuffers),
                 (("go1eval_push",), Go1PushConfig, Go1PushBuffers),
                 (("go1eval_recovery", "go1eval_recovery_reduce"), Go1RecoveryConfig, Go1RecoveryBuffers),
                 (("go1eval_terrain_clear", "go1eval_terrain_accumulate", "go1eval_terrain_reduce"), Go1TerrainConfig, Go1TerrainBuffers),
                 (("go1eval_joint_clear", "go1eval_joint_accumulate", "go1eval_joint_reduce"), Go1JointConfig, Go1JointBuffers)]

_lib = None


class Go1EvalLibraryMissing(RuntimeError):
    pass


def _load(module, path, missing, what, entry_points, version):
    """The loader of the three metric libraries.  module: the caller's globals(), whose LIB_PATH is the default path and whose _lib
    caches the library loaded from it (a library loaded from another path is not cached); missing(...) is raised for an absent file,
    `what` names in its message what has no CPU fallback; entry_points: (symbols, config, buffers) rows, each symbol
    f(const config*, const buffers*, void* stream) -> int, go1eval_trace_record alone with the row (int32) in front of the stream."""
    if path is None and module["_lib"] is not None:
        return module["_lib"]
    p = path or module["LIB_PATH"]
    if not os.path.exists(p):
        raise missing(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"(hipcc --offload-arch=gfx950). Device-side {what} have no CPU fallback.")
    lib = ctypes.CDLL(p)
    for symbols, config, buffers in entry_points:
        for fn in symbols:
            row = [ctypes.c_int32] if fn == "go1eval_trace_record" else []
            getattr(lib, fn).argtypes = [ctypes.POINTER(config), ctypes.POINTER(buffers)] + row + [ctypes.c_void_p]
            getattr(lib, fn).restype = ctypes.c_int
    getattr(lib, version).restype = ctypes.c_char_p
    if path is None:
        module["_lib"] = lib
    return lib


def load_library(path=None):
    """Load libgo1eval.so (HIP, gfx950).  Fails loudly: the metrics kernels have no CPU fallback."""
    return _load(globals(), path, Go1EvalLibraryMissing, "evaluation metrics", _ENTRY_POINTS, "go1eval_version")


def _groups(groups, count, member="environment"):
    """(group ids as a flat int32 tensor, G = the largest id + 1) of `groups`: one int per member, -1 = not evaluated"""
    g = torch.as_tensor(groups).to(torch.int32).reshape(-1)
    assert g.numel() == count, (g.numel(), count)
    G = int(g.max()) + 1                                       # (on the host, before the step loop)
    assert G >= 1, f"no {member} carries a group id >= 0"
    return g, G


def _env_ids(env_ids, N, word, rows=None):
    """`env_ids` as a flat int64 array on the host, refused unless there are `rows` of them (None: any number but none), all in
    [0, N) and none named twice; `word` names the caller in the message"""
    ids = np.asarray(torch.as_tensor(env_ids).cpu(), dtype=np.int64).reshape(-1)                # (on the host, before the step loop)
    if rows is not None and ids.size != rows:
        raise ValueError(f"{word}: {ids.size} environment ids for {rows} rows")
    if ids.size == 0 or ids.min() < 0 or ids.max() >= N:
        raise ValueError(f"{word}: environment ids have to lie in [0, {N})")
    if np.unique(ids).size != ids.size:
        raise ValueError(f"{word}: an environment is named twice")
    return ids


class _Host:
    """What every family's host object holds: the library, the simulator's buffers, and how a launch is made and checked."""
    measure_heights = False

    def __init__(self, buffers, lib=None):
        self.lib = lib if lib is not None else load_library()
        self.buffers = buffers
        self.device = buffers.device

    def _heights(self, S):
        """base heights are taken above measured_heights if the simulator measures them, else above z = 0"""
        self.measure_heights = bool(S.measure_heights)
        self.cfg.num_height_points = int(self.buffers.measured_heights.shape[0]) if self.measure_heights else 0

    def _bind(self, buf, names):
        """the simulator's tensors `names` into buf; NULL for one it does not have, and for heights that are not measured"""
        for n in names:
            t = getattr(self.buffers, n)
            bound = t is not None and (n != "measured_heights" or self.measure_heights)
            setattr(buf, n, t.data_ptr() if bound else None)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc}")

    def _launch(self, name, cfg, buf, *row):
        self._check(getattr(self.lib, name)(ctypes.byref(cfg), ctypes.byref(buf), *row, self._stream()), name)


_ACC_DTYPES = {"count": torch.int32, "sum": torch.float64, "sumsq": torch.float64, "min": torch.float32, "max": torch.float32,
               "nonfinite": torch.int32}          # (uint32 on the device; torch reads the same bits as int32)


class _Table(_Host):
    """An accumulating family of one simulator instance: it owns the accumulators ([ROWS][N]), its per-environment state, the
    group ids and the result table ([G][TABLE_ROWS][NUM_FIELDS]), and launches PREFIX_clear / _accumulate / _reduce.  A family
    names these, sets what else its config holds, and reads its table."""
    PREFIX = CONFIG = BUFFERS = None
    INPUTS, ROWS, TABLE_ROWS = (), 0, 0
    STATE_ATTR, STATE = "state", {}               # the attribute the state tensors live under; {name: (dtype, dimensions in front of [N])}

    def __init__(self, S, buffers, lib=None):
        super().__init__(buffers, lib)
        N = self.num_envs = int(S.num_envs)
        self.cfg = self.CONFIG()
        self.cfg.num_envs = N
        self.acc = {n: torch.zeros(self.ROWS, N, dtype=dt, device=self.device) for n, dt in _ACC_DTYPES.items()}
        setattr(self, self.STATE_ATTR, {n: torch.zeros(*lead, N, dtype=dt, device=self.device) for n, (dt, lead) in self.STATE.items()})
        self.group = torch.full((N,), -1, dtype=torch.int32, device=self.device)
        self.table = None
        self.armed = False
        self.buf = self.BUFFERS()

    def _refresh(self):
        b = self.buf
        self._bind(b, self.INPUTS)
        for n, t in list(self.acc.items()) + list(getattr(self, self.STATE_ATTR).items()):
            setattr(b, n, t.data_ptr())
        b.group = self.group.data_ptr()
        b.results = self.table.data_ptr() if self.table is not None else None

    def _call(self, name):
        self._launch(name, self.cfg, self.buf)

    def _size_tables(self, G):
        self.table = torch.zeros(G, self.TABLE_ROWS, NUM_FIELDS, dtype=torch.float64, device=self.device)

    def clear(self):
        """empty accumulators and the family's state as at the start of a measurement (one launch, no sync)"""
        self._call(self.PREFIX + "_clear")

    def arm(self, groups, warmup_steps=0):
        """start a measurement: `groups` = int group id per environment (-1: not evaluated); sizes the table and clears"""
        g, G = _groups(groups, self.num_envs)
        self.group.copy_(g)
        self.cfg.num_groups, self.cfg.warmup_steps = G, int(warmup_steps)
        self._size_tables(G)
        self._refresh()
        self.clear()
        self.armed = True

    def accumulate(self):
        """after a step: fold it into the accumulators and advance the family's state (one launch, no sync)"""
        self._call(self.PREFIX + "_accumulate")

    def disarm(self):
        """stop folding steps (the accumulators keep what they hold for the next read)"""
        self.armed = False

    def reduce(self):
        """the result table [G][TABLE_ROWS][NUM_FIELDS] as a device tensor (one launch, no sync)"""
        assert self.table is not None, "arm() first"
        self._call(self.PREFIX + "_reduce")
        return self.table


class Go1Eval(_Table):
    """Metrics of one simulator instance.  S: its Go1SimConfig, buffers: its SimBuffers (device tensors)."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1eval", Go1EvalConfig, Go1EvalBuffers, _INPUTS
    ROWS, TABLE_ROWS = NUM_METRICS, NUM_METRICS + 1
    STATE_ATTR, STATE = "per_env", {n: (torch.int32, ()) for n in _PER_ENV}

    def __init__(self, S, buffers, lib=None):
        super().__init__(S, buffers, lib)
        self.cfg.default_body_mass = DEFAULT_BODY_MASS
        self._heights(S)
        self._refresh()

    def results(self):
        """{metric name: (G, 6) array with the columns FIELD_NAMES, "groups": (G, 5) array with the columns GROUP_FIELD_NAMES}:
        one launch and one device-to-host copy"""
        return table_to_dict(self.reduce().cpu().numpy())


def table_to_dict(table):
    out = {name: table[:, m, :].copy() for m, name in enumerate(METRIC_NAMES)}
    out["groups"] = table[:, NUM_METRICS, :len(GROUP_FIELD_NAMES)].copy()
    return out


class Go1Behaviour(_Table):
    """The behaviour table of one simulator instance, beside `Go1Eval`: it owns its accumulators and the per-foot stride state,
    which arm() forgets.  S: the simulator's Go1SimConfig, buffers: its SimBuffers (device tensors), dt: the policy step in seconds."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1eval_behaviour", Go1BehaviourConfig, Go1BehaviourBuffers, _BEHAVIOUR_INPUTS
    ROWS, TABLE_ROWS = NUM_BEHAVIOUR, NUM_BEHAVIOUR
    STATE_ATTR = "stride"
    STATE = {"prev_contact": (torch.uint8, (4,)), "stride_steps": (torch.int32, (4,)), "stance_steps": (torch.int32, (4,)),
             "swing_peak": (torch.float32, (4,))}

    def __init__(self, S, buffers, dt, lib=None):
        super().__init__(S, buffers, lib)
        c = self.cfg
        c.num_commands, c.dt, c.base_height_target = int(S.num_commands), float(dt), float(S.base_height_target)
        self._heights(S)
        self._refresh()

    def results(self):
        """{behaviour metric name: (G, 6) array with the columns FIELD_NAMES}: one launch and one device-to-host copy"""
        table = self.reduce().cpu().numpy()
        return {name: table[:, m, :].copy() for m, name in enumerate(BEHAVIOUR_NAMES)}


def response_signals(cfg, signals):
    """fill cfg.signal / cfg.num_signals from {name: (y_channel, r_channel or None[, fixed_target, fixed_scale])}; returns the names"""
    names = list(signals)
    if not 1 <= len(names) <= MAX_SIGNALS:
        raise ValueError(f"response: between 1 and {MAX_SIGNALS} signals, not {len(names)}")
    for s, name in enumerate(names):
        y, r, target, scale = (tuple(signals[name]) + (0.0, 0.0))[:4]
        g = cfg.signal[s]
        g.y_channel, g.r_channel, g.fixed_target, g.fixed_scale = int(y), -1 if r is None else int(r), float(target), float(scale)
    cfg.num_signals = len(names)
    return names


class Go1Trace(_Host):
    """The trace of one simulator instance: a ring of `capacity` rows x 24 channels x K traced environments on the device, one
    launch per recorded step, and the step-response analysis of what it holds.  S: the simulator's Go1SimConfig, buffers: its
    SimBuffers (device tensors).  Nothing is allocated before the first arm()."""

    def __init__(self, S, buffers, lib=None):
        super().__init__(buffers, lib)
        c = self.cfg = Go1TraceConfig()
        c.num_envs, c.base_height_target = int(S.num_envs), float(S.base_height_target)
        self._heights(S)
        self.buf = Go1TraceBuffers()
        self.trace = self.ids = self.env_ids = None
        self.rows, self.truncated, self.armed = 0, False, False

    def arm(self, env_ids=None, capacity=1):
        """start a trace of the environments `env_ids` (None: all of them, in order) with room for `capacity` steps"""
        N = self.cfg.num_envs
        if env_ids is None:
            self.env_ids, self.ids = np.arange(N, dtype=np.int32), None
        else:
            self.env_ids = _env_ids(env_ids, N, "trace").astype(np.int32)
            self.ids = torch.from_numpy(self.env_ids).to(self.device)
        K, capacity = int(self.env_ids.size), int(capacity)
        if capacity < 1:
            raise ValueError("trace: capacity has to be at least 1")
        if self.trace is None or tuple(self.trace.shape) != (capacity, NUM_TRACE, K):
            self.trace = torch.zeros(capacity, NUM_TRACE, K, dtype=torch.float32, device=self.device)
        self.cfg.num_traced, self.cfg.capacity = K, capacity
        b = self.buf
        self._bind(b, _TRACE_INPUTS)
        b.env_ids = self.ids.data_ptr() if self.ids is not None else None
        b.trace = self.trace.data_ptr()
        self.rows, self.truncated, self.armed = 0, False, True

    def record(self):
        """after a step: the next row (one launch, no sync).  A full ring records nothing more and sets `truncated`."""
        if self.rows >= self.cfg.capacity:
            self.truncated = True
            return
        self._launch("go1eval_trace_record", self.cfg, self.buf, self.rows)
        self.rows += 1

    def disarm(self):
        """stop recording (the trace keeps what it holds for `read()` and `response()`)"""
        self.armed = False

    def read(self):
        """{channel name: (rows, K) float32 array} plus "env_ids" (K,), "rows" and "truncated": one device-to-host copy"""
        assert self.trace is not None, "arm() first"
        t = self.trace[:self.rows].cpu().numpy()
        out = {name: t[:, c, :].copy() for c, name in enumerate(TRACE_CHANNELS)}
        out.update(env_ids=self.env_ids.copy(), rows=self.rows, truncated=self.truncated)
        return out

    def _analysis(self, c, buffers, symbols, V, groups):
        """The back half of an analysis of the recorded rows: c = its config, filled but for num_traced, rows and num_groups,
        buffers = its buffers type, symbols = (per-environment kernel's entry point, reduction's), V = values per traced
        environment.  The table, the values and the status share one allocation (fp64 first: aligned), so two launches and one
        device-to-host copy.  Returns (table (G, V + 1, 6) float64, values (V, K) float32, status (K,) int32) on the host."""
        K = int(self.cfg.num_traced)
        g, G = _groups(groups, K, "traced environment")
        c.num_traced, c.rows, c.num_groups = K, self.rows, G
        nbytes = [G * (V + 1) * NUM_FIELDS * 8, V * K * 4, K * 4]                     # results, values, status
        out = torch.zeros(sum(nbytes), dtype=torch.uint8, device=self.device)
        group = g.to(self.device)
        b = buffers()
        b.trace, b.group = self.trace.data_ptr(), group.data_ptr()
        b.results, b.values, b.status = out.data_ptr(), out.data_ptr() + nbytes[0], out.data_ptr() + nbytes[0] + nbytes[1]
        for name in symbols:
            self._launch(name, c, b)
        host = out.cpu().numpy()
        return (host[:nbytes[0]].view(np.float64).reshape(G, V + 1, NUM_FIELDS), host[nbytes[0]:nbytes[0] + nbytes[1]].view(np.float32).reshape(V, K),
                host[nbytes[0] + nbytes[1]:].view(np.int32).copy())

    def response(self, signals, switch_row, pre, smooth, band, hold, tail, dt, groups):
        """The step response of the recorded rows.  signals: {name: (y_channel, r_channel or None[, fixed_target, fixed_scale])};
        groups: one int per traced environment (-1: not evaluated).  Returns {signal: {metric: (G, 6) array with the columns
        FIELD_NAMES}}, "groups": (G, 4) array with the columns RESPONSE_GROUP_FIELDS, "values": {signal: {metric: (K,) float32}}
        and "status": (K,) int32.  Two launches and one device-to-host copy."""
        assert self.trace is not None, "arm() first"
        c = Go1ResponseConfig()
        names = response_signals(c, signals)
        c.switch_row, c.pre, c.smooth, c.hold, c.tail, c.band, c.dt = int(switch_row), int(pre), int(smooth), int(hold), int(tail), float(band), float(dt)
        table, values, status = self._analysis(c, Go1ResponseBuffers, ("go1eval_response", "go1eval_response_reduce"), len(names) * NUM_RESPONSE, groups)
        rows, values = table[:, :-1, :].reshape(-1, len(names), NUM_RESPONSE, NUM_FIELDS), values.reshape(len(names), NUM_RESPONSE, -1)
        res = {name: {m: rows[:, s, i, :].copy() for i, m in enumerate(RESPONSE_METRICS)} for s, name in enumerate(names)}
        res["groups"] = table[:, -1, :len(RESPONSE_GROUP_FIELDS)].copy()
        res["values"] = {name: {m: values[s, i].copy() for i, m in enumerate(RESPONSE_METRICS)} for s, name in enumerate(names)}
        res["status"] = status
        return res

    def recovery(self, push_row, pre, smooth, band, hold, dt, groups):
        """The recovery from a push of the recorded rows: push_row = the first row recorded after the push, `pre` baseline rows
        before it, a box filter of `smooth` rows, `band` in m/s above the baseline, `hold` rows at the end inside the band.
        groups: one int per traced environment (-1: not evaluated).  Returns {metric: (G, 6) array with the columns FIELD_NAMES},
        "groups": (G, 5) array with the columns RECOVERY_GROUP_FIELDS, "values": {metric: (K,) float32} and "status": (K,) int32
        (RECOVERY_STATUS).  Two launches and one device-to-host copy."""
        assert self.trace is not None, "arm() first"
        c = Go1RecoveryConfig()
        c.push_row, c.pre, c.smooth, c.hold, c.band, c.dt = int(push_row), int(pre), int(smooth), int(hold), float(band), float(dt)
        table, values, status = self._analysis(c, Go1RecoveryBuffers, ("go1eval_recovery", "go1eval_recovery_reduce"), NUM_RECOVERY, groups)
        res = {m: table[:, i, :].copy() for i, m in enumerate(RECOVERY_METRICS)}
        res["groups"] = table[:, -1, :len(RECOVERY_GROUP_FIELDS)].copy()
        res["values"] = {m: values[i].copy() for i, m in enumerate(RECOVERY_METRICS)}
        res["status"] = status
        return res


class Go1Push(_Host):
    """Pushes of one simulator instance: a table of velocity steps (forward, left, up, yaw rate; PUSH_ROWS) for chosen environments,
    checked on the host, held on the device, and added to the base velocities in root_states by one launch per `launch()`.
    S: the simulator's Go1SimConfig, buffers: its SimBuffers (device tensors).  Nothing is allocated before the first load()."""

    def __init__(self, S, buffers, lib=None):
        super().__init__(buffers, lib)
        self.cfg = Go1PushConfig()
        self.cfg.num_envs = int(S.num_envs)
        self.buf = Go1PushBuffers()
        self.table = self.ids = self.env_ids = None

    def load(self, push, env_ids=None):
        """the table of the next launches: push (K, 4), one row of PUSH_ROWS per pushed environment; env_ids (K,) or None (every
        environment, in order).  Refused before anything is copied: a table that is not (K, 4) or not finite, an id outside
        [0, N), an id named twice.  A tensor on the device is read to the host for the check."""
        N = self.cfg.num_envs
        p = np.asarray(torch.as_tensor(push).detach().cpu(), dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != NUM_PUSH or p.shape[0] == 0:
            raise ValueError(f"push: the table has to be (K, {NUM_PUSH}) with K >= 1, not {p.shape}")
        if not np.isfinite(p).all():
            raise ValueError("push: the table holds a value that is not finite")
        K = int(p.shape[0])
        if env_ids is None:
            if K != N:
                raise ValueError(f"push: a table without environment ids needs one row per environment ({N}), not {K}")
            ids = None
        else:
            ids = _env_ids(env_ids, N, "push", rows=K)
        self.env_ids = np.arange(N, dtype=np.int32) if ids is None else ids.astype(np.int32)
        self.ids = None if ids is None else torch.from_numpy(self.env_ids).to(self.device)
        self.table = torch.from_numpy(np.ascontiguousarray(p.T)).to(self.device)              # [4][K]
        self.cfg.num_pushed = K
        b = self.buf
        b.root_states = self.buffers.root_states.data_ptr()
        b.env_ids = self.ids.data_ptr() if self.ids is not None else None
        b.push = self.table.data_ptr()

    def launch(self):
        """add the loaded table to the base velocities now (one launch, no sync): between two simulator steps"""
        assert self.table is not None, "load() first"
        self._launch("go1eval_push", self.cfg, self.buf)


class Go1Terrain(_Table):
    """Terrain traversal of one simulator instance, beside the tables: it owns its accumulators and the per-environment status,
    step count and distance, and binds the simulator's height field and env_origins.  S: the simulator's Go1SimConfig, buffers:
    its SimBuffers (device tensors), dt: the policy step in seconds, tile_length / tile_width: a tile's extent along x / y in
    metres.  A simulator without a height field (the plane) gives height_samples = NULL: the ground is 0.  clear() leaves every
    environment RUNNING at step 0."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1eval_terrain", Go1TerrainConfig, Go1TerrainBuffers, _TERRAIN_INPUTS
    ROWS, TABLE_ROWS = NUM_TERRAIN, NUM_TERRAIN + NUM_OUTCOME + 1
    STATE = {"status": (torch.uint8, ()), "steps": (torch.int32, ()), "end_step": (torch.int32, ()), "max_dist": (torch.float32, ())}

    def __init__(self, S, buffers, dt, tile_length, tile_width, lib=None):
        super().__init__(S, buffers, lib)
        c = self.cfg
        c.dt, c.tile_length, c.tile_width = float(dt), float(tile_length), float(tile_width)
        c.penalised_body_mask = int(S.penalised_body_mask)
        self.field = buffers.height_samples
        if self.field is not None:
            c.hf_rows, c.hf_cols = int(self.field.shape[0]), int(self.field.shape[1])
            c.hf_hscale, c.hf_vscale, c.hf_border = float(S.hf_hscale), float(S.hf_vscale), float(S.hf_border)
        else:
            c.hf_rows, c.hf_cols, c.hf_hscale, c.hf_vscale, c.hf_border = 0, 0, 1.0, 0.0, 0.0          # not read: every sample is 0
        self._refresh()

    def read(self):
        """{"metrics": {name: (G, 6) array with the columns FIELD_NAMES}, "outcomes": {name: (G, 6) array}, "groups": (G, 6) array with
        the columns TERRAIN_GROUP_FIELDS, "status", "steps", "end_step": (N,) integer arrays, "max_dist": (N,) float32}: one launch
        and the device-to-host copies of the table and the four state arrays"""
        table = self.reduce().cpu().numpy()
        out = dict(metrics={name: table[:, m, :].copy() for m, name in enumerate(TERRAIN_NAMES)},
                   outcomes={name: table[:, NUM_TERRAIN + o, :].copy() for o, name in enumerate(TERRAIN_OUTCOMES)},
                   groups=table[:, NUM_TERRAIN + NUM_OUTCOME, :].copy())
        out.update({n: t.cpu().numpy() for n, t in self.state.items()})
        return out


def joint_edges(limit):
    """the nine edges of the eight histogram bins on the scale `limit`: bin k covers [edges[k], edges[k + 1]); values beyond the two
    ends are counted in the first and the last bin"""
    return float(limit) * (np.arange(JOINT_TAU_BINS + 1) / 4.0 - 1.0)


class Go1Joints(_Table):
    """Per-joint actuator usage of one simulator instance, beside the tables: it owns its accumulators ([12 * 10][N]), its copy of the
    previous joint velocities and the per-environment torque-speed histogram ([12][64][N]).  S: the simulator's Go1SimConfig,
    buffers: its SimBuffers (device tensors), dt: the policy step in seconds, vel_limit: the twelve URDF speed limits in rad/s,
    soft_torque_limit / soft_vel_limit: the factors of the two saturation tests.  The torque limits and the soft position limits are
    the simulator's own (S.torque_limits, S.dof_pos_soft_lower / upper).  clear() also empties the histogram and takes the
    simulator's current joint velocities as the previous ones."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1eval_joint", Go1JointConfig, Go1JointBuffers, _JOINT_INPUTS
    ROWS, TABLE_ROWS = NUM_DOF * NUM_JOINT, NUM_DOF * NUM_JOINT + 1
    STATE = {"prev_dof_vel": (torch.float32, (NUM_DOF,)), "steps": (torch.int32, ()), "resets": (torch.int32, ()),
             "hist": (torch.int32, (NUM_DOF, JOINT_TAU_BINS * JOINT_VEL_BINS))}

    def __init__(self, S, buffers, dt, vel_limit, soft_torque_limit=1.0, soft_vel_limit=1.0, lib=None):
        super().__init__(S, buffers, lib)
        c = self.cfg
        c.dt, c.soft_torque_limit, c.soft_vel_limit = float(dt), float(soft_torque_limit), float(soft_vel_limit)
        for j in range(NUM_DOF):
            c.torque_limit[j], c.vel_limit[j] = float(S.torque_limits[j]), float(vel_limit[j])
            c.pos_lower[j], c.pos_upper[j] = float(S.dof_pos_soft_lower[j]), float(S.dof_pos_soft_upper[j])
        self.hist_table = None
        self._refresh()

    def _refresh(self):
        super()._refresh()
        self.buf.hist_results = self.hist_table.data_ptr() if self.hist_table is not None else None

    def _size_tables(self, G):
        super()._size_tables(G)
        self.hist_table = torch.zeros(G, NUM_DOF, JOINT_TAU_BINS, JOINT_VEL_BINS, dtype=torch.int64, device=self.device)   # (uint64 on the device)

    def reduce(self):
        """(the result table [G][12 * 10 + 1][NUM_FIELDS], the histogram table [G][12][8][8]) as device tensors (one launch, no sync)"""
        return super().reduce(), self.hist_table

    def read(self):
        """{"metrics": {name: (G, 12, 6) array with the columns FIELD_NAMES, one row per joint of DOF_NAMES}, "groups": (G, 3) array with
        the columns JOINT_GROUP_FIELDS, "hist": (G, 12, 8, 8) int64 array [group][joint][torque bin][speed bin], "tau_edges", "vel_edges":
        (12, 9) bin edges, "steps", "resets": (N,) integer arrays, "prev_dof_vel": (12, N) float32, "env_hist": (12, 64, N)}: one launch
        and the device-to-host copies of the two tables and the state arrays"""
        table, hist = self.reduce()
        table = table.cpu().numpy()
        rows = table[:, :NUM_DOF * NUM_JOINT, :].reshape(-1, NUM_DOF, NUM_JOINT, NUM_FIELDS)
        out = dict(metrics={name: rows[:, :, m, :].copy() for m, name in enumerate(JOINT_NAMES)},
                   groups=table[:, NUM_DOF * NUM_JOINT, :len(JOINT_GROUP_FIELDS)].copy(), hist=hist.cpu().numpy(),
                   tau_edges=np.stack([joint_edges(self.cfg.torque_limit[j]) for j in range(NUM_DOF)]),
                   vel_edges=np.stack([joint_edges(self.cfg.vel_limit[j]) for j in range(NUM_DOF)]))
        out.update({("env_hist" if n == "hist" else n): t.cpu().numpy() for n, t in self.state.items()})
        return out
