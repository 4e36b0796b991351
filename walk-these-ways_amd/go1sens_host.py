"""Host side of the sensitivity C-ABI (include/go1sens.h): ctypes mirrors, library loading, and `Go1Sensitivity`, which owns the
`value` accumulators, the parameter values in force, the per-bin counters and sums, the pair map and the four result tables of one
simulator instance.

libgo1sens.so is a library of its own (the other table libraries' surfaces stay as they are) whose device code shares
csrc/go1_tables.h with them, and the host side shares as much: `load_library` is `go1eval_host._load` with this module's path, cache,
error class and entry points, and `Go1Sensitivity` subclasses `go1eval_host._Table` and hands it its own library, so arm / accumulate /
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
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1sens.so")

PARAMETERS = ["friction", "restitution", "payload", "com_x", "com_y", "com_z", "motor_strength", "Kp_factor", "Kd_factor"]       # enum Go1SensParam
QUANTITIES = ["steps", "measured", "falls", "timeouts", "reward_sum", "lin_err_sum", "yaw_err_sum", "power_sum"]                # enum Go1SensQuantity
COUNTS = ["unbinned", "redraws", "bad"]                                                                                      # enum Go1SensCount
PAIR_QUANTITIES = ["steps", "falls", "measured", "lin_err_sum"]                                                              # enum Go1SensPairQuantity
SENS_GROUP_FIELDS = ["envs", "launches"]                                                                                     # enum Go1SensGroupField
NUM_PARAMETERS, BINS, NUM_QUANT, NUM_COUNTS, PAIR_SIDE, PAIR_CELLS, PAIR_QUANT = 9, 16, 8, 3, 8, 64, 4
# parameter -> (the configuration's switch, its range) in cfg.domain_rand: what the simulator draws the parameter from
DOMAIN_RAND = dict(friction=("randomize_friction", "friction_range"), restitution=("randomize_restitution", "restitution_range"),
                   payload=("randomize_base_mass", "added_mass_range"), com_x=("randomize_com_displacement", "com_displacement_range"),
                   com_y=("randomize_com_displacement", "com_displacement_range"), com_z=("randomize_com_displacement", "com_displacement_range"),
                   motor_strength=("randomize_motor_strength", "motor_strength_range"), Kp_factor=("randomize_Kp_factor", "Kp_factor_range"),
                   Kd_factor=("randomize_Kd_factor", "Kd_factor_range"))


class Go1SensConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("warmup_steps", ctypes.c_int32), ("num_groups", ctypes.c_int32), ("pair_a", ctypes.c_int32),
                ("pair_b", ctypes.c_int32), ("active", ctypes.c_int32 * NUM_PARAMETERS), ("lo", ctypes.c_float * NUM_PARAMETERS),
                ("scale", ctypes.c_float * NUM_PARAMETERS)]


_SENS_STEP_INPUTS = ["reset_buf", "time_out_buf", "episode_length_buf", "rew_buf", "base_lin_vel", "base_ang_vel", "commands", "torques", "dof_vel"]
_SENS_PARAMETER_INPUTS = ["friction_coeffs", "restitutions", "payloads", "com_displacements", "motor_strengths", "Kp_factors", "Kd_factors"]
_SENS_INPUTS = _SENS_STEP_INPUTS + _SENS_PARAMETER_INPUTS
_SENS_STATE = ["cur", "pair_cur", "steps", "measured", "falls", "timeouts", "reward_sum", "lin_err_sum", "yaw_err_sum", "power_sum", "unbinned", "redraws",
               "bad", "launches", "pair_steps", "pair_falls", "pair_measured", "pair_lin_err_sum"]
_SENS_TABLES = ["results", "curves", "counts", "pair_results"]


class Go1SensBuffers(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in _SENS_INPUTS + _ACCUMULATORS + _SENS_STATE + ["group"] + _SENS_TABLES]


EXPORTED_SYMBOLS = ["go1sens_clear", "go1sens_snapshot", "go1sens_accumulate", "go1sens_reduce", "go1sens_version"]

_lib = None


class Go1SensLibraryMissing(RuntimeError):
    pass


def load_library(path=None):
    """Load libgo1sens.so (HIP, gfx950).  Fails loudly: the sensitivity kernels have no CPU fallback."""
    return _load(globals(), path, Go1SensLibraryMissing, "sensitivity metrics", [(EXPORTED_SYMBOLS[:4], Go1SensConfig, Go1SensBuffers)],
                 "go1sens_version")


def configured_range(domain_rand, name):
    """(lo, hi): the range the configuration section `domain_rand` holds for the parameter `name`, sorted"""
    lo, hi = sorted(float(x) for x in getattr(domain_rand, DOMAIN_RAND[name][1]))
    return lo, hi


def default_ranges(domain_rand):
    """{parameter: (lo, hi)} of the parameters whose randomize_* switch is on in the configuration section `domain_rand`: the range the
    simulator draws from, sorted (the reference's static_low carries a motor strength range of [0.9, -0.99]).  A range of no width says
    nothing about where the bins should lie: its parameter is left out, as one whose switch is off."""
    out = {}
    for name in PARAMETERS:
        if getattr(domain_rand, DOMAIN_RAND[name][0], False):
            lo, hi = configured_range(domain_rand, name)
            if math.isfinite(lo) and math.isfinite(hi) and hi > lo:
                out[name] = (lo, hi)
    return out


def checked_ranges(ranges):
    """{parameter: (lo, hi)} as floats in the order of PARAMETERS; ValueError for a name that is no parameter, a bound that is not finite
    or a range with hi <= lo"""
    unknown = [name for name in ranges if name not in PARAMETERS]
    if unknown:
        raise ValueError(f"sensitivity: {unknown[0]!r} is no parameter: one of {PARAMETERS}")
    out = {}
    for name in PARAMETERS:
        if name in ranges:
            lo, hi = (float(x) for x in ranges[name])
            if not (math.isfinite(lo) and math.isfinite(hi)):
                raise ValueError(f"sensitivity: the range of {name} has to be finite, not ({lo}, {hi})")
            if hi <= lo:
                raise ValueError(f"sensitivity: the range of {name} needs hi > lo, not ({lo}, {hi})")
            out[name] = (lo, hi)
    return out


def bin_edges(ranges):
    """(9, 17): the edges of every active parameter's sixteen bins, NaN for an inactive one.  Bin k holds edges[k] <= v < edges[k + 1];
    the end bins also hold what lies outside the range"""
    edges = np.full((NUM_PARAMETERS, BINS + 1), np.nan)
    for name, (lo, hi) in ranges.items():
        edges[PARAMETERS.index(name)] = np.linspace(lo, hi, BINS + 1)
    return edges


class Go1Sensitivity(_Table):
    """The sensitivity tables of one simulator instance: it owns the nine `value` rows ([9][N]), the values in force, the counters and
    sums per (parameter, bin) ([9][16][N]) and the pair map ([64][N]).  S: the simulator's Go1SimConfig, buffers: its SimBuffers (device
    tensors).  arm() takes the values in force from the simulator's buffers; snapshot() takes them again without clearing."""
    PREFIX, CONFIG, BUFFERS, INPUTS = "go1sens", Go1SensConfig, Go1SensBuffers, _SENS_INPUTS
    ROWS, TABLE_ROWS = NUM_PARAMETERS, NUM_PARAMETERS + 1
    _I, _D = torch.int32, torch.float64                                      # (uint32 on the device; torch reads the same bits as int32)
    STATE = {"cur": (torch.float32, (NUM_PARAMETERS,)), "pair_cur": (torch.float32, (2,)),
             "steps": (_I, (NUM_PARAMETERS, BINS)), "measured": (_I, (NUM_PARAMETERS, BINS)), "falls": (_I, (NUM_PARAMETERS, BINS)),
             "timeouts": (_I, (NUM_PARAMETERS, BINS)), "reward_sum": (_D, (NUM_PARAMETERS, BINS)), "lin_err_sum": (_D, (NUM_PARAMETERS, BINS)),
             "yaw_err_sum": (_D, (NUM_PARAMETERS, BINS)), "power_sum": (_D, (NUM_PARAMETERS, BINS)), "unbinned": (_I, (NUM_PARAMETERS,)),
             "redraws": (_I, (NUM_PARAMETERS,)), "bad": (_I, (NUM_PARAMETERS,)), "launches": (_I, ()), "pair_steps": (_I, (PAIR_CELLS,)),
             "pair_falls": (_I, (PAIR_CELLS,)), "pair_measured": (_I, (PAIR_CELLS,)), "pair_lin_err_sum": (_D, (PAIR_CELLS,))}

    def __init__(self, S, buffers, lib=None):
        super().__init__(S, buffers, lib if lib is not None else load_library())
        self.cfg.pair_a = self.cfg.pair_b = -1
        self.ranges, self.pair = {}, None
        self.curves_table = self.counts_table = self.pair_table = None
        self._refresh()

    def _refresh(self):
        super()._refresh()
        for field, table in (("curves", self.curves_table), ("counts", self.counts_table), ("pair_results", self.pair_table)):
            setattr(self.buf, field, table.data_ptr() if table is not None else None)

    def _size_tables(self, G):
        super()._size_tables(G)
        self.curves_table = torch.zeros(G, NUM_PARAMETERS, NUM_QUANT, BINS, dtype=torch.float64, device=self.device)
        self.counts_table = torch.zeros(G, NUM_PARAMETERS, NUM_COUNTS, dtype=torch.float64, device=self.device)
        self.pair_table = torch.zeros(G, PAIR_QUANT, PAIR_CELLS, dtype=torch.float64, device=self.device)

    def ranges_of(self, domain_rand, ranges=None):
        """the configuration's default_ranges() with the entries of `ranges` replacing or adding to them; an entry of None stands for the
        configuration's own range of that parameter, whether its switch is on or not"""
        ranges = dict(ranges or {})
        for name, span in ranges.items():
            if span is None and name in DOMAIN_RAND:
                ranges[name] = configured_range(domain_rand, name)
        out = default_ranges(domain_rand)
        out.update(checked_ranges(ranges))
        return {name: out[name] for name in PARAMETERS if name in out}

    def arm(self, groups, warmup_steps=0, ranges=None, pair=None):
        """as _Table.arm().  ranges: {parameter name: (lo, hi)}: the parameters measured and the span of their sixteen bins, every other
        parameter is inactive; pair: two names of them for the 8 x 8 map, or None.  The clear takes the values in force from the
        simulator's buffers"""
        ranges = checked_ranges(ranges or {})
        if pair is not None:
            pair = tuple(pair)
            if len(pair) != 2 or pair[0] == pair[1] or any(name not in ranges for name in pair):
                raise ValueError(f"sensitivity: a pair is two different active parameters of {list(ranges)}, not {pair}")
        c = self.cfg
        for p, name in enumerate(PARAMETERS):
            lo, hi = ranges.get(name, (0.0, 0.0))
            c.active[p], c.lo[p], c.scale[p] = int(name in ranges), lo, (BINS / (hi - lo) if name in ranges else 0.0)      # (fp64, rounded once)
        c.pair_a, c.pair_b = (PARAMETERS.index(pair[0]), PARAMETERS.index(pair[1])) if pair else (-1, -1)
        self.ranges, self.pair = ranges, pair
        super().arm(groups, warmup_steps)

    def snapshot(self):
        """take the values in force from the simulator's buffers again, clearing nothing (one launch, no sync): after a reset from
        outside the step, which re-draws the motor parameters"""
        self._call(self.PREFIX + "_snapshot")

    def reduce(self):
        """(the result table [G][10][6], the curves [G][9][8][16], the counts [G][9][3], the pair map [G][4][64]) as device tensors (one
        launch, no sync)"""
        return super().reduce(), self.curves_table, self.counts_table, self.pair_table

    def read(self):
        """{"parameters": the nine names, "active": (9,) bool, "edges": (9, 17) bin edges (NaN for an inactive parameter), "ranges",
        "value": {name: (G, 6) array with the columns go1eval_host.FIELD_NAMES}, "curves": {quantity: (G, 9, 16)} for QUANTITIES,
        "counts": (G, 9, 3) unbinned, redraws, bad, "groups": (G, 2) environments and launches, "pair": the two names or None,
        "pair_map": {quantity: (G, 8, 8)} for PAIR_QUANTITIES stacked as (G, 4, 8, 8) or None, and the per-environment state under
        "env_" + its name}: one launch and the device-to-host copies"""
        table, curves, counts, pair = (t.cpu().numpy() for t in self.reduce())
        out = dict(parameters=list(PARAMETERS), active=np.array([name in self.ranges for name in PARAMETERS]), edges=bin_edges(self.ranges),
                   ranges=dict(self.ranges), value={name: table[:, p, :].copy() for p, name in enumerate(PARAMETERS)},
                   curves={q: curves[:, :, k, :].copy() for k, q in enumerate(QUANTITIES)}, counts=counts.copy(),
                   groups=table[:, self.ROWS, :len(SENS_GROUP_FIELDS)].copy(), pair=self.pair,
                   pair_map=pair.reshape(-1, PAIR_QUANT, PAIR_SIDE, PAIR_SIDE).copy() if self.pair else None)
        out.update({"env_" + n: t.cpu().numpy() for n, t in self.state.items()})
        return out
