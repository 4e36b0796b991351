"""Host side of the state C-ABI (include/go1state.h): the classification of the simulator's buffers, ctypes mirrors, library loading,
`SimState` (a packed snapshot) and `Go1State`, which captures and restores the state of one simulator instance.

libgo1state.so is a library of its own: nothing imports this module until an environment saves or loads a state
(LeggedRobot.save_state / load_state), and libgo1sim.so's surface stays as it is.  A capture is one launch that gathers the chosen
environments into the packed sections; a restore is one launch that scatters snapshot rows into chosen environments, re-phased to the
simulator's current ring positions.  Neither reads simulator data on the host.
"""
import ctypes
import os

import numpy as np
import torch

import go1sim_abi as abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1state.so")

# ---- the classification: every tensor of a SimBuffers is in exactly one of the three --------------------------------------------------------
# PER_ENV: name -> the packed section and the kind of copy.  "words": SoA rows of 4-byte words; "lag": the lag ring, stored in logical order;
# "bytes": SoA rows of bytes; "rows": row-major (N, cols); "history": the observation-history ring, stored in logical order.  The outputs of
# the last step (obs_buf, rew_buf, reset_buf, measured_heights, ...) are here too: after a load the caller reads what it read at the save.
PER_ENV = {
    "root_states": "words", "dof_pos": "words", "dof_vel": "words", "contact_forces": "words", "foot_positions": "words",
    "foot_velocities": "words", "prev_foot_velocities": "words", "lag_buffer": "lag",
    "joint_pos_err_last": "words", "joint_pos_err_last_last": "words", "joint_vel_last": "words", "joint_vel_last_last": "words",
    "joint_pos_target": "words", "last_joint_pos_target": "words", "last_last_joint_pos_target": "words",
    "actions": "words", "last_actions": "words", "last_last_actions": "words", "last_dof_vel": "words", "torques": "words",
    "base_lin_vel": "words", "base_ang_vel": "words", "projected_gravity": "words",
    "commands": "words", "gait_indices": "words", "clock_inputs": "words", "desired_contact_states": "words", "foot_indices": "words",
    "episode_length_buf": "words", "reset_buf": "bytes", "time_out_buf": "bytes", "last_contacts": "bytes", "resample_flags": "bytes",
    "rew_buf": "words", "episode_sums": "words", "command_sums": "words", "episode_sums_eval": "words",
    "friction_coeffs": "words", "restitutions": "words", "payloads": "words", "com_displacements": "words",
    "motor_strengths": "words", "motor_offsets": "words", "Kp_factors": "words", "Kd_factors": "words", "env_origins": "words",
    "env_command_bins": "words", "env_command_categories": "words",
    "obs_buf": "rows", "privileged_obs_buf": "rows", "obs_history": "history",
    "fault_flags": "words", "measured_heights": "words",
}
# GLOBAL: not per environment; copied by whole-state saves only, in this order
GLOBAL = ["curriculum_weights", "curriculum_cdf", "curriculum_success", "episode_log", "fault_counts", "contact_drop_counts"]
# STATIC: never part of a snapshot
STATIC = {
    "curriculum_nbr_ptr": "the CSR of the curriculum grid's neighbourhoods: a function of the configuration, written once at construction",
    "curriculum_nbr_idx": "as curriculum_nbr_ptr",
    "height_samples": "the terrain: not part of a snapshot, bound once by bind_height_field()",
    "contact_signature": "a test record of the last step's substeps, allocated on request only: no step reads it",
}
SECTION_ORDER = {"rows": ["obs_buf", "obs_history", "privileged_obs_buf"]}          # (words and bytes: the order of include/go1sim.h)

HEADER_WORDS = 12
HEADER_NAMES = ["magic", "version", "num_obs", "num_privileged_obs", "num_obs_history", "lag_timesteps", "num_rewards", "num_height_points",
                "command_rows", "num_categories", "num_bins", "curriculum_update_interval"]
RETURN_CODES = {-1: "no config, buffers or environments", -2: "no snapshot storage", -3: "a simulator buffer is missing",
                -8: "a subset without ids", -12: "a refused geometry (another layout, or a ring position out of range)", -20: "the launch failed"}


class Go1StateConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ["num_envs"] + HEADER_NAMES[2:]]


class Go1StateLayout(ctypes.Structure):
    _fields_ = [("header", ctypes.c_int32 * HEADER_WORDS), ("word_rows", ctypes.c_int32), ("byte_rows", ctypes.c_int32),
                ("row_words", ctypes.c_int32), ("global_words", ctypes.c_int32), ("bytes_per_env", ctypes.c_int64)]


class Go1StateSnapshot(ctypes.Structure):
    _fields_ = [("header", ctypes.c_int32 * HEADER_WORDS), ("num_rows", ctypes.c_int32), ("words", ctypes.c_void_p), ("bytes", ctypes.c_void_p),
                ("rows", ctypes.c_void_p), ("global", ctypes.c_void_p), ("skipped", ctypes.c_void_p)]


EXPORTED_SYMBOLS = ["go1state_layout", "go1state_capture", "go1state_restore", "go1state_capture_global", "go1state_restore_global",
                    "go1state_version"]

_lib = None


class Go1StateLibraryMissing(RuntimeError):
    pass


def load_library(path=None):
    """Load libgo1state.so (HIP, gfx950).  Fails loudly: the state kernels have no CPU fallback.  A library loaded from another path is
    not cached."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise Go1StateLibraryMissing(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                     f"(hipcc --offload-arch=gfx950). Device-side state copies have no CPU fallback.")
    lib = ctypes.CDLL(p)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    cfg, buf, snap = ctypes.POINTER(Go1StateConfig), ctypes.POINTER(abi.Go1SimBuffers), ctypes.POINTER(Go1StateSnapshot)
    lib.go1state_layout.argtypes = [cfg, ctypes.POINTER(Go1StateLayout)]
    lib.go1state_capture.argtypes = [cfg, buf, vp, i32, i32, i32, snap, vp]
    lib.go1state_restore.argtypes = [cfg, buf, vp, vp, i32, i32, i32, snap, vp]
    lib.go1state_capture_global.argtypes = [cfg, buf, snap, vp]
    lib.go1state_restore_global.argtypes = [cfg, buf, snap, vp]
    for fn in EXPORTED_SYMBOLS[:-1]:
        getattr(lib, fn).restype = ctypes.c_int
    lib.go1state_version.restype = ctypes.c_char_p
    if path is None:
        _lib = lib
    return lib


def state_config(S):
    """the Go1StateConfig of a simulator configuration (Go1SimConfig)"""
    c = Go1StateConfig()
    c.num_envs, c.num_obs, c.num_privileged_obs, c.num_obs_history = int(S.num_envs), int(S.num_obs), int(S.num_privileged_obs), int(S.num_obs_history)
    c.lag_timesteps, c.num_rewards = int(S.lag_timesteps), int(S.num_rewards)
    c.num_height_points, c.command_rows = int(S.num_height_x) * int(S.num_height_y), int(abi.GO1_MAX_COMMANDS)
    c.num_categories, c.num_bins = int(S.num_categories), int(S.num_bins)
    c.curriculum_update_interval = max(int(S.curriculum_update_interval), 1)
    return c


def _layout_dict(L):
    return dict(header=np.array(list(L.header), dtype=np.int32), word_rows=int(L.word_rows), byte_rows=int(L.byte_rows),
                row_words=int(L.row_words), global_words=int(L.global_words), bytes_per_env=int(L.bytes_per_env))


def layout_of(cfg, lib=None):
    """{"header": (12,) int32, "word_rows", "byte_rows", "row_words", "global_words", "bytes_per_env"} of a Go1StateConfig"""
    L = Go1StateLayout()
    rc = (lib if lib is not None else load_library()).go1state_layout(ctypes.byref(cfg), ctypes.byref(L))
    if rc != 0:
        raise RuntimeError(f"go1state_layout failed: {rc} ({RETURN_CODES.get(rc, '?')})")
    return _layout_dict(L)


class SimState:
    """A packed snapshot of `num_rows` environments (include/go1state.h): device-resident where it was taken.
    layout: layout_of()'s dict; env_ids: the environments it was taken from (int32 tensor) or None for all, in order; counter: the
    simulator's step counter at the save; whole: taken with env_ids=None, so it carries the global section (`glob`) too; words (W, K)
    int32, bytes (B, K) uint8, rows (row_words * K,) int32: the per-environment sections."""
    SECTIONS = ("words", "bytes", "rows", "glob")

    def __init__(self, layout, num_rows, env_ids, counter, whole, words, bytes, rows, glob=None):
        self.layout, self.num_rows, self.env_ids, self.counter, self.whole = layout, int(num_rows), env_ids, int(counter), bool(whole)
        self.words, self.bytes, self.rows, self.glob = words, bytes, rows, glob

    @property
    def device(self):
        return self.words.device

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.words, self.bytes, self.rows, self.glob) if t is not None)

    def to(self, device):
        """a copy on `device` (this object if it is there already)"""
        device = torch.device(device)
        if device == self.device:
            return self
        mv = lambda t: None if t is None else t.to(device)       # noqa: E731
        return SimState(self.layout, self.num_rows, mv(self.env_ids), self.counter, self.whole, mv(self.words), mv(self.bytes), mv(self.rows),
                        mv(self.glob))

    def cpu(self):
        return self.to("cpu")

    def save(self, path):
        """one .npz: the header, the sizes, the sections and the counter"""
        s = self.cpu()
        arrays = dict(header=s.layout["header"], sizes=np.array([s.layout[k] for k in ("word_rows", "byte_rows", "row_words", "global_words",
                                                                                        "bytes_per_env")], dtype=np.int64),
                      num_rows=np.int64(s.num_rows), counter=np.int64(s.counter), whole=np.bool_(s.whole),
                      words=s.words.numpy(), bytes=s.bytes.numpy(), rows=s.rows.numpy())
        if s.env_ids is not None:
            arrays["env_ids"] = s.env_ids.numpy()
        if s.glob is not None:
            arrays["glob"] = s.glob.numpy()
        with open(path, "wb") as fh:
            np.savez(fh, **arrays)

    @classmethod
    def load(cls, path):
        """the snapshot of a file written by save(), on the CPU (`.to(device)` moves it)"""
        with np.load(path, allow_pickle=False) as d:
            sizes = d["sizes"]
            layout = dict(header=d["header"].astype(np.int32), word_rows=int(sizes[0]), byte_rows=int(sizes[1]), row_words=int(sizes[2]),
                          global_words=int(sizes[3]), bytes_per_env=int(sizes[4]))
            K = int(d["num_rows"])
            words, bytes_, rows = d["words"], d["bytes"], d["rows"]
            if words.shape != (layout["word_rows"], K) or bytes_.shape != (layout["byte_rows"], K) or rows.shape != (layout["row_words"] * K,) \
                    or words.dtype != np.int32 or bytes_.dtype != np.uint8 or rows.dtype != np.int32:
                raise ValueError(f"{path}: the sections do not have the sizes of the header")
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
            return cls(layout, K, t(d["env_ids"]) if "env_ids" in d.files else None, int(d["counter"]), bool(d["whole"]), t(words), t(bytes_),
                       t(rows), t(d["glob"]) if "glob" in d.files else None)


def _host_ids(ids, what, limit, distinct):
    """ids given by the caller (a list, an array or a tensor) as a contiguous int32 numpy array, checked on the host"""
    a = np.asarray(torch.as_tensor(ids).cpu(), dtype=np.int64).reshape(-1)
    if a.size == 0:
        raise ValueError(f"{what}: no entries")
    if a.min() < 0 or a.max() >= limit:
        raise ValueError(f"{what}: entries have to lie in [0, {limit})")
    if distinct and np.unique(a).size != a.size:
        raise ValueError(f"{what}: an environment is named twice")
    return a.astype(np.int32)


class Go1State:
    """Save and restore of one simulator instance.  S: its Go1SimConfig, buffers: its SimBuffers, sim: its Go1Sim (the ring positions and
    the step counter are host values of the handle: nothing is read from the device)."""

    def __init__(self, S, buffers, sim, lib=None):
        self.lib = lib if lib is not None else load_library()
        self.S, self.buffers, self.sim = S, buffers, sim
        self.device = buffers.device
        self.cfg = state_config(S)
        self.layout = layout_of(self.cfg, self.lib)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=self.device)      # entries the kernels skipped (ids out of range)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if self.device.type == "cuda" else None

    def _phase(self):
        """(step counter, lag_head, history_slot) of the handle"""
        counter, lag_head = self.sim.counters()
        no, R = int(self.S.num_obs), int(self.S.num_obs_history) + 1
        return int(counter), int(lag_head), (self.sim.history_window_offset() // no - 1) % R

    def _snapshot(self, state):
        snap = Go1StateSnapshot()
        for i, v in enumerate(state.layout["header"]):
            snap.header[i] = int(v)
        snap.num_rows = state.num_rows
        snap.words, snap.bytes, snap.rows = state.words.data_ptr(), state.bytes.data_ptr(), state.rows.data_ptr()
        snap.skipped = self.skipped.data_ptr()
        setattr(snap, "global", state.glob.data_ptr() if state.glob is not None else None)
        return snap

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc} ({RETURN_CODES.get(rc, '?')})")

    def _ids(self, a):
        t = torch.from_numpy(a).to(self.device)
        return t, ctypes.c_void_p(t.data_ptr())

    def capture(self, env_ids=None):
        """the state of the environments `env_ids` (None: all, and the global section with them) as a SimState on the buffers' device: one
        launch (two for all)"""
        L, N = self.layout, int(self.cfg.num_envs)
        ids = ids_ptr = None
        K = N
        if env_ids is not None:
            ids, ids_ptr = self._ids(_host_ids(env_ids, "save_state(env_ids)", N, distinct=False))
            K = ids.numel()
        z = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=self.device)       # noqa: E731
        counter, lag_head, hslot = self._phase()
        state = SimState(L, K, ids, counter, env_ids is None, z(L["word_rows"], K), z(L["byte_rows"], K, dtype=torch.uint8), z(L["row_words"] * K),
                         z(L["global_words"]) if env_ids is None else None)
        snap = self._snapshot(state)
        self._check(self.lib.go1state_capture(ctypes.byref(self.cfg), ctypes.byref(self.buffers.struct), ids_ptr, K, lag_head, hslot,
                                              ctypes.byref(snap), self._stream()), "go1state_capture")
        if state.whole:
            self._check(self.lib.go1state_capture_global(ctypes.byref(self.cfg), ctypes.byref(self.buffers.struct), ctypes.byref(snap),
                                                         self._stream()), "go1state_capture_global")
        return state

    def restore(self, state, env_ids=None, rows=None, restore_global=False):
        """snapshot row rows[k] (None: k) into environment env_ids[k] (None: the environments in order), re-phased to the handle's current
        ring positions: one launch (two with the global section)"""
        N = int(self.cfg.num_envs)
        if not np.array_equal(np.asarray(state.layout["header"]), self.layout["header"]):
            raise RuntimeError("load_state(): the state was saved from another layout "
                               f"({dict(zip(HEADER_NAMES, np.asarray(state.layout['header']).tolist()))} against "
                               f"{dict(zip(HEADER_NAMES, self.layout['header'].tolist()))})")
        if state.device != self.device:
            raise RuntimeError(f"load_state(): the state is on {state.device}, the simulator's buffers on {self.device}: move it with .to()")
        dst = dst_ptr = src = src_ptr = None
        K = N
        if env_ids is not None:
            dst, dst_ptr = self._ids(_host_ids(env_ids, "load_state(env_ids)", N, distinct=True))
            K = dst.numel()
        if rows is not None:
            src, src_ptr = self._ids(_host_ids(rows, "load_state(rows)", state.num_rows, distinct=False))
            if src.numel() != K:
                raise ValueError(f"load_state(): {src.numel()} rows for {K} environments")
        elif K > state.num_rows:
            raise ValueError(f"load_state(): {K} environments from a state of {state.num_rows} rows: name the rows")
        if restore_global and state.glob is None:
            raise RuntimeError("load_state(): the state carries no global section (it was not saved with env_ids=None)")
        _, lag_head, hslot = self._phase()
        snap = self._snapshot(state)
        self._keep = (dst, src, state)          # alive until the next call: the launch reads them
        self._check(self.lib.go1state_restore(ctypes.byref(self.cfg), ctypes.byref(self.buffers.struct), dst_ptr, src_ptr, K, lag_head, hslot,
                                              ctypes.byref(snap), self._stream()), "go1state_restore")
        if restore_global:
            self._check(self.lib.go1state_restore_global(ctypes.byref(self.cfg), ctypes.byref(self.buffers.struct), ctypes.byref(snap),
                                                         self._stream()), "go1state_restore_global")
