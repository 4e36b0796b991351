"""Host side of the renderer C-ABI (include/go1render.h): ctypes mirror, library loading, and `Go1Render`, which owns the
per-camera device control blocks and frame rings of a recording.

The recording follows the reference (go1_gym/envs/base/legged_robot.py start_recording / _render_headless / reset_idx,
:1003-1015, :1622-1673) but keeps its state on the device: after each step `record()` enqueues the state launch and the
frame launch, and the host learns that a recording is complete only when it asks (`complete_frames`, one small read).
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgo1render.so")

W, H = 360, 240
FRAME_BYTES = W * H * 4
MAX_CAMERAS = 2
IDLE, WAITING, RECORDING, COMPLETE = 0, 1, 2, 3
CONTROL_WORDS = 8                 # int32 words of Go1RecordControl


class Go1RecordControl(ctypes.Structure):
    _fields_ = [("env", ctypes.c_int32), ("state", ctypes.c_int32), ("frames", ctypes.c_int32), ("capacity", ctypes.c_int32),
                ("slot", ctypes.c_int32), ("pad", ctypes.c_int32 * 3)]


class Go1RenderConfig(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("num_cameras", ctypes.c_int32), ("terrain_type", ctypes.c_int32),
                ("hf_rows", ctypes.c_int32), ("hf_cols", ctypes.c_int32),
                ("hf_hscale", ctypes.c_float), ("hf_vscale", ctypes.c_float), ("hf_border", ctypes.c_float),
                ("hf_zmin", ctypes.c_float), ("hf_zmax", ctypes.c_float)]


class Go1RenderBuffers(ctypes.Structure):
    _fields_ = [("root_states", ctypes.c_void_p), ("dof_pos", ctypes.c_void_p), ("reset_buf", ctypes.c_void_p),
                ("height_samples", ctypes.c_void_p), ("control", ctypes.c_void_p), ("frames", ctypes.c_void_p * MAX_CAMERAS)]


EXPORTED_SYMBOLS = ["go1render_record", "go1render_note_reset", "go1render_image", "go1render_version"]

_lib = None


class Go1RenderLibraryMissing(RuntimeError):
    pass


def load_library(path=None):
    """Load libgo1render.so (HIP, gfx950).  Fails loudly: there is no CPU renderer."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise Go1RenderLibraryMissing(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(hipcc --offload-arch=gfx950). Recording videos has no CPU fallback.")
    lib = ctypes.CDLL(p)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    cfg_p, buf_p = ctypes.POINTER(Go1RenderConfig), ctypes.POINTER(Go1RenderBuffers)
    lib.go1render_record.argtypes = [cfg_p, buf_p, vp]
    lib.go1render_note_reset.argtypes = [cfg_p, buf_p, vp, i32, vp]
    lib.go1render_image.argtypes = [cfg_p, buf_p, i32, vp, vp]
    for fn in ("go1render_record", "go1render_note_reset", "go1render_image"):
        getattr(lib, fn).restype = ctypes.c_int
    lib.go1render_version.restype = ctypes.c_char_p
    if path is None:
        _lib = lib
    return lib


class Go1Render:
    """Renderer of one simulator instance: `image(env)` draws now; cameras 0..num_cameras-1 record episodes of one env each.

    S: the simulator's Go1SimConfig (terrain fields), buffers: its SimBuffers (device tensors).  Frame rings are allocated by
    the first `arm()` of a camera and reused afterwards."""

    def __init__(self, S, buffers, num_cameras=1, lib=None):
        assert 1 <= num_cameras <= MAX_CAMERAS
        self.lib = lib if lib is not None else load_library()
        self.buffers = buffers
        self.device = buffers.device
        c = self.cfg = Go1RenderConfig()
        c.num_envs, c.num_cameras = int(S.num_envs), int(num_cameras)
        hs = buffers.tensors.get("height_samples")
        c.terrain_type = int(S.terrain_type) if hs is not None else 0
        if c.terrain_type:
            c.hf_rows, c.hf_cols = int(S.hf_rows), int(S.hf_cols)
            c.hf_hscale, c.hf_vscale, c.hf_border = float(S.hf_hscale), float(S.hf_vscale), float(S.hf_border)
            lo, hi = int(hs.min()), int(hs.max())            # (once, at the first recording or render())
            c.hf_zmin, c.hf_zmax = lo * float(np.float32(S.hf_vscale)), hi * float(np.float32(S.hf_vscale))
            # the kernel compares fp32 heights (sample * vscale) with these bounds: widen by a rounding margin
            pad = 1e-4 + 1e-6 * max(abs(c.hf_zmin), abs(c.hf_zmax))
            c.hf_zmin, c.hf_zmax = c.hf_zmin - pad, c.hf_zmax + pad
        self.control = torch.zeros(num_cameras, CONTROL_WORDS, dtype=torch.int32, device=self.device)
        self.rings = [None] * num_cameras
        self.armed = [False] * num_cameras
        self._image = None
        self.buf = Go1RenderBuffers()
        self._refresh()

    def _refresh(self):
        b, B = self.buf, self.buffers
        b.root_states, b.dof_pos, b.reset_buf = B.root_states.data_ptr(), B.dof_pos.data_ptr(), B.reset_buf.data_ptr()
        hs = B.tensors.get("height_samples")
        b.height_samples = hs.data_ptr() if (hs is not None and self.cfg.terrain_type) else None
        b.control = self.control.data_ptr()
        for i, r in enumerate(self.rings):
            b.frames[i] = r.data_ptr() if r is not None else None

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc}")

    @property
    def any_armed(self):
        return any(self.armed)

    def arm(self, cam, env, capacity):
        """start a recording of `env` on camera `cam`: waiting for the env's next reset (a running recording is dropped)"""
        capacity = int(capacity)
        if self.rings[cam] is None or self.rings[cam].shape[0] < capacity:
            self.rings[cam] = torch.empty(capacity, H, W, 4, dtype=torch.uint8, device=self.device)
        self.control[cam] = torch.tensor([int(env), WAITING, 0, capacity, -1, 0, 0, 0], dtype=torch.int32)
        self.armed[cam] = True
        self._refresh()

    def disarm(self, cam):
        """stop recording on `cam` (its ring is kept for the next recording)"""
        self.control[cam, 1] = IDLE
        self.armed[cam] = False

    def record(self):
        """after a step: advance the armed cameras' states from reset_buf and draw their frames (two launches, no sync)"""
        self._check(self.lib.go1render_record(ctypes.byref(self.cfg), ctypes.byref(self.buf), self._stream()), "go1render_record")

    def note_reset(self, ids=None):
        """a host reset_idx(ids) (None: every env) is a recording boundary of the recorded env (scanned on the device)"""
        if ids is None:
            rc = self.lib.go1render_note_reset(ctypes.byref(self.cfg), ctypes.byref(self.buf), None, 0, self._stream())
        else:
            ids = torch.as_tensor(ids, device=self.device).to(torch.int32).contiguous()
            self._keep = ids
            rc = self.lib.go1render_note_reset(ctypes.byref(self.cfg), ctypes.byref(self.buf), ctypes.c_void_p(ids.data_ptr()),
                                               ids.numel(), self._stream())
        self._check(rc, "go1render_note_reset")

    def status(self):
        """(state, frames) per camera: one small device-to-host read"""
        c = self.control[:, :3].cpu()
        return [(int(c[i, 1]), int(c[i, 2])) for i in range(c.shape[0])]

    def complete_frames(self, cam, status=None):
        """the frames of a complete recording as a list of (H, W, 4) uint8 arrays (one device-to-host copy), else None"""
        state, frames = (status or self.status())[cam]
        if state != COMPLETE:
            return None
        self.armed[cam] = False
        if frames == 0:
            return []
        arr = self.rings[cam][:frames].cpu().numpy()
        return list(arr)

    def image(self, env):
        """draw `env` now: (H, W, 4) uint8 device tensor (reused by the next call)"""
        if self._image is None:
            self._image = torch.empty(H, W, 4, dtype=torch.uint8, device=self.device)
        self._check(self.lib.go1render_image(ctypes.byref(self.cfg), ctypes.byref(self.buf), int(env),
                                             ctypes.c_void_p(self._image.data_ptr()), self._stream()), "go1render_image")
        return self._image
