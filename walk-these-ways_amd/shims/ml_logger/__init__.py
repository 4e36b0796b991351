"""Local stand-in for the `ml_logger` package: the subset of `logger` the Go1 scripts and
the Runner use, writing under a local root instead of a remote instrument server."""
import contextlib
import datetime
import os
import pickle
import shutil
import time
from collections import defaultdict


class _Logger:
    def __init__(self):
        self.root = None
        self.prefix = "."
        self._metrics = defaultdict(list)
        self._metric_prefix = ""
        self._timers = {}
        self._counters = defaultdict(int)
        self.print_summary = True

    # ---- configuration -------------------------------------------------------------------------
    def configure(self, prefix=None, root=None, **kw):
        self.root = str(root) if root is not None else os.path.abspath("runs")
        self.prefix = prefix or "."
        os.makedirs(self._path(""), exist_ok=True)
        # a new run: nothing of the previous one (pending metrics, `every` phases, timers) carries over
        self._metrics.clear()
        self._counters.clear()
        self._timers.clear()

    def utcnow(self, fmt="%Y-%m-%d/%H%M%S.%f"):
        return datetime.datetime.utcnow().strftime(fmt)

    def _path(self, key):
        return os.path.join(self.root or os.path.abspath("runs"), self.prefix, key)

    # ---- text / params ---------------------------------------------------------------------------
    def log_text(self, text, filename="text.log", dedent=False, **kw):
        if dedent:
            import textwrap
            text = textwrap.dedent(text)
        p = self._path(filename)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "a") as f:
            f.write(text)

    def log_params(self, path="parameters.pkl", **kwargs):
        self.save_pkl(kwargs, path)

    def save_pkl(self, data, path, append=False):
        p = self._path(path)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "ab" if append else "wb") as f:
            pickle.dump(data, f)

    def load_pkl(self, path):
        out = []
        with open(self._path(path), "rb") as f:
            while True:
                try:
                    out.append(pickle.load(f))
                except EOFError:
                    return out

    # ---- timers ------------------------------------------------------------------------------------
    def start(self, *keys):
        now = time.perf_counter()
        for k in keys:
            self._timers[k] = now

    def since(self, key):
        return time.perf_counter() - self._timers.get(key, time.perf_counter())

    def split(self, key):
        now = time.perf_counter()
        last = self._timers.get(key, now)
        self._timers[key] = now
        return now - last

    def every(self, n, key="default", start_on=0):
        self._counters[key] += 1
        return (self._counters[key] - start_on) % n == 0 and self._counters[key] >= start_on

    # ---- metrics -------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def Prefix(self, *a, metrics=None, **kw):
        old = self._metric_prefix
        if metrics:
            self._metric_prefix = metrics.rstrip("/") + "/"
        try:
            yield
        finally:
            self._metric_prefix = old

    def store_metrics(self, **kv):
        for k, v in kv.items():
            self._metrics[self._metric_prefix + k].append(v)

    def log_metrics_summary(self, key_values=None, **kw):
        summary = dict(key_values or {})
        for k, vals in self._metrics.items():
            try:
                nums = [float(v) for v in vals]
                summary[k + "/mean"] = sum(nums) / max(len(nums), 1)
            except (TypeError, ValueError):
                pass
        self._metrics.clear()
        self.save_pkl(summary, "metrics.pkl", append=True)
        if self.print_summary:
            keys = ["iterations", "timesteps", "train/episode/rew_total/mean", "adaptation_loss/mean", "time_iter/mean"]
            print(" | ".join(f"{k}={summary[k]:.4g}" for k in keys if k in summary))
        return summary

    def job_running(self):
        pass

    @contextlib.contextmanager
    def Sync(self):
        yield

    # ---- artefacts -------------------------------------------------------------------------------------
    def torch_save(self, obj, path):
        import torch
        p = self._path(path)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        torch.save(obj, p)

    def load_torch(self, path, **kw):
        import torch
        return torch.load(self._path(path), **kw)

    def duplicate(self, src, dst):
        shutil.copyfile(self._path(src), self._path(dst))

    def upload_file(self, file_path, target_path, once=True):
        dst = self._path(os.path.join(target_path, os.path.basename(file_path)))
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(file_path, dst)

    def save_video(self, frames, path, fps=30):
        """Write `frames` ((H, W, 3 or 4) uint8 arrays) as an animated PNG at `path` with its suffix replaced by .png (no mp4 encoder
        offline; browsers play APNG).  Encoded on a background (non-daemon) thread, which is returned: join() it to wait for the file."""
        import threading
        import numpy as np
        frames = [np.asarray(f) for f in frames]
        p = os.path.splitext(self._path(path))[0] + ".png"
        os.makedirs(os.path.dirname(p), exist_ok=True)
        t = threading.Thread(target=write_apng, args=(p, frames, fps), name="save_video", daemon=False)
        t.start()
        return t


def _chunk(kind, data):
    import struct
    import zlib
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_apng(path, frames, fps, level=6):
    """Animated PNG (APNG) with zlib and struct only: signature, IHDR, acTL, then per frame fcTL (delay 1/fps as a fraction) and
    IDAT (first frame) or fdAT (the others) with one shared sequence number, IEND.  8-bit RGBA (RGB frames get alpha 255), every
    frame full size, filter type 0 on every row."""
    import struct
    import zlib
    from fractions import Fraction
    import numpy as np
    if len(frames) == 0:
        raise ValueError("save_video: no frames")
    h, w = frames[0].shape[:2]
    sec = 1.0 / float(fps)
    delay = Fraction(sec).limit_denominator(max(1, min(65535, int(65535 / max(sec, 1.0)))))      # both terms fit 16 bits
    num, den = delay.numerator, delay.denominator
    out = [b"\x89PNG\r\n\x1a\n", _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)),
           _chunk(b"acTL", struct.pack(">II", len(frames), 0))]
    seq = 0
    for i, f in enumerate(frames):
        f = np.ascontiguousarray(f, dtype=np.uint8)
        if f.shape[:2] != (h, w):
            raise ValueError(f"save_video: frame {i} is {f.shape[:2]}, frame 0 is {(h, w)}")
        if f.ndim == 3 and f.shape[2] == 3:
            f = np.concatenate([f, np.full((h, w, 1), 255, np.uint8)], axis=2)
        raw = np.zeros((h, 1 + 4 * w), np.uint8)          # filter byte 0, then the row
        raw[:, 1:] = f.reshape(h, 4 * w)
        data = zlib.compress(raw.tobytes(), level)
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, num, den, 0, 0)))
        seq += 1
        if i == 0:
            out.append(_chunk(b"IDAT", data))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    tmp = path + ".part"
    with open(tmp, "wb") as fh:
        fh.writelines(out)
    os.replace(tmp, path)


logger = _Logger()
ML_Logger = _Logger
