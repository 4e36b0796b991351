"""numpy model of include/go1state.h, written from the header's text: capture (gather into the packed sections) and restore (scatter, re-phased)
over a dict {buffer name: numpy array in the simulator's layout}.  It knows the classification only through the lists it is handed
(go1state_host.PER_ENV / GLOBAL) and the declaration order of include/go1sim.h; the offsets, the logical ring orders, the double history
write, the byte section, fan-out and the skipped entries are restated here.  TEST INFRASTRUCTURE."""
import numpy as np

ROWS_ORDER = ["obs_buf", "obs_history", "privileged_obs_buf"]


def u32(a):
    """a 4-byte array's bits"""
    return np.ascontiguousarray(a).view(np.uint32)


def scripted(arrays, salt=0):
    """fill every array in place: every word is a hash of (field, flat position in the simulator's layout, salt), every byte likewise (its low
    byte).  Floats get arbitrary bit patterns, NaNs and infinities among them: the copies move bits."""
    for f, name in enumerate(sorted(arrays)):
        a = arrays[name]
        if a is None:
            continue
        i = np.arange(a.size, dtype=np.uint64)
        h = (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) ^ np.uint64((f + 1) * 0x85EBCA6B + salt * 0xC2B2AE35)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
        if a.dtype.itemsize == 1:
            a.reshape(-1)[:] = (h & np.uint64(0xFF)).astype(np.uint8)
        elif a.dtype.itemsize == 2:
            a.reshape(-1).view(np.uint16)[:] = (h & np.uint64(0xFFFF)).astype(np.uint16)
        else:
            a.reshape(-1).view(np.uint32)[:] = (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return arrays


class Model:
    """order: the declaration order of Go1SimBuffers; per_env: {name: "words" | "lag" | "bytes" | "rows" | "history"}; global_order: the global
    section's fields; num_obs, num_obs_history, lag_timesteps: the three values the rings depend on"""

    def __init__(self, order, per_env, global_order, num_obs, num_obs_history, lag_timesteps):
        self.words = [n for n in order if per_env.get(n) in ("words", "lag")]
        self.bytes = [n for n in order if per_env.get(n) == "bytes"]
        self.rows = list(ROWS_ORDER)
        assert sorted(self.rows) == sorted(n for n in order if per_env.get(n) in ("rows", "history"))
        self.kind, self.glob = dict(per_env), list(global_order)
        self.no, self.R, self.lag_n = int(num_obs), int(num_obs_history) + 1, int(lag_timesteps) + 1

    # ---- the layout
    def rows_of(self, arrays, name, N):
        a = arrays[name]
        if self.kind[name] == "history":
            assert a.shape == (N, 2 * self.R * self.no)
            return self.R * self.no
        if self.kind[name] == "rows":
            assert a.shape[0] == N and a.ndim == 2
            return a.shape[1]
        assert a.shape[-1] == N
        return a.size // N

    def sizes(self, arrays, N):
        """(W, B, row words, G)"""
        return (sum(self.rows_of(arrays, n, N) for n in self.words), sum(self.rows_of(arrays, n, N) for n in self.bytes),
                sum(self.rows_of(arrays, n, N) for n in self.rows), sum(arrays[n].size for n in self.glob))

    # ---- the simulator's side of one environment's field, in the snapshot's (logical) order
    def _lag_rows(self, lag_head):
        return np.array([((lag_head + i) % self.lag_n) * 12 + j for i in range(self.lag_n) for j in range(12)])

    def _hist_cols(self, hslot):
        return np.concatenate([((hslot + 1 + ls) % self.R) * self.no + np.arange(self.no) for ls in range(self.R)])

    def capture(self, arrays, ids, lag_head, hslot):
        """ids: a list of environment indices or None (all).  Returns {"words": (W, K) uint32, "bytes": (B, K) uint8, "rows": (row words * K,)
        uint32, "skipped": entries whose id lies outside [0, N): their rows stay zero}"""
        N = arrays["root_states"].shape[-1]
        ids = np.arange(N) if ids is None else np.asarray(ids, dtype=np.int64)
        K = len(ids)
        ok = (ids >= 0) & (ids < N)
        W, Bt, RW, _ = self.sizes(arrays, N)
        words, bytes_, rows = np.zeros((W, K), np.uint32), np.zeros((Bt, K), np.uint8), np.zeros(RW * K, np.uint32)
        off = 0
        for n in self.words:
            a = u32(arrays[n]).reshape(-1, N)
            if self.kind[n] == "lag":
                a = a[self._lag_rows(lag_head)]
            words[off:off + len(a), ok] = a[:, ids[ok]]
            off += len(a)
        off = 0
        for n in self.bytes:
            a = arrays[n].reshape(-1, N)
            bytes_[off:off + len(a), ok] = a[:, ids[ok]]
            off += len(a)
        off = 0
        for n in self.rows:
            a = u32(arrays[n])
            if self.kind[n] == "history":
                a = a[:, self._hist_cols(hslot)]
            block = rows[off * K:(off + a.shape[1]) * K].reshape(K, a.shape[1])
            block[ok] = a[ids[ok]]
            off += a.shape[1]
        return dict(words=words, bytes=bytes_, rows=rows, skipped=int((~ok).sum()))

    def capture_global(self, arrays):
        return np.concatenate([u32(arrays[n]).reshape(-1) for n in self.glob])

    def restore(self, arrays, snap, dst, src_rows, lag_head, hslot):
        """scatter snapshot row src_rows[k] (None: k) into environment dst[k] (None: k) of `arrays`, in place, at the ring positions given.
        Returns the number of skipped entries (a destination outside [0, N) or a row outside [0, K))."""
        N = arrays["root_states"].shape[-1]
        Ks = snap["words"].shape[1]
        dst = np.arange(N) if dst is None else np.asarray(dst, dtype=np.int64)
        src = np.arange(len(dst)) if src_rows is None else np.asarray(src_rows, dtype=np.int64)
        assert len(src) == len(dst)
        ok = (dst >= 0) & (dst < N) & (src >= 0) & (src < Ks)
        d, s = dst[ok], src[ok]
        off = 0
        for n in self.words:
            a = u32(arrays[n]).reshape(-1, N)          # (a view: the writes land in `arrays`)
            rows = self._lag_rows(lag_head) if self.kind[n] == "lag" else np.arange(len(a))
            a[np.ix_(rows, d)] = snap["words"][off:off + len(a)][:, s]
            off += len(a)
        off = 0
        for n in self.bytes:
            a = arrays[n].reshape(-1, N)
            a[:, d] = snap["bytes"][off:off + len(a)][:, s]
            off += len(a)
        off = 0
        for n in self.rows:
            a = u32(arrays[n])
            cols = self.R * self.no if self.kind[n] == "history" else a.shape[1]
            block = snap["rows"][off * Ks:(off + cols) * Ks].reshape(Ks, cols)[s]
            if self.kind[n] == "history":
                p = self._hist_cols(hslot)
                a[np.ix_(d, p)] = block
                a[np.ix_(d, p + cols)] = block                 # both copies of every slot
            else:
                a[d] = block
            off += cols
        return int((~ok).sum())

    def restore_global(self, arrays, glob):
        off = 0
        for n in self.glob:
            k = arrays[n].size
            u32(arrays[n]).reshape(-1)[:] = glob[off:off + k]
            off += k
