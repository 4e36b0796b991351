// go1state.hip — gather and scatter of the simulator's state (include/go1state.h), gfx950.
//
// One kernel, state_kernel<RESTORE>, driven by a field table in kernel-argument memory: a line per simulator buffer (pointer, kind,
// rows, offset in its packed section, first tile).  The work is cut into tiles of 256 elements; a tile belongs to one field, so the
// table walk that finds it is uniform over the workgroup and stays on the scalar unit.  The grid is capped at GO1STATE_MAX_BLOCKS
// workgroups, each striding over the tiles.
//   SoA fields (words, the lag ring, bytes): a tile is 256 consecutive entries of one row, the environment fastest: with contiguous ids
//     a wavefront reads 64 consecutive words and writes 64 consecutive words.  Bytes move as bytes (one writer per byte, the neighbours'
//     bytes are not touched).
//   Row-major fields (obs_buf, obs_history, privileged_obs_buf): a tile is 256 consecutive vector elements of the packed block, the column
//     fastest.  The vector is 8 bytes where the row pitch, the packed offset and the pointer prove it aligned (70 observations: rows of
//     280 bytes are 8-byte aligned, not 16), 4 bytes otherwise (odd num_obs).
//   Global fields: flat runs of words.
// No LDS, no cross-lane operation, no atomics but the count of skipped entries; every destination word has one writer as long as the
// destinations are distinct.  A buffer added to Go1SimBuffers later is one line in fields().
#include "../../include/go1state.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int T = 256, MAX_FIELDS = 64;
struct alignas(8) Pair { uint32_t x, y; };            // the 8-byte vector of the row-major fields
enum Kind : int32_t { K_WORD = 0, K_LAG = 1, K_BYTE = 2, K_ROWS = 3, K_HIST = 4, K_FLAT = 5 };

struct Field {
  void* ptr;        // the simulator's buffer
  int32_t kind;
  int32_t rows;     // SoA: rows; row-major: packed columns per environment; flat: words
  int32_t off;      // SoA: first row in the section; row-major: columns in front of it; flat: first word
  int32_t vec;      // row-major: words per vector element (1 or 2)
  int32_t tile0;    // its first tile
  int32_t pad;
};

struct Plan {
  Field f[MAX_FIELDS];
  int32_t nf, tiles, grid;
  int32_t N, K, Ks;                     // environments of the buffers, entries of this call, rows of the snapshot
  int32_t lag_n, lag_head, R, hslot, no;
  const int32_t* ids;                   // capture: sources; restore: destinations
  const int32_t* src_rows;
  uint32_t* words;
  uint8_t* bytes;
  uint32_t* rows;
  uint32_t* global;
  uint32_t* skipped;
};
static_assert(sizeof(Plan) <= 4096, "the plan is a kernel argument");

// entry k of the call: its environment e and snapshot row s; false (and, for `count`, one more skipped entry) when either is out of range
template <bool RESTORE>
__device__ __forceinline__ bool resolve(const Plan& P, int k, int* e, int* s, bool count) {
  *e = P.ids ? P.ids[k] : k;
  *s = (RESTORE && P.src_rows) ? P.src_rows[k] : k;
  const bool ok = *e >= 0 && *e < P.N && *s >= 0 && *s < P.Ks;
  if (!ok && count) atomicAdd(P.skipped, 1u);
  return ok;
}

template <class V>
__device__ __forceinline__ void move_rows(const Plan& P, const Field& F, bool restore, size_t sim, size_t packed) {
  V* a = (V*)((uint32_t*)F.ptr + sim);
  V* b = (V*)(P.rows + packed);
  if (restore) {
    const V v = *b;
    *a = v;
    if (F.kind == K_HIST) *(V*)((uint32_t*)F.ptr + sim + F.rows) = v;       // the slot's second copy, R * num_obs words on
  } else {
    *b = *a;
  }
}

}  // namespace

template <bool RESTORE>
__global__ void __launch_bounds__(T) state_kernel(const Plan P) {
  const int t = (int)threadIdx.x;
  for (int tile = (int)blockIdx.x; tile < P.tiles; tile += P.grid) {
    int fi = 0;
    while (fi + 1 < P.nf && tile >= P.f[fi + 1].tile0) fi++;
    const Field F = P.f[fi];
    const int lt = tile - F.tile0;
    if (F.kind <= K_BYTE) {
      const int per_row = (P.K + T - 1) / T;
      const int r = lt / per_row, k = (lt % per_row) * T + t;
      if (k >= P.K) continue;
      int e, s;
      if (!resolve<RESTORE>(P, k, &e, &s, fi == 0 && r == 0)) continue;    // (field 0 is root_states: every entry is counted once)
      int pr = r;
      if (F.kind == K_LAG) pr = ((P.lag_head + r / 12) % P.lag_n) * 12 + r % 12;
      const size_t sim = (size_t)pr * P.N + e, packed = (size_t)(F.off + r) * P.Ks + s;
      if (F.kind == K_BYTE) {
        uint8_t* a = (uint8_t*)F.ptr + sim;
        if (RESTORE) *a = P.bytes[packed]; else P.bytes[packed] = *a;
      } else {
        uint32_t* a = (uint32_t*)F.ptr + sim;
        if (RESTORE) *a = P.words[packed]; else P.words[packed] = *a;
      }
    } else if (F.kind == K_FLAT) {
      const int i = lt * T + t;
      if (i >= F.rows) continue;
      uint32_t* a = (uint32_t*)F.ptr + i;
      if (RESTORE) *a = P.global[F.off + i]; else P.global[F.off + i] = *a;
    } else {
      const uint32_t cv = (uint32_t)(F.rows / F.vec);                       // vector elements per environment
      const uint64_t i = (uint64_t)lt * T + t, total = (uint64_t)P.K * cv;
      if (i >= total) continue;
      const uint32_t k = total >> 32 ? (uint32_t)(i / cv) : (uint32_t)i / cv;
      const int c = (int)(i - (uint64_t)k * cv) * F.vec;
      int e, s;
      if (!resolve<RESTORE>(P, (int)k, &e, &s, false)) continue;
      int pc = c;
      size_t pitch = (size_t)F.rows;
      if (F.kind == K_HIST) {                                               // logical slot c / num_obs is slot (history_slot + 1 + .) % R
        pc = ((P.hslot + 1 + c / P.no) % P.R) * P.no + c % P.no;
        pitch *= 2;
      }
      const size_t sim = (size_t)e * pitch + pc, packed = (size_t)F.off * P.Ks + (size_t)s * F.rows + c;
      if (F.vec == 2) move_rows<Pair>(P, F, RESTORE, sim, packed);
      else move_rows<uint32_t>(P, F, RESTORE, sim, packed);
    }
  }
}

// ---- the host side: the layout, the field table, the validation in the order the header gives the codes, one launch -------------------------
namespace {

bool in_range(const Go1StateConfig* c) {
  const int64_t cur = (int64_t)c->num_categories * c->num_bins * c->curriculum_update_interval;
  return c->num_obs > 0 && c->num_obs <= (1 << 16) && c->num_privileged_obs >= 0 && c->num_privileged_obs <= (1 << 16) &&
         c->num_obs_history >= 0 && c->num_obs_history <= 4096 && (int64_t)(c->num_obs_history + 1) * c->num_obs <= (1 << 24) &&
         c->lag_timesteps >= 0 && c->lag_timesteps < GO1_MAX_LAG && c->num_rewards >= 0 && c->num_rewards <= 4096 &&
         c->num_height_points >= 0 && c->num_height_points <= (1 << 16) && c->command_rows > 0 && c->command_rows <= 4096 &&
         c->num_categories > 0 && c->num_bins > 0 && c->curriculum_update_interval > 0 && cur <= (1 << 28);
}

void header_of(const Go1StateConfig* c, int32_t* h) {
  const int32_t v[GO1STATE_HEADER_WORDS] = {GO1STATE_MAGIC, GO1STATE_LAYOUT_VERSION, c->num_obs, c->num_privileged_obs, c->num_obs_history,
                                            c->lag_timesteps, c->num_rewards, c->num_height_points, c->command_rows, c->num_categories,
                                            c->num_bins, c->curriculum_update_interval};
  for (int i = 0; i < GO1STATE_HEADER_WORDS; i++) h[i] = v[i];
}

bool same_header(const Go1StateConfig* c, const int32_t* h) {
  int32_t mine[GO1STATE_HEADER_WORDS];
  header_of(c, mine);
  for (int i = 0; i < GO1STATE_HEADER_WORDS; i++)
    if (mine[i] != h[i]) return false;
  return true;
}

// the field table of a call.  `b` may be NULL (the layout alone).  K entries against a snapshot of Ks rows.
struct Table {
  Plan P;
  Go1StateLayout L;
  bool missing;
};

bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

void fields(const Go1StateConfig* c, const Go1SimBuffers* b, int K, int Ks, bool global, Table* tb) {
  Plan& P = tb->P;
  P = Plan{};
  tb->missing = false;
  int words = 0, bytes = 0, cols = 0, flat = 0;
  int64_t tiles = 0;
  const int per_row = (K + T - 1) / T;
  const bool per_env = !global;
  // one line: SoA words / the lag ring / bytes
  auto soa = [&](const void* p, int kind, int rows, bool optional) {
    int& off = kind == K_BYTE ? bytes : words;
    if (per_env && b && p) {
      Field& F = P.f[P.nf++];
      F.ptr = (void*)p; F.kind = kind; F.rows = rows; F.off = off; F.vec = 1; F.tile0 = (int32_t)tiles;
      tiles += (int64_t)rows * per_row;
    } else if (per_env && b && !optional) {
      tb->missing = true;
    }
    off += rows;
  };
  auto rowmajor = [&](const void* p, int kind, int n) {
    if (per_env && b && p) {
      Field& F = P.f[P.nf++];
      F.ptr = (void*)p; F.kind = kind; F.rows = n; F.off = cols; F.tile0 = (int32_t)tiles;
      const bool even = n % 2 == 0 && ((int64_t)cols * Ks) % 2 == 0 && aligned8(p) && (kind != K_HIST || c->num_obs % 2 == 0);
      F.vec = even ? 2 : 1;
      tiles += ((int64_t)K * (n / F.vec) + T - 1) / T;
    } else if (per_env && b) {
      tb->missing = true;
    }
    cols += n;
  };
  auto run = [&](const void* p, int64_t n, bool optional) {
    if (global && b && p) {
      Field& F = P.f[P.nf++];
      F.ptr = (void*)p; F.kind = K_FLAT; F.rows = (int32_t)n; F.off = flat; F.vec = 1; F.tile0 = (int32_t)tiles;
      tiles += (n + T - 1) / T;
    } else if (global && b && !optional) {
      tb->missing = true;
    }
    flat += (int32_t)n;
  };
#define W(name, rows) soa(b ? b->name : nullptr, K_WORD, (rows), false)
#define B8(name, rows) soa(b ? b->name : nullptr, K_BYTE, (rows), false)
  const int nr = c->num_rewards;
  W(root_states, 13); W(dof_pos, 12); W(dof_vel, 12); W(contact_forces, 51); W(foot_positions, 12); W(foot_velocities, 12);
  W(prev_foot_velocities, 12);
  soa(b ? b->lag_buffer : nullptr, K_LAG, 12 * (c->lag_timesteps + 1), false);
  W(joint_pos_err_last, 12); W(joint_pos_err_last_last, 12); W(joint_vel_last, 12); W(joint_vel_last_last, 12);
  W(joint_pos_target, 12); W(last_joint_pos_target, 12); W(last_last_joint_pos_target, 12);
  W(actions, 12); W(last_actions, 12); W(last_last_actions, 12); W(last_dof_vel, 12); W(torques, 12);
  W(base_lin_vel, 3); W(base_ang_vel, 3); W(projected_gravity, 3);
  W(commands, c->command_rows); W(gait_indices, 1); W(clock_inputs, 4); W(desired_contact_states, 4); W(foot_indices, 4);
  W(episode_length_buf, 1); W(rew_buf, 1); W(episode_sums, nr + 1); W(command_sums, nr + 5);
  soa(b ? b->episode_sums_eval : nullptr, K_WORD, nr + 1, true);
  W(friction_coeffs, 1); W(restitutions, 1); W(payloads, 1); W(com_displacements, 3); W(motor_strengths, 12); W(motor_offsets, 12);
  W(Kp_factors, 12); W(Kd_factors, 12); W(env_origins, 3); W(env_command_bins, 1); W(env_command_categories, 1); W(fault_flags, 1);
  soa(b ? b->measured_heights : nullptr, K_WORD, c->num_height_points > 0 ? c->num_height_points : 1, true);
  B8(reset_buf, 1); B8(time_out_buf, 1); B8(last_contacts, 4); B8(resample_flags, 1);
#undef W
#undef B8
  const int R = c->num_obs_history + 1;
  rowmajor(b ? b->obs_buf : nullptr, K_ROWS, c->num_obs);
  rowmajor(b ? b->obs_history : nullptr, K_HIST, R * c->num_obs);
  rowmajor(b ? b->privileged_obs_buf : nullptr, K_ROWS, c->num_privileged_obs > 0 ? c->num_privileged_obs : 1);
  const int64_t grid_words = (int64_t)c->num_categories * c->num_bins;
  run(b ? b->curriculum_weights : nullptr, grid_words, false);
  run(b ? b->curriculum_cdf : nullptr, grid_words, false);
  run(b ? b->curriculum_success : nullptr, grid_words * c->curriculum_update_interval, false);
  run(b ? b->episode_log : nullptr, nr + 2, false);
  run(b ? b->fault_counts : nullptr, GO1_FAULT_BITS, false);
  run(b ? b->contact_drop_counts : nullptr, GO1_CC_COUNT, true);

  Go1StateLayout& L = tb->L;
  header_of(c, L.header);
  L.word_rows = words; L.byte_rows = bytes; L.row_words = cols; L.global_words = flat;
  L.bytes_per_env = 4 * ((int64_t)words + cols) + bytes;
  P.tiles = tiles > 0x7fffffff ? -1 : (int32_t)tiles;
  P.grid = P.tiles < GO1STATE_MAX_BLOCKS ? P.tiles : GO1STATE_MAX_BLOCKS;
  P.N = c->num_envs; P.K = K; P.Ks = Ks;
  P.lag_n = c->lag_timesteps + 1; P.R = R; P.no = c->num_obs;
}

template <bool RESTORE>
int go(Table* tb, void* stream) {
  const Plan& P = tb->P;
  if (P.tiles <= 0 || P.nf <= 0) return -12;
  hipLaunchKernelGGL(state_kernel<RESTORE>, dim3((unsigned)P.grid), dim3(T), 0, (hipStream_t)stream, P);
  return hipGetLastError() == hipSuccess ? 0 : -20;
}

// what capture and restore ask alike, in the order of the codes; fills the table
int prepare(const Go1StateConfig* cfg, const Go1SimBuffers* buf, const int32_t* ids, int32_t K, int32_t lag_head, int32_t history_slot,
            const Go1StateSnapshot* snap, int Ks, bool restore, bool identity_rows, Table* tb) {
  if (!cfg || !buf || cfg->num_envs <= 0 || K <= 0) return -1;
  if (!snap || !snap->words || !snap->bytes || !snap->rows || !snap->skipped) return -2;
  const bool ok = in_range(cfg);
  fields(cfg, buf, K, Ks, false, tb);                 // (with a layout value out of range the table still tells which pointers are missing)
  if (tb->missing) return -3;
  if (!ids && K != cfg->num_envs) return -8;
  if (!ok || lag_head < 0 || lag_head > cfg->lag_timesteps || history_slot < 0 || history_slot > cfg->num_obs_history) return -12;
  if (restore && (Ks <= 0 || !same_header(cfg, snap->header) || (identity_rows && K > Ks))) return -12;
  tb->P.lag_head = lag_head; tb->P.hslot = history_slot; tb->P.ids = ids;
  tb->P.words = snap->words; tb->P.bytes = snap->bytes; tb->P.rows = snap->rows; tb->P.skipped = snap->skipped;
  return 0;
}

int prepare_global(const Go1StateConfig* cfg, const Go1SimBuffers* buf, const Go1StateSnapshot* snap, bool restore, Table* tb) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!snap || !snap->global) return -2;
  const bool ok = in_range(cfg);
  fields(cfg, buf, 1, 1, true, tb);
  if (tb->missing) return -3;
  if (!ok || (restore && !same_header(cfg, snap->header))) return -12;
  tb->P.global = snap->global;
  return 0;
}

}  // namespace

extern "C" int go1state_layout(const Go1StateConfig* cfg, Go1StateLayout* out) {
  if (!cfg || !out) return -1;
  if (!in_range(cfg)) return -12;
  Table tb;
  fields(cfg, nullptr, 1, 1, false, &tb);
  *out = tb.L;
  return 0;
}

extern "C" int go1state_capture(const Go1StateConfig* cfg, const Go1SimBuffers* buf, const int32_t* ids, int32_t K, int32_t lag_head,
                                int32_t history_slot, Go1StateSnapshot* snap, void* stream) {
  Table tb;
  if (int rc = prepare(cfg, buf, ids, K, lag_head, history_slot, snap, K, false, false, &tb)) return rc;
  header_of(cfg, snap->header);
  snap->num_rows = K;
  return go<false>(&tb, stream);
}

extern "C" int go1state_restore(const Go1StateConfig* cfg, const Go1SimBuffers* buf, const int32_t* dst_ids, const int32_t* src_rows, int32_t K,
                                int32_t lag_head, int32_t history_slot, const Go1StateSnapshot* snap, void* stream) {
  Table tb;
  if (int rc = prepare(cfg, buf, dst_ids, K, lag_head, history_slot, snap, snap ? snap->num_rows : 0, true, src_rows == nullptr, &tb)) return rc;
  tb.P.src_rows = src_rows;
  return go<true>(&tb, stream);
}

extern "C" int go1state_capture_global(const Go1StateConfig* cfg, const Go1SimBuffers* buf, Go1StateSnapshot* snap, void* stream) {
  Table tb;
  if (int rc = prepare_global(cfg, buf, snap, false, &tb)) return rc;
  header_of(cfg, snap->header);
  return go<false>(&tb, stream);
}

extern "C" int go1state_restore_global(const Go1StateConfig* cfg, const Go1SimBuffers* buf, const Go1StateSnapshot* snap, void* stream) {
  Table tb;
  if (int rc = prepare_global(cfg, buf, snap, true, &tb)) return rc;
  return go<true>(&tb, stream);
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1state_version(void) { return "go1state 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
