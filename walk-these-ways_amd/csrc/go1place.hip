// go1place.hip — foot placement and stride geometry of a policy rollout on the device (include/go1place.h), gfx950.
//
// place_accumulate_kernel: one thread per (foot, environment) in a one-dimensional launch whose blocks each belong to one foot, so every
// row access of a wavefront is one contiguous run of 64 words (the map word alone is scattered: its cell differs from lane to lane).
// Each word has one writer: nothing is shared between threads and nothing depends on scheduling.  The rows and the state words of an
// event (touchdown, liftoff) and the map word are read and written only on the steps of that event.
// place_reduce_kernel: one workgroup per (group, row of the result table), then one per (group, foot, sixteen cells of the map).
// Thread t combines environments t, t + 256, ... in ascending order in fp64, then a binary tree of fixed shape in LDS.
// tests/place_ref.py restates both in numpy from the header's text.
//
// The fold of a value into the six accumulators, the clear, the launch of one thread per (row, environment), the fixed-order reductions
// (a metric row, the sums of a group row, the sums per bin of sixteen cells) and the validation and launch helpers are go1_tables.h's,
// shared with the other table libraries.  The library's surface, symbols and stamp remain its own: the stamp covers that header.
#include "../../include/go1place.h"
#include "go1_tables.h"

namespace {

constexpr int NM = GO1PLACE_NUM, FEET = GO1PLACE_NUM_FEET, SIDE = GO1PLACE_MAP_SIDE, CELLS = GO1PLACE_MAP_CELLS, QUARTERS = CELLS / BINS;
GO1_TABLES_MATCH(GO1PLACE);
static_assert(SIDE * SIDE == CELLS && QUARTERS * BINS == CELLS, "the reduction sums the map sixteen cells at a time");

using PlaceArgs = Args<Go1PlaceConfig, Go1PlaceBuffers>;

// (bx, by): the x and y of R v = v + w t + u x t, u = (0, 0, z), t = 2 (u x v), every product formed (see the header)
__device__ __forceinline__ void yaw_rotate(float z, float w, float vx, float vy, float vz, float* bx, float* by) {
  const float cx = 0.0f * vz - z * vy, cy = z * vx - 0.0f * vz, cz = 0.0f * vy - 0.0f * vx;
  const float tx = 2.0f * cx, ty = 2.0f * cy, tz = 2.0f * cz;
  const float dx = 0.0f * tz - z * ty, dy = z * tx - 0.0f * tz;
  *bx = vx + w * tx + dx;
  *by = vy + w * ty + dy;
}

// the map coordinate of p (metres from the nominal point), as a float: in [0, SIDE) inside the map
__device__ __forceinline__ float map_coord(float p, float cell) { return floorf((p + 4.0f * cell) / cell); }

}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) place_clear_kernel(const PlaceArgs A) {
  const int N = A.c.num_envs;
  int f, e;
  if (!row_thread(N, FEET, &f, &e)) return;                               // (block k is foot k / blocks_per_foot)
  const Go1PlaceBuffers& b = A.b;
  const size_t i = (size_t)f * N + e;
  clear_rows(b, f * NM, NM, N, e);
  for (int cell = 0; cell < CELLS; cell++) b.map[(size_t)(f * CELLS + cell) * N + e] = 0u;
  b.prev_contact[i] = 2; b.stance_open[i] = 0; b.stride_open[i] = 0;
  b.td_x[i] = 0.0f; b.last_x[i] = 0.0f; b.last_y[i] = 0.0f; b.td_world_x[i] = 0.0f; b.td_world_y[i] = 0.0f;
  b.touchdowns[i] = 0u; b.liftoffs[i] = 0u; b.strides[i] = 0u; b.map_outside[i] = 0u;
  if (f == 0) { b.steps[e] = 0u; b.resets[e] = 0u; }
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) place_accumulate_kernel(const PlaceArgs A) {
  const Go1PlaceConfig& c = A.c;
  const int N = c.num_envs;
  int f, e;
  if (!row_thread(N, FEET, &f, &e)) return;                               // (block k is foot k / blocks_per_foot)
  const Go1PlaceBuffers& b = A.b;
  const size_t i = (size_t)f * N + e;
  const bool reset = b.reset_buf[e] != 0;
  if (f == 0) {
    b.steps[e] += 1u;
    if (reset) b.resets[e] += 1u;
  }
  if (reset || b.episode_length_buf[e] <= c.warmup_steps) {                // nothing folded; no stance or stride spans this step
    b.prev_contact[i] = 2; b.stance_open[i] = 0; b.stride_open[i] = 0;
    return;
  }
  const Row row = {N, e};
  const float cmd_vx = row(b.commands, 0), cmd_vyc = row(b.commands, 1), cmd_yaw = row(b.commands, 2), cmd_freq = row(b.commands, 4);
  const float width = c.num_commands >= 13 ? row(b.commands, 12) : 0.3f;
  const float length = c.num_commands >= 14 ? row(b.commands, 13) : 0.45f;
  const float base_x = row(b.root_states, 0), base_y = row(b.root_states, 1), base_z = row(b.root_states, 2);
  const float qz = row(b.root_states, 5), qw = row(b.root_states, 6);
  const int p = f ^ 1;
  const float pos_x = row(b.foot_positions, 3 * f), pos_y = row(b.foot_positions, 3 * f + 1), pos_z = row(b.foot_positions, 3 * f + 2);
  const float fz = row(b.contact_forces, 12 * (f + 1) + 2);
  const float index = row(b.foot_indices, f);
  const int prev = (int)b.prev_contact[i];

  // ---- the Raibert block of go1eval_behaviour_accumulate, operation for operation
  const float yaw_norm = fmaxf(sqrtf(qz * qz + qw * qw), 1e-9f);
  const float yaw_z = -qz / yaw_norm, yaw_w = qw / yaw_norm;
  const float half_period = 0.5f / cmd_freq, cmd_vy = cmd_yaw * length / 2;
  float bx, by;
  yaw_rotate(yaw_z, yaw_w, pos_x - base_x, pos_y - base_y, pos_z - base_z, &bx, &by);
  const float xs = (f < 2 ? 1.0f : -1.0f) * length / 2, ys = (f % 2 == 0 ? 1.0f : -1.0f) * width / 2;
  const float phase = fabsf(1.0f - index * 2.0f) * 1.0f - 0.5f;
  const float xo = phase * cmd_vx * half_period;
  float yo = phase * cmd_vy * half_period;
  if (f >= 2) yo = -yo;
  const float ex = bx - (xs + xo), ey = by - (ys + yo);
  const float px = bx - xs, py = by - ys;
  const bool contact = fz > (float)GO1PLACE_CONTACT_FORCE;

  const int r = f * NM;
  fold(b, r + (contact ? GO1PLACE_STANCE_ERR_X : GO1PLACE_SWING_ERR_X), N, e, ex);
  fold(b, r + (contact ? GO1PLACE_STANCE_ERR_Y : GO1PLACE_SWING_ERR_Y), N, e, ey);

  if (contact && prev == 0) {                                              // touchdown
    fold(b, r + GO1PLACE_TOUCHDOWN_X, N, e, px);
    fold(b, r + GO1PLACE_TOUCHDOWN_Y, N, e, py);
    fold(b, r + GO1PLACE_TOUCHDOWN_ERR_X, N, e, ex);
    fold(b, r + GO1PLACE_TOUCHDOWN_ERR_Y, N, e, ey);
    float bx_p, by_p;
    yaw_rotate(yaw_z, yaw_w, row(b.foot_positions, 3 * p) - base_x, row(b.foot_positions, 3 * p + 1) - base_y,
               row(b.foot_positions, 3 * p + 2) - base_z, &bx_p, &by_p);
    fold(b, r + GO1PLACE_TRACK_WIDTH_ERR, N, e, fabsf(by - by_p) - width);
    const float u = map_coord(px, c.map_cell), v = map_coord(py, c.map_cell), side = (float)SIDE;
    if (u >= 0.0f && u < side && v >= 0.0f && v < side)                    // (as floats: a NaN fails, so the cell is in [0, CELLS))
      b.map[(size_t)(f * CELLS + SIDE * (int)v + (int)u) * N + e] += 1u;
    else
      b.map_outside[i] += 1u;
    if (b.stride_open[i] != 0) {
      const float dx = pos_x - b.td_world_x[i], dy = pos_y - b.td_world_y[i];
      const float stride = sqrtf(dx * dx + dy * dy);
      fold(b, r + GO1PLACE_STRIDE_LENGTH, N, e, stride);
      fold(b, r + GO1PLACE_STRIDE_LENGTH_ERR, N, e, stride - sqrtf(cmd_vx * cmd_vx + cmd_vyc * cmd_vyc) / cmd_freq);
      b.strides[i] += 1u;
    }
    b.td_x[i] = px; b.td_world_x[i] = pos_x; b.td_world_y[i] = pos_y;
    b.stance_open[i] = 1; b.stride_open[i] = 1;
    b.touchdowns[i] += 1u;
  }
  if (!contact && prev == 1) {                                             // liftoff
    if (b.stance_open[i] != 0) {
      const float last_x = b.last_x[i];
      fold(b, r + GO1PLACE_LIFTOFF_X, N, e, last_x);
      fold(b, r + GO1PLACE_LIFTOFF_Y, N, e, b.last_y[i]);
      fold(b, r + GO1PLACE_STANCE_SWEEP, N, e, b.td_x[i] - last_x);
      b.liftoffs[i] += 1u;
    }
    b.stance_open[i] = 0;
  }
  if (contact) { b.last_x[i] = px; b.last_y[i] = py; }
  b.prev_contact[i] = contact ? 1 : 0;
}

extern "C" __global__ void __launch_bounds__(RT) place_reduce_kernel(const PlaceArgs A) {
  __shared__ double lds[NF][RT];
  constexpr int rows = FEET * NM + 1;
  const int N = A.c.num_envs, G = A.c.num_groups;
  const int t = (int)threadIdx.x;
  const Go1PlaceBuffers& b = A.b;
  if ((int)blockIdx.x < G * rows) {
    const int g = (int)blockIdx.x / rows, m = (int)blockIdx.x % rows;
    double* out = b.results + ((size_t)g * rows + m) * NF;
    if (m != rows - 1) { reduce_metric_row(b, g, m, N, lds, out); return; }
    // the group's own row: a[0] envs, a[1] steps, a[2] resets, a[3] touchdowns, a[4] strides, a[5] touchdowns outside the map
    group_sums<6>(b.group, g, N, lds, [&b, N](int e, double* a) {
      a[0] += 1.0; a[1] += (double)b.steps[e]; a[2] += (double)b.resets[e];
      for (int f = 0; f < FEET; f++) {
        const size_t i = (size_t)f * N + e;
        a[3] += (double)b.touchdowns[i]; a[4] += (double)b.strides[i]; a[5] += (double)b.map_outside[i];
      }
    });
    if (t != 0) return;
    out[GO1PLACE_G_ENVS] = lds[0][0]; out[GO1PLACE_G_STEPS] = lds[1][0]; out[GO1PLACE_G_RESETS] = lds[2][0];
    out[GO1PLACE_G_TOUCHDOWNS] = lds[3][0]; out[GO1PLACE_G_STRIDES] = lds[4][0]; out[GO1PLACE_G_MAP_OUTSIDE] = lds[5][0];
    return;
  }
  // sixteen cells of the map of (group, foot): thread t owns cell 16 k + t % 16 and the environments t / 16, t / 16 + 16, ...
  const int k = (int)blockIdx.x - G * rows;
  const int g = k / (FEET * QUARTERS), first = (k % (FEET * QUARTERS)) * BINS;           // first: f * CELLS + 16 * quarter
  const uint32_t* words = b.map + (size_t)(first + t % BINS) * N;
  bin_sums<1>(b.group, g, N, lds, [words](int e, double* a) { a[0] += (double)words[e]; });
  if (t < BINS) b.map_results[(size_t)g * FEET * CELLS + first + t] = lds[0][t];
}

// ---- the entry points: validation in the order the header gives the codes, then one launch ---------------------------------------------
namespace {
// what every entry point asks first: -1, -2
int check(const Go1PlaceConfig* cfg, const Go1PlaceBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->prev_contact || !buf->stance_open || !buf->stride_open || !buf->td_x || !buf->last_x || !buf->last_y ||
      !buf->td_world_x || !buf->td_world_y || !buf->touchdowns || !buf->liftoffs || !buf->strides || !buf->map_outside || !buf->map ||
      !buf->steps || !buf->resets) return -2;
  return 0;
}
}  // namespace

extern "C" int go1place_clear(const Go1PlaceConfig* cfg, const Go1PlaceBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  return launch(place_clear_kernel, row_grid(FEET, cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1place_accumulate(const Go1PlaceConfig* cfg, const Go1PlaceBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->commands || !buf->root_states || !buf->foot_positions || !buf->contact_forces || !buf->foot_indices || !buf->reset_buf ||
      !buf->episode_length_buf) return -3;
  if (!positive(cfg->map_cell) || cfg->num_commands < 5) return -12;
  return launch(place_accumulate_kernel, row_grid(FEET, cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1place_reduce(const Go1PlaceConfig* cfg, const Go1PlaceBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf) || !buf->map_results) return -5;
  return launch(place_reduce_kernel, table_grid(cfg->num_groups, FEET * NM + 1 + FEET * QUARTERS), RT, stream, cfg, buf);
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1place_version(void) { return "go1place 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
