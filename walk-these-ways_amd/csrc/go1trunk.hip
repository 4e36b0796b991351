// go1trunk.hip — trunk motion, support margin and path drift of a policy rollout on the device (include/go1trunk.h), gfx950.
//
// trunk_accumulate_kernel: one thread per environment, lanes on consecutive environments, so every row access of a wavefront is one
// contiguous run of 64 words (the histogram word alone is scattered: its bin differs from lane to lane).  Each word has one writer: no
// atomics, no LDS, nothing depends on scheduling.  The rows of an event (the accelerations, the support rows, a segment's close) are
// read and written only on the steps that fold into them.  The four feet are walked in their cyclic order by an unrolled loop over
// registers: no array is indexed by a run-time value, so nothing lives in scratch.
// trunk_reduce_kernel: one workgroup per (group, row of the result table), then one per group for the tilt histogram.  Thread t
// combines environments t, t + 256, ... in ascending order in fp64, then a binary tree of fixed shape in LDS.
// tests/trunk_ref.py restates both in numpy from the header's text.
//
// The fold of a value into the six accumulators, the clear, the fixed-order reductions (a metric row, the sums of a group row, the sums
// per bin of the histogram) and the validation and launch helpers are go1_tables.h's, shared with the evaluation and foot libraries.
// The library's surface, symbols and stamp remain its own: the stamp covers that header.
#include "../../include/go1trunk.h"
#include "go1_tables.h"

namespace {

constexpr int NM = GO1TRUNK_NUM;
GO1_TABLES_MATCH(GO1TRUNK);
static_assert(GO1TRUNK_TILT_BINS == BINS, "trunk_reduce_kernel: the histogram's bins are bin_sums'");

using TrunkArgs = Args<Go1TrunkConfig, Go1TrunkBuffers>;

// the histogram bin of the finite tilt: clamped as a float, then converted (see the header)
__device__ __forceinline__ int tilt_bin(float tilt) {
  const float b = floorf(tilt * 32.0f), last = (float)(BINS - 1);
  return (int)(b > last ? last : (b > 0.0f ? b : 0.0f));
}

// the signed distance of the base (px, py) from the edge (ax, ay) -> (bx, by): positive to the left of it
__device__ __forceinline__ float edge_distance(float ax, float ay, float bx, float by, float px, float py) {
  const float ex = bx - ax, ey = by - ay;
  return (ex * (py - ay) - ey * (px - ax)) / sqrtf(ex * ex + ey * ey);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) trunk_clear_kernel(const TrunkArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)blockIdx.x * ACC_THREADS + (int)threadIdx.x;
  if (e >= N) return;
  const Go1TrunkBuffers& b = A.b;
  clear_rows(b, 0, NM, N, e);
  for (int bin = 0; bin < BINS; bin++) b.tilt_hist[(size_t)bin * N + e] = 0u;
  b.prev_valid[e] = 0; b.seg_valid[e] = 0; b.seg_steps[e] = 0;
  for (int k = 0; k < 3; k++) { b.prev_lin_vel[(size_t)k * N + e] = 0.0f; b.prev_ang_vel[(size_t)k * N + e] = 0.0f; }
  for (int k = 0; k < 4; k++) b.seg_anchor[(size_t)k * N + e] = 0.0f;
  for (int k = 0; k < 2; k++) b.seg_command[(size_t)k * N + e] = 0.0f;
  b.segments_dropped[e] = 0u; b.steps[e] = 0u; b.resets[e] = 0u;
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) trunk_accumulate_kernel(const TrunkArgs A) {
  const Go1TrunkConfig& c = A.c;
  const int N = c.num_envs;
  const int e = (int)blockIdx.x * ACC_THREADS + (int)threadIdx.x;
  if (e >= N) return;
  const Go1TrunkBuffers& b = A.b;
  const size_t n = (size_t)N;
  const bool reset = b.reset_buf[e] != 0;
  b.steps[e] += 1u;
  if (reset) b.resets[e] += 1u;
  if (reset || b.episode_length_buf[e] <= c.warmup_steps) {                // nothing folded; no previous velocity, no open segment
    b.prev_valid[e] = 0; b.seg_valid[e] = 0;
    return;
  }
  const float* rs = b.root_states + e;
  const float px = rs[0], py = rs[n];
  const float qx = rs[3 * n], qy = rs[4 * n], qz = rs[5 * n], qw = rs[6 * n];
  const float vx = rs[7 * n], vy = rs[8 * n], vz = rs[9 * n];
  const float wx = rs[10 * n], wy = rs[11 * n], wz = rs[12 * n];
  const float bvz = b.base_lin_vel[2 * n + e];
  const float bwx = b.base_ang_vel[e], bwy = b.base_ang_vel[n + e];
  const float gx = b.projected_gravity[e], gy = b.projected_gravity[n + e];
  const float dt = c.dt;

  // ---- the trunk's attitude and rates
  const float tilt = sqrtf(gx * gx + gy * gy);
  fold(b, GO1TRUNK_ROLL_SIN, N, e, gy);
  fold(b, GO1TRUNK_PITCH_SIN, N, e, gx);
  fold(b, GO1TRUNK_TILT, N, e, tilt);
  fold(b, GO1TRUNK_TILT_EXCEEDED, N, e, tilt > c.tilt_limit ? 1.0f : 0.0f);
  fold(b, GO1TRUNK_ROLL_RATE, N, e, bwx);
  fold(b, GO1TRUNK_PITCH_RATE, N, e, bwy);
  fold(b, GO1TRUNK_VERTICAL_VEL, N, e, bvz);

  // ---- the accelerations: differences against the last folded step's velocities
  if (b.prev_valid[e] != 0) {
    const float ax = (vx - b.prev_lin_vel[e]) / dt, ay = (vy - b.prev_lin_vel[n + e]) / dt, az = (vz - b.prev_lin_vel[2 * n + e]) / dt;
    const float ux = (wx - b.prev_ang_vel[e]) / dt, uy = (wy - b.prev_ang_vel[n + e]) / dt, uz = (wz - b.prev_ang_vel[2 * n + e]) / dt;
    fold(b, GO1TRUNK_ACCEL_HORIZONTAL, N, e, sqrtf(ax * ax + ay * ay));
    fold(b, GO1TRUNK_ACCEL_VERTICAL, N, e, az);
    fold(b, GO1TRUNK_ANG_ACCEL, N, e, sqrtf((ux * ux + uy * uy) + uz * uz));
  }

  // ---- the support: the feet in contact, walked in the cyclic order FL, RL, RR, FR
  constexpr int ORDER[4] = {0, 2, 3, 1};
  int n_c = 0;
  float first_x = 0.0f, first_y = 0.0f, last_x = 0.0f, last_y = 0.0f;      // the first and the latest foot in contact
  float first_d = 0.0f, margin = 0.0f;                                     // the first edge's d; the smallest d so far
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int f = ORDER[k];
    const float fz = b.contact_forces[(size_t)(12 * (f + 1) + 2) * n + e];
    if (!(fz > (float)GO1TRUNK_CONTACT_FORCE)) continue;
    const float x = b.foot_positions[(size_t)(3 * f) * n + e], y = b.foot_positions[(size_t)(3 * f + 1) * n + e];
    if (n_c == 0) {
      first_x = x; first_y = y;
    } else {
      const float d = edge_distance(last_x, last_y, x, y, px, py);
      if (n_c == 1) { first_d = d; margin = d; }
      else if (d < margin || d != d) margin = d;
    }
    last_x = x; last_y = y;
    n_c += 1;
  }
  fold(b, GO1TRUNK_SUPPORT_FEET, N, e, (float)n_c);
  if (n_c >= 3) {
    const float d = edge_distance(last_x, last_y, first_x, first_y, px, py);    // wrapping round
    if (d < margin || d != d) margin = d;
    fold(b, GO1TRUNK_SUPPORT_MARGIN, N, e, margin);
    fold(b, GO1TRUNK_MARGIN_NEGATIVE, N, e, margin < 0.0f ? 1.0f : 0.0f);
  } else if (n_c == 2) {
    fold(b, GO1TRUNK_SUPPORT_LINE_DIST, N, e, fabsf(first_d));
  }

  // ---- the tilt histogram
  if (isfinite(tilt)) b.tilt_hist[(size_t)tilt_bin(tilt) * n + e] += 1u;   // the bin is clamped: in [0, BINS)

  b.prev_lin_vel[e] = vx; b.prev_lin_vel[n + e] = vy; b.prev_lin_vel[2 * n + e] = vz;
  b.prev_ang_vel[e] = wx; b.prev_ang_vel[n + e] = wy; b.prev_ang_vel[2 * n + e] = wz;
  b.prev_valid[e] = 1;

  // ---- the segment
  const float h0x = 1.0f - 2.0f * (qy * qy + qz * qz), h0y = 2.0f * (qx * qy + qw * qz);
  const float hn = sqrtf(h0x * h0x + h0y * h0y);
  const float hx = h0x / hn, hy = h0y / hn;
  const bool heading_ok = isfinite(hn) && hn > 0.0f && isfinite(px) && isfinite(py);
  bool anchor = false;
  if (b.seg_valid[e] == 0) {
    if (heading_ok) { anchor = true; b.seg_valid[e] = 1; }
  } else {
    const float cw = b.commands[2 * n + e];
    if (!(cw == 0.0f) || !heading_ok) {
      b.seg_valid[e] = 0;
      b.segments_dropped[e] += 1u;
    } else {
      const float sx = b.seg_command[e] + b.commands[e] * dt, sy = b.seg_command[n + e] + b.commands[n + e] * dt;
      const int steps = b.seg_steps[e] + 1;
      if (steps == c.segment_steps) {
        const float x0 = b.seg_anchor[e], y0 = b.seg_anchor[n + e], hx0 = b.seg_anchor[2 * n + e], hy0 = b.seg_anchor[3 * n + e];
        const float dx = px - x0, dy = py - y0;
        const float along = dx * hx0 + dy * hy0, lateral = dy * hx0 - dx * hy0;
        fold(b, GO1TRUNK_LATERAL_DRIFT, N, e, lateral - sy);
        fold(b, GO1TRUNK_HEADING_DRIFT, N, e, hx0 * hy - hy0 * hx);
        fold(b, GO1TRUNK_PROGRESS_ERR, N, e, along - sx);
        anchor = true;
      } else {
        b.seg_command[e] = sx; b.seg_command[n + e] = sy; b.seg_steps[e] = steps;
      }
    }
  }
  if (anchor) {                                                            // a segment begins at this step's pose
    b.seg_anchor[e] = px; b.seg_anchor[n + e] = py; b.seg_anchor[2 * n + e] = hx; b.seg_anchor[3 * n + e] = hy;
    b.seg_command[e] = 0.0f; b.seg_command[n + e] = 0.0f; b.seg_steps[e] = 0;
  }
}

extern "C" __global__ void __launch_bounds__(RT) trunk_reduce_kernel(const TrunkArgs A) {
  __shared__ double lds[NF][RT];
  constexpr int rows = NM + 1;
  const int N = A.c.num_envs, G = A.c.num_groups;
  const int t = (int)threadIdx.x;
  const Go1TrunkBuffers& b = A.b;
  if ((int)blockIdx.x < G * rows) {
    const int g = (int)blockIdx.x / rows, m = (int)blockIdx.x % rows;
    double* out = b.results + ((size_t)g * rows + m) * NF;
    if (m != rows - 1) { reduce_metric_row(b, g, m, N, lds, out); return; }
    // the group's own row: a[0] envs, a[1] steps, a[2] resets, a[3] segments dropped
    group_sums<4>(b.group, g, N, lds, [&b](int e, double* a) {
      a[0] += 1.0; a[1] += (double)b.steps[e]; a[2] += (double)b.resets[e]; a[3] += (double)b.segments_dropped[e];
    });
    if (t != 0) return;
    out[GO1TRUNK_G_ENVS] = lds[0][0]; out[GO1TRUNK_G_STEPS] = lds[1][0]; out[GO1TRUNK_G_RESETS] = lds[2][0];
    out[GO1TRUNK_G_SEGMENTS_DROPPED] = lds[3][0]; out[4] = 0.0; out[5] = 0.0;
    return;
  }
  // the tilt histogram of a group: thread t owns bin t % 16 and the environments t / 16, t / 16 + 16, ...
  const int g = (int)blockIdx.x - G * rows;
  const size_t w = (size_t)(t % BINS) * N;
  bin_sums<1>(b.group, g, N, lds, [&b, w](int e, double* a) { a[0] += (double)b.tilt_hist[w + e]; });
  if (t < BINS) b.hist_results[(size_t)g * BINS + t] = lds[0][t];
}

// ---- the entry points: validation in the order the header gives the codes, then one launch ---------------------------------------------
namespace {
// what every entry point asks first: -1, -2
int check(const Go1TrunkConfig* cfg, const Go1TrunkBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->prev_valid || !buf->prev_lin_vel || !buf->prev_ang_vel || !buf->seg_valid || !buf->seg_steps ||
      !buf->seg_anchor || !buf->seg_command || !buf->segments_dropped || !buf->steps || !buf->resets || !buf->tilt_hist) return -2;
  return 0;
}
}  // namespace

extern "C" int go1trunk_clear(const Go1TrunkConfig* cfg, const Go1TrunkBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  return launch(trunk_clear_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1trunk_accumulate(const Go1TrunkConfig* cfg, const Go1TrunkBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->root_states || !buf->base_lin_vel || !buf->base_ang_vel || !buf->projected_gravity || !buf->commands || !buf->contact_forces ||
      !buf->foot_positions || !buf->reset_buf || !buf->episode_length_buf) return -3;
  if (!(finite(cfg->dt) && cfg->dt > 0.0f && finite(cfg->tilt_limit) && cfg->tilt_limit >= 0.0f && cfg->segment_steps > 0)) return -12;
  return launch(trunk_accumulate_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1trunk_reduce(const Go1TrunkConfig* cfg, const Go1TrunkBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf) || !buf->hist_results) return -5;
  return launch(trunk_reduce_kernel, table_grid(cfg->num_groups, NM + 1 + 1), RT, stream, cfg, buf);
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1trunk_version(void) { return "go1trunk 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
