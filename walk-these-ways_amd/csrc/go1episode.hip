// go1episode.hip — whole episodes of a policy rollout on the device (include/go1episode.h), gfx950: returns, lengths, distances, the
// tracking error over an episode, and the length histograms of the episodes that fell, timed out and are still open.
//
// episode_accumulate_kernel: one thread per environment, lanes on consecutive environments, so every row access of a wavefront is one
// contiguous run of 64 words (the histogram words alone are scattered: their bin differs from lane to lane).  Each word has one writer:
// no atomics, no LDS, nothing depends on scheduling.  The state of the open episode is read and written on every step; the rows of an
// episode's close, the first position and the histograms only on the steps that close or open one.
// episode_reduce_kernel: one workgroup per (group, row of the result table), then one per (group, histogram).  Thread t combines
// environments t, t + 256, ... in ascending order in fp64, then a binary tree of fixed shape in LDS.
// tests/episode_ref.py restates both in numpy from the header's text.
//
// The fold of a value into the six accumulators, the clear, the fixed-order reductions (a metric row, the sums of a group row, the sums
// per bin of a histogram) and the validation and launch helpers are go1_tables.h's, shared with the other table libraries.  The
// library's surface, symbols and stamp remain its own: the stamp covers that header.
#include "../../include/go1episode.h"
#include "go1_tables.h"

namespace {

constexpr int NM = GO1EPISODE_NUM, HISTS = GO1EPISODE_NUM_HISTS;
GO1_TABLES_MATCH(GO1EPISODE);
static_assert(GO1EPISODE_BINS == BINS, "episode_reduce_kernel: the histograms' bins are bin_sums'");
static_assert(GO1EPISODE_PATH_LENGTH == NM - 1 && NM == 11, "episode_accumulate_kernel: eleven rows");

using EpisodeArgs = Args<Go1EpisodeConfig, Go1EpisodeBuffers>;

// the length bin of an episode of age + 1 steps: the sixteenth is open-ended (age >= 0, bin_steps >= 1)
__device__ __forceinline__ int length_bin(int age, int bin_steps) {
  const int b = age / bin_steps;
  return b < BINS - 1 ? b : BINS - 1;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) episode_clear_kernel(const EpisodeArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)blockIdx.x * ACC_THREADS + (int)threadIdx.x;
  if (e >= N) return;
  const Go1EpisodeBuffers& b = A.b;
  const size_t n = (size_t)N;
  clear_rows(b, 0, NM, N, e);
  for (int bin = 0; bin < BINS; bin++) { b.fall_hist[bin * n + e] = 0u; b.timeout_hist[bin * n + e] = 0u; }
  b.age[e] = -1; b.whole[e] = 0;
  b.ret[e] = 0.0f; b.disc_ret[e] = 0.0f; b.disc_w[e] = 1.0f;
  b.first_pos[e] = 0.0f; b.first_pos[n + e] = 0.0f; b.prev_pos[e] = 0.0f; b.prev_pos[n + e] = 0.0f;
  b.path[e] = 0.0f; b.lin_err[e] = 0.0f; b.yaw_err[e] = 0.0f; b.track_steps[e] = 0;
  b.steps[e] = 0u; b.closed[e] = 0u; b.fell[e] = 0u; b.timed_out[e] = 0u; b.cut[e] = 0u; b.unseen[e] = 0u;
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) episode_accumulate_kernel(const EpisodeArgs A) {
  const Go1EpisodeConfig& c = A.c;
  const int N = c.num_envs;
  const int e = (int)blockIdx.x * ACC_THREADS + (int)threadIdx.x;
  if (e >= N) return;
  const Go1EpisodeBuffers& b = A.b;
  const size_t n = (size_t)N;
  const float r = b.rew_buf[e];
  b.steps[e] += 1u;
  fold(b, GO1EPISODE_STEP_REWARD, N, e, r);
  const int age = b.age[e];
  const float x = b.root_states[e], y = b.root_states[n + e];

  if (b.reset_buf[e] != 0) {
    if (age >= 0) {                                                        // (a) an episode of L = age + 1 steps closes
      const float L = (float)(age + 1);
      const bool timed = b.time_out_buf[e] != 0;
      const float ret = b.ret[e] + r;
      const float disc = b.disc_ret[e] + b.disc_w[e] * r;
      fold(b, GO1EPISODE_LENGTH, N, e, L);
      fold(b, GO1EPISODE_FELL, N, e, timed ? 0.0f : 1.0f);
      if (!timed) fold(b, GO1EPISODE_LENGTH_FELL, N, e, L);
      fold(b, GO1EPISODE_RETURN, N, e, ret);
      fold(b, GO1EPISODE_REWARD_RATE, N, e, ret / L);
      const int tracked = b.track_steps[e];
      if (tracked > 0) {
        fold(b, GO1EPISODE_LIN_VEL_ERR, N, e, b.lin_err[e] / (float)tracked);
        fold(b, GO1EPISODE_YAW_VEL_ERR, N, e, b.yaw_err[e] / (float)tracked);
      }
      if (b.whole[e] != 0) {
        const float dx = b.prev_pos[e] - b.first_pos[e], dy = b.prev_pos[n + e] - b.first_pos[n + e];
        fold(b, GO1EPISODE_DISCOUNTED_RETURN, N, e, disc);
        fold(b, GO1EPISODE_DISPLACEMENT, N, e, sqrtf(dx * dx + dy * dy));
        fold(b, GO1EPISODE_PATH_LENGTH, N, e, b.path[e]);
      }
      const size_t word = (size_t)length_bin(age, c.bin_steps) * n + e;      // the bin is clamped: in [0, BINS)
      b.closed[e] += 1u;
      if (timed) { b.timeout_hist[word] += 1u; b.timed_out[e] += 1u; }
      else { b.fall_hist[word] += 1u; b.fell[e] += 1u; }
    } else {                                                               // (b) nothing of the episode that ended was seen
      b.unseen[e] += 1u;
    }
    // (c) a whole episode opens at the respawn pose
    b.age[e] = 0; b.whole[e] = 1;
    b.ret[e] = 0.0f; b.disc_ret[e] = 0.0f; b.disc_w[e] = 1.0f;
    b.first_pos[e] = x; b.first_pos[n + e] = y; b.prev_pos[e] = x; b.prev_pos[n + e] = y;
    b.path[e] = 0.0f; b.lin_err[e] = 0.0f; b.yaw_err[e] = 0.0f; b.track_steps[e] = 0;
    return;
  }

  const int elb = b.episode_length_buf[e];
  bool first = age < 0;
  if (!first && elb != age + 1) { b.cut[e] += 1u; first = true; }          // cut from outside: dropped, and seen anew
  float lin, yaw;
  int tracked;
  b.age[e] = elb;
  if (first) {
    b.whole[e] = elb == 1 ? 1 : 0;
    b.ret[e] = b.episode_sums[(size_t)c.return_row * n + e];
    b.disc_ret[e] = r; b.disc_w[e] = c.gamma;
    b.first_pos[e] = x; b.first_pos[n + e] = y;
    b.path[e] = 0.0f;
    lin = 0.0f; yaw = 0.0f; tracked = 0;
  } else {
    const float w = b.disc_w[e];
    b.ret[e] = b.ret[e] + r;
    b.disc_ret[e] = b.disc_ret[e] + w * r;
    b.disc_w[e] = w * c.gamma;
    const float dx = x - b.prev_pos[e], dy = y - b.prev_pos[n + e];
    b.path[e] = b.path[e] + sqrtf(dx * dx + dy * dy);
    lin = b.lin_err[e]; yaw = b.yaw_err[e]; tracked = b.track_steps[e];
  }
  b.prev_pos[e] = x; b.prev_pos[n + e] = y;
  if (elb > c.warmup_steps) {
    const float ex = b.base_lin_vel[e] - b.commands[e], ey = b.base_lin_vel[n + e] - b.commands[n + e];
    lin = lin + sqrtf(ex * ex + ey * ey);
    yaw = yaw + fabsf(b.base_ang_vel[2 * n + e] - b.commands[2 * n + e]);
    tracked += 1;
  }
  b.lin_err[e] = lin; b.yaw_err[e] = yaw; b.track_steps[e] = tracked;
}

extern "C" __global__ void __launch_bounds__(RT) episode_reduce_kernel(const EpisodeArgs A) {
  __shared__ double lds[NF][RT];
  constexpr int rows = NM + 2;
  const int N = A.c.num_envs, G = A.c.num_groups;
  const int t = (int)threadIdx.x;
  const Go1EpisodeBuffers& b = A.b;
  if ((int)blockIdx.x < G * rows) {
    const int g = (int)blockIdx.x / rows, m = (int)blockIdx.x % rows;
    double* out = b.results + ((size_t)g * rows + m) * NF;
    if (m < NM) { reduce_metric_row(b, g, m, N, lds, out); return; }
    if (m == NM) {
      // the group's first own row: a[0] envs, a[1] steps, a[2] closed, a[3] fell, a[4] timed out, a[5] open
      group_sums<6>(b.group, g, N, lds, [&b](int e, double* a) {
        a[0] += 1.0; a[1] += (double)b.steps[e]; a[2] += (double)b.closed[e]; a[3] += (double)b.fell[e]; a[4] += (double)b.timed_out[e];
        a[5] += b.age[e] >= 0 ? 1.0 : 0.0;
      });
      if (t != 0) return;
      out[GO1EPISODE_G_ENVS] = lds[0][0]; out[GO1EPISODE_G_STEPS] = lds[1][0]; out[GO1EPISODE_G_CLOSED] = lds[2][0];
      out[GO1EPISODE_G_FELL] = lds[3][0]; out[GO1EPISODE_G_TIMED_OUT] = lds[4][0]; out[GO1EPISODE_G_OPEN] = lds[5][0];
      return;
    }
    // the second: a[0] cut, a[1] unseen, a[2] the steps of the open episodes
    group_sums<3>(b.group, g, N, lds, [&b](int e, double* a) {
      a[0] += (double)b.cut[e]; a[1] += (double)b.unseen[e]; a[2] += b.age[e] >= 0 ? (double)b.age[e] : 0.0;
    });
    if (t != 0) return;
    out[GO1EPISODE_H_CUT] = lds[0][0]; out[GO1EPISODE_H_UNSEEN] = lds[1][0]; out[GO1EPISODE_H_OPEN_STEPS] = lds[2][0];
    out[3] = 0.0; out[4] = 0.0; out[5] = 0.0;
    return;
  }
  // histogram h of a group: thread t owns bin t % 16 and the environments t / 16, t / 16 + 16, ...
  const int k = (int)blockIdx.x - G * rows;
  const int g = k / HISTS, h = k % HISTS;
  const int bin = t % BINS;
  if (h < 2) {
    const uint32_t* hist = h == 0 ? b.fall_hist : b.timeout_hist;
    const size_t w = (size_t)bin * N;
    bin_sums<1>(b.group, g, N, lds, [hist, w](int e, double* a) { a[0] += (double)hist[w + e]; });
  } else {                                                                 // the open episodes by age bin: the censored observations
    const int bin_steps = A.c.bin_steps;
    bin_sums<1>(b.group, g, N, lds, [&b, bin, bin_steps](int e, double* a) {
      const int age = b.age[e];
      a[0] += (age >= 0 && length_bin(age, bin_steps) == bin) ? 1.0 : 0.0;
    });
  }
  if (t < BINS) b.hist_results[((size_t)g * HISTS + h) * BINS + t] = lds[0][t];
}

// ---- the entry points: validation in the order the header gives the codes, then one launch ---------------------------------------------
namespace {
// what every entry point asks first: -1, -2
int check(const Go1EpisodeConfig* cfg, const Go1EpisodeBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->age || !buf->whole || !buf->ret || !buf->disc_ret || !buf->disc_w || !buf->first_pos || !buf->prev_pos ||
      !buf->path || !buf->lin_err || !buf->yaw_err || !buf->track_steps || !buf->steps || !buf->closed || !buf->fell || !buf->timed_out ||
      !buf->cut || !buf->unseen || !buf->fall_hist || !buf->timeout_hist) return -2;
  return 0;
}
}  // namespace

extern "C" int go1episode_clear(const Go1EpisodeConfig* cfg, const Go1EpisodeBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  return launch(episode_clear_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1episode_accumulate(const Go1EpisodeConfig* cfg, const Go1EpisodeBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->rew_buf || !buf->reset_buf || !buf->time_out_buf || !buf->episode_length_buf || !buf->root_states || !buf->base_lin_vel ||
      !buf->base_ang_vel || !buf->commands || !buf->episode_sums) return -3;
  if (!positive(cfg->gamma) || cfg->gamma > 1.0f || cfg->bin_steps < 1 || cfg->return_row < 0) return -12;
  return launch(episode_accumulate_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1episode_reduce(const Go1EpisodeConfig* cfg, const Go1EpisodeBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf) || !buf->hist_results) return -5;
  if (cfg->bin_steps < 1) return -12;
  return launch(episode_reduce_kernel, table_grid(cfg->num_groups, NM + 2 + HISTS), RT, stream, cfg, buf);
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1episode_version(void) { return "go1episode 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
