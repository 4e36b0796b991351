// go1obs.hip — the distribution of the policy's observations on the device (include/go1obs.h), gfx950: per column of obs_buf (and of
// privileged_obs_buf) the moments, sixteen bins with two tails, the steps at the clip and the moments of the step-to-step change.
//
// obs_accumulate_kernel: one thread per (channel, environment) through row_thread; lanes on consecutive environments, so every state and
// accumulator access of a wavefront is one contiguous run of 64 words (the words of a bin alone are scattered: the bin differs from lane
// to lane).  The one read that is not: obs_buf is environment-major, a wavefront's 64 reads of one channel are num_obs words apart; the
// whole buffer (N * num_obs words, about 1 MB at 4096 environments) stays in L2 between the channels' blocks.  Each word has one writer
// and no thread reads what another writes: no atomics, no LDS, nothing depends on scheduling.
// obs_reduce_kernel: one workgroup per (group, row of the result table), then one per (group, channel) for the bins and one per
// (group, channel) for the three tails.
// tests/obs_ref.py restates all of it in numpy from the header's text.
//
// The fold of a value into the six accumulators, the clear of a row, the fixed-order reductions (a metric row, the sums of a group row,
// the sums per bin) and the validation and launch helpers are go1_tables.h's, shared with the other table libraries.  The library's
// surface, symbols and stamp remain its own: the stamp covers that header.
#include "../../include/go1obs.h"
#include "go1_tables.h"

namespace {

constexpr int MAXC = GO1OBS_MAX_CHANNELS, NT = GO1OBS_NUM_TAILS;
GO1_TABLES_MATCH(GO1OBS);
static_assert(GO1OBS_BINS == BINS, "obs_reduce_kernel: the histogram's bins are bin_sums'");
static_assert(NT == 3 && GO1OBS_T_AT_CLIP == NT - 1, "obs_reduce_kernel: three tails");
static_assert(sizeof(Go1ObsConfig) + sizeof(Go1ObsBuffers) < 4096, "the kernels take config and buffers by value: the argument has to stay under 4 KB");

using ObsArgs = Args<Go1ObsConfig, Go1ObsBuffers>;

// C of the header, for the kernels and the entry points alike (constexpr: callable on both sides); the entry points refuse a config for
// which this is outside [1, MAXC]
constexpr int channels(const Go1ObsConfig& c) { return c.num_obs + (c.privileged != 0 ? c.num_privileged_obs : 0); }

}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) obs_clear_kernel(const ObsArgs A) {
  const int N = A.c.num_envs, C = channels(A.c);
  int c, e;
  if (!row_thread(N, C, &c, &e)) return;
  const Go1ObsBuffers& b = A.b;
  const size_t n = (size_t)N, row = (size_t)c * n + e;
  clear_rows(b, c, 1, N, e);
  clear_rows(b, C + c, 1, N, e);
  b.prev[row] = 0.0f; b.age[row] = 0u; b.below[row] = 0u; b.above[row] = 0u; b.at_clip[row] = 0u;
  for (int k = 0; k < BINS; k++) b.hist[((size_t)c * BINS + k) * n + e] = 0u;
  if (c == 0) { b.launches[e] = 0u; b.resets[e] = 0u; }
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) obs_break_kernel(const ObsArgs A) {
  const int N = A.c.num_envs, C = channels(A.c);
  const int K = A.b.break_ids ? A.c.num_break : N;
  int c, k;
  if (!row_thread(K, C, &c, &k)) return;
  const int64_t id = A.b.break_ids ? A.b.break_ids[k] : (int64_t)k;
  if (id < 0 || id >= (int64_t)N) return;
  const size_t row = (size_t)c * N + (size_t)id;
  const uint32_t warm = A.c.warmup_steps > 0 ? (uint32_t)A.c.warmup_steps : 0u;
  if (A.b.age[row] > warm) A.b.age[row] = warm;
  if (c == 0) A.b.resets[id] += 1u;
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) obs_accumulate_kernel(const ObsArgs A) {
  const Go1ObsConfig& cf = A.c;
  const int N = cf.num_envs, C = channels(cf);
  int c, e;
  if (!row_thread(N, C, &c, &e)) return;
  const Go1ObsBuffers& b = A.b;
  const size_t n = (size_t)N, row = (size_t)c * n + e;
  const float v = c < cf.num_obs ? b.obs_buf[(size_t)e * cf.num_obs + c] : b.privileged_obs_buf[(size_t)e * cf.num_privileged_obs + (c - cf.num_obs)];
  if (c == 0) b.launches[e] += 1u;                                         // 0
  const uint32_t a = b.age[row] + 1u;                                      // 1
  b.age[row] = a;
  if ((int64_t)a <= (int64_t)cf.warmup_steps) { b.prev[row] = v; return; }
  fold(b, c, N, e, v);                                                     // 2
  if (isfinite(v)) {                                                       // 3
    const float t = (v - cf.lo[c]) * cf.scale[c];
    if (t < 0.0f) b.below[row] += 1u;
    else if (t < (float)BINS) b.hist[((size_t)c * BINS + (int)t) * n + e] += 1u;      // 0 <= t < 16: the bin is in [0, BINS)
    else b.above[row] += 1u;
  }
  if (fabsf(v) >= cf.clip) b.at_clip[row] += 1u;                           // 4
  if (b.reset_buf[e] != 0) {                                               // 5
    if (c == 0) b.resets[e] += 1u;
  } else if ((int64_t)a - 1 > (int64_t)cf.warmup_steps) {
    fold(b, C + c, N, e, fabsf(v - b.prev[row]));
  }
  b.prev[row] = v;                                                         // 6
}

extern "C" __global__ void __launch_bounds__(RT) obs_reduce_kernel(const ObsArgs A) {
  __shared__ double lds[NF][RT];
  const int N = A.c.num_envs, G = A.c.num_groups, C = channels(A.c);
  const int rows = 2 * C + 1;
  const int t = (int)threadIdx.x;
  const Go1ObsBuffers& b = A.b;
  const size_t n = (size_t)N;
  int k = (int)blockIdx.x;
  if (k < G * rows) {
    const int g = k / rows, m = k % rows;
    double* out = b.results + ((size_t)g * rows + m) * NF;
    if (m < 2 * C) { reduce_metric_row(b, g, m, N, lds, out); return; }
    // the group's own row, from channel 0: a[0] envs, a[1] launches, a[2] measured, a[3] resets
    group_sums<4>(b.group, g, N, lds, [&b](int e, double* a) {
      a[0] += 1.0; a[1] += (double)b.launches[e]; a[2] += (double)b.count[e] + (double)b.nonfinite[e]; a[3] += (double)b.resets[e];
    });
    if (t != 0) return;
    out[GO1OBS_G_ENVS] = lds[0][0]; out[GO1OBS_G_LAUNCHES] = lds[1][0]; out[GO1OBS_G_MEASURED] = lds[2][0]; out[GO1OBS_G_RESETS] = lds[3][0];
    out[4] = 0.0; out[5] = 0.0;
    return;
  }
  k -= G * rows;
  if (k < G * C) {
    // the bins of (group, channel): thread t owns bin t % 16 and the environments t / 16, t / 16 + 16, ...
    const int g = k / C, c = k % C;
    const size_t w = ((size_t)c * BINS + t % BINS) * n;
    bin_sums<1>(b.group, g, N, lds, [&b, w](int e, double* a) { a[0] += (double)b.hist[w + e]; });
    if (t < BINS) b.hist_results[((size_t)g * C + c) * BINS + t] = lds[0][t];
    return;
  }
  k -= G * C;
  // the three tails of (group, channel)
  const int g = k / C, c = k % C;
  const size_t w = (size_t)c * n;
  group_sums<NT>(b.group, g, N, lds, [&b, w](int e, double* a) {
    a[GO1OBS_T_BELOW] += (double)b.below[w + e]; a[GO1OBS_T_ABOVE] += (double)b.above[w + e]; a[GO1OBS_T_AT_CLIP] += (double)b.at_clip[w + e];
  });
  if (t != 0) return;
  double* out = b.tails + ((size_t)g * C + c) * NT;
  out[GO1OBS_T_BELOW] = lds[0][0]; out[GO1OBS_T_ABOVE] = lds[1][0]; out[GO1OBS_T_AT_CLIP] = lds[2][0];
}

// ---- the entry points: validation in the order the header gives the codes, then one launch ---------------------------------------------
namespace {
// what every entry point asks first: -1, -2
int check(const Go1ObsConfig* cfg, const Go1ObsBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->prev || !buf->age || !buf->hist || !buf->below || !buf->above || !buf->at_clip || !buf->launches || !buf->resets) return -2;
  return 0;
}

// -12: the channels, which size every launch
bool good_channels(const Go1ObsConfig* cfg) {
  if (cfg->num_obs < 1 || cfg->num_obs > MAXC) return false;
  if (cfg->privileged != 0 && (cfg->num_privileged_obs < 0 || cfg->num_privileged_obs > MAXC)) return false;
  return channels(*cfg) <= MAXC;
}

// -12: the bins of every channel, and the clip
bool good_bins(const Go1ObsConfig* cfg) {
  for (int c = 0; c < channels(*cfg); c++)
    if (!positive(cfg->scale[c]) || !finite(cfg->lo[c])) return false;
  return cfg->clip == cfg->clip;
}
}  // namespace

extern "C" int go1obs_clear(const Go1ObsConfig* cfg, const Go1ObsBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!good_channels(cfg)) return -12;
  return launch(obs_clear_kernel, row_grid(channels(*cfg), cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1obs_break(const Go1ObsConfig* cfg, const Go1ObsBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!good_channels(cfg) || (buf->break_ids && cfg->num_break < 0)) return -12;
  const int K = buf->break_ids ? cfg->num_break : cfg->num_envs;
  if (K == 0) return 0;
  return launch(obs_break_kernel, row_grid(channels(*cfg), K), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1obs_accumulate(const Go1ObsConfig* cfg, const Go1ObsBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->obs_buf || !buf->reset_buf || (cfg->privileged != 0 && !buf->privileged_obs_buf)) return -3;
  if (!good_channels(cfg) || !good_bins(cfg)) return -12;
  return launch(obs_accumulate_kernel, row_grid(channels(*cfg), cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1obs_reduce(const Go1ObsConfig* cfg, const Go1ObsBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf) || !buf->hist_results || !buf->tails) return -5;
  if (!good_channels(cfg)) return -12;
  const int C = channels(*cfg);
  return launch(obs_reduce_kernel, table_grid(cfg->num_groups, 2 * C + 1 + C + C), RT, stream, cfg, buf);
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1obs_version(void) { return "go1obs 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
