// go1gait.hip — inter-leg coordination and the realised gait of a policy rollout on the device (include/go1gait.h), gfx950.
//
// gait_accumulate_kernel: one thread per environment, lanes on consecutive environments, so every row access of a wavefront is one
// contiguous run of 64 words (the histogram words alone are scattered: their bin differs from lane to lane).  Each word has one writer:
// no atomics, no LDS, nothing depends on scheduling.  The rows of a stride's close and the per-foot stride words are read and written
// only on the steps that need them.  The four feet and the six pairs are walked by unrolled loops over registers: no array is indexed
// by a run-time value, so nothing lives in scratch.
// gait_reduce_kernel: one workgroup per (group, row of the result table), then one per (group, histogram).  Thread t combines
// environments t, t + 256, ... in ascending order in fp64, then a binary tree of fixed shape in LDS.
// tests/gait_ref.py restates both in numpy from the header's text.
//
// The fold of a value into the six accumulators, the clear, the fixed-order reductions (a metric row, the sums of a group row, the sums
// per bin of a histogram) and the validation and launch helpers are go1_tables.h's, shared with the evaluation, foot and trunk
// libraries.  The library's surface, symbols and stamp remain its own: the stamp covers that header.
#include "../../include/go1gait.h"
#include "go1_tables.h"

namespace {

constexpr int NM = GO1GAIT_NUM, HISTS = GO1GAIT_NUM_HISTS;
GO1_TABLES_MATCH(GO1GAIT);
static_assert(GO1GAIT_BINS == BINS, "gait_reduce_kernel: the histograms' bins are bin_sums'");
static_assert(GO1GAIT_SYNC_RL_RR == 5 && GO1GAIT_PHASE_ERR_FR == 6 && GO1GAIT_PHASE_ABS_ERR_FR == 9 && GO1GAIT_TOUCHDOWNS_FR == 12 && NM == 15,
              "gait_accumulate_kernel: six pairs, then three rows per kind for FR, RL, RR");

using GaitArgs = Args<Go1GaitConfig, Go1GaitBuffers>;

// the histogram bin of the touchdown phase p in [0, 1): centred on k / 16; 16 wraps to 0 as a float, then converted (see the header)
__device__ __forceinline__ int phase_bin(float p) {
  const float b = floorf(p * (float)BINS + 0.5f);
  return (int)((b >= 1.0f && b <= (float)(BINS - 1)) ? b : 0.0f);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) gait_clear_kernel(const GaitArgs A) {
  const int N = A.c.num_envs;
  const int e = (int)blockIdx.x * ACC_THREADS + (int)threadIdx.x;
  if (e >= N) return;
  const Go1GaitBuffers& b = A.b;
  clear_rows(b, 0, NM, N, e);
  for (int bin = 0; bin < BINS; bin++) b.support_hist[(size_t)bin * N + e] = 0u;
  for (int k = 0; k < 3 * BINS; k++) b.phase_hist[(size_t)k * N + e] = 0u;
  for (int f = 0; f < 4; f++) b.prev_contact[(size_t)f * N + e] = 2;
  b.ref_steps[e] = -1;
  for (int k = 0; k < 3; k++) { b.last_td[(size_t)k * N + e] = -1; b.td_count[(size_t)k * N + e] = 0; }
  b.steps[e] = 0u; b.resets[e] = 0u; b.strides[e] = 0u; b.strides_dropped[e] = 0u;
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) gait_accumulate_kernel(const GaitArgs A) {
  const Go1GaitConfig& c = A.c;
  const int N = c.num_envs;
  const int e = (int)blockIdx.x * ACC_THREADS + (int)threadIdx.x;
  if (e >= N) return;
  const Go1GaitBuffers& b = A.b;
  const size_t n = (size_t)N;
  const bool reset = b.reset_buf[e] != 0;
  b.steps[e] += 1u;
  if (reset) b.resets[e] += 1u;
  if (reset || b.episode_length_buf[e] <= c.warmup_steps) {                // nothing folded; every contact unknown, no open stride
#pragma unroll
    for (int f = 0; f < 4; f++) b.prev_contact[f * n + e] = 2;
    b.ref_steps[e] = -1;
    return;
  }

  // ---- contact, support pattern and touchdowns
  bool c0, c1, c2, c3, td0, td1, td2, td3;
  {
    bool ct[4], td[4];                                                     // (indexed by unrolled constants only: registers)
#pragma unroll
    for (int f = 0; f < 4; f++) {
      ct[f] = b.contact_forces[(size_t)(12 * (f + 1) + 2) * n + e] > (float)GO1GAIT_CONTACT_FORCE;
      td[f] = ct[f] && b.prev_contact[f * n + e] == 0;
    }
    c0 = ct[0]; c1 = ct[1]; c2 = ct[2]; c3 = ct[3];
    td0 = td[0]; td1 = td[1]; td2 = td[2]; td3 = td[3];
  }
  fold(b, GO1GAIT_SYNC_FL_FR, N, e, c0 == c1 ? 1.0f : 0.0f);
  fold(b, GO1GAIT_SYNC_FL_RL, N, e, c0 == c2 ? 1.0f : 0.0f);
  fold(b, GO1GAIT_SYNC_FL_RR, N, e, c0 == c3 ? 1.0f : 0.0f);
  fold(b, GO1GAIT_SYNC_FR_RL, N, e, c1 == c2 ? 1.0f : 0.0f);
  fold(b, GO1GAIT_SYNC_FR_RR, N, e, c1 == c3 ? 1.0f : 0.0f);
  fold(b, GO1GAIT_SYNC_RL_RR, N, e, c2 == c3 ? 1.0f : 0.0f);
  const int mask = (c0 ? 1 : 0) | (c1 ? 2 : 0) | (c2 ? 4 : 0) | (c3 ? 8 : 0);
  b.support_hist[(size_t)mask * n + e] += 1u;                              // mask is in [0, BINS)

  // ---- the reference stride
  int ref = b.ref_steps[e];
  if (ref >= 0) {
    ref += 1;
    if (ref > c.max_stride_steps) { ref = -1; b.strides_dropped[e] += 1u; }
  }
  bool fresh = false;                                                      // a stride opened on this step: the per-foot words are 0 / -1
  if (td0) {
    if (ref >= c.min_stride_steps) {                                       // (a) a stride of L = ref steps closes (min_stride_steps >= 1)
      const float L = (float)ref;
      const float fi0 = b.foot_indices[e];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int count = b.td_count[k * n + e];
        fold(b, GO1GAIT_TOUCHDOWNS_FR + k, N, e, (float)count);
        if (count >= 1) {
          const float p = (float)b.last_td[k * n + e] / L;
          const float d = fi0 - b.foot_indices[(k + 1) * n + e];
          const float cmd = d - floorf(d);
          float err = p - cmd;
          err = err - floorf(err + 0.5f);
          fold(b, GO1GAIT_PHASE_ERR_FR + k, N, e, err);
          fold(b, GO1GAIT_PHASE_ABS_ERR_FR + k, N, e, fabsf(err));
          b.phase_hist[(size_t)(k * BINS + phase_bin(p)) * n + e] += 1u;   // the bin is wrapped: in [0, BINS)
        }
      }
      b.strides[e] += 1u;
      fresh = true;
    } else if (ref < 0) {                                                  // (c) a stride opens
      fresh = true;
    }                                                                      // (b) chatter: the stride goes on
    if (fresh) ref = 0;
  }
  b.ref_steps[e] = ref;
  const bool tds[3] = {td1, td2, td3};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const bool hit = tds[k] && ref >= 0;
    if (fresh) {
      b.last_td[k * n + e] = hit ? 0 : -1;
      b.td_count[k * n + e] = hit ? 1 : 0;
    } else if (hit) {
      b.last_td[k * n + e] = ref;
      b.td_count[k * n + e] += 1;
    }
  }
  b.prev_contact[e] = c0 ? 1 : 0; b.prev_contact[n + e] = c1 ? 1 : 0; b.prev_contact[2 * n + e] = c2 ? 1 : 0; b.prev_contact[3 * n + e] = c3 ? 1 : 0;
}

extern "C" __global__ void __launch_bounds__(RT) gait_reduce_kernel(const GaitArgs A) {
  __shared__ double lds[NF][RT];
  constexpr int rows = NM + 1;
  const int N = A.c.num_envs, G = A.c.num_groups;
  const int t = (int)threadIdx.x;
  const Go1GaitBuffers& b = A.b;
  if ((int)blockIdx.x < G * rows) {
    const int g = (int)blockIdx.x / rows, m = (int)blockIdx.x % rows;
    double* out = b.results + ((size_t)g * rows + m) * NF;
    if (m != rows - 1) { reduce_metric_row(b, g, m, N, lds, out); return; }
    // the group's own row: a[0] envs, a[1] steps, a[2] resets, a[3] strides, a[4] strides dropped
    group_sums<5>(b.group, g, N, lds, [&b](int e, double* a) {
      a[0] += 1.0; a[1] += (double)b.steps[e]; a[2] += (double)b.resets[e]; a[3] += (double)b.strides[e]; a[4] += (double)b.strides_dropped[e];
    });
    if (t != 0) return;
    out[GO1GAIT_G_ENVS] = lds[0][0]; out[GO1GAIT_G_STEPS] = lds[1][0]; out[GO1GAIT_G_RESETS] = lds[2][0];
    out[GO1GAIT_G_STRIDES] = lds[3][0]; out[GO1GAIT_G_STRIDES_DROPPED] = lds[4][0]; out[5] = 0.0;
    return;
  }
  // histogram h of a group: thread t owns bin t % 16 and the environments t / 16, t / 16 + 16, ...
  const int k = (int)blockIdx.x - G * rows;
  const int g = k / HISTS, h = k % HISTS;
  const uint32_t* hist = h == 0 ? b.support_hist : b.phase_hist + (size_t)(h - 1) * BINS * N;
  const size_t w = (size_t)(t % BINS) * N;
  bin_sums<1>(b.group, g, N, lds, [hist, w](int e, double* a) { a[0] += (double)hist[w + e]; });
  if (t < BINS) b.hist_results[((size_t)g * HISTS + h) * BINS + t] = lds[0][t];
}

// ---- the entry points: validation in the order the header gives the codes, then one launch ---------------------------------------------
namespace {
// what every entry point asks first: -1, -2
int check(const Go1GaitConfig* cfg, const Go1GaitBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->prev_contact || !buf->ref_steps || !buf->last_td || !buf->td_count || !buf->steps || !buf->resets ||
      !buf->strides || !buf->strides_dropped || !buf->support_hist || !buf->phase_hist) return -2;
  return 0;
}
}  // namespace

extern "C" int go1gait_clear(const Go1GaitConfig* cfg, const Go1GaitBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  return launch(gait_clear_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1gait_accumulate(const Go1GaitConfig* cfg, const Go1GaitBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->contact_forces || !buf->foot_indices || !buf->reset_buf || !buf->episode_length_buf) return -3;
  if (cfg->min_stride_steps < 1 || cfg->max_stride_steps < cfg->min_stride_steps) return -12;
  return launch(gait_accumulate_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1gait_reduce(const Go1GaitConfig* cfg, const Go1GaitBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf) || !buf->hist_results) return -5;
  return launch(gait_reduce_kernel, table_grid(cfg->num_groups, NM + 1 + HISTS), RT, stream, cfg, buf);
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1gait_version(void) { return "go1gait 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
