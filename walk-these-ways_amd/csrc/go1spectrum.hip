// go1spectrum.hip — the power spectra of a policy rollout's actions, torques, joint speeds and trunk rates on the device
// (include/go1spectrum.h), gfx950.
//
// spectrum_record_kernel: one thread per (signal, environment), lanes on consecutive environments: one coalesced load and one coalesced
// store of the ring per wavefront; the signal is uniform over a block.  The s = 0 thread of an environment keeps the segment's state.
// spectrum_fold_kernel: the transform.  One wavefront per block, the lane is the environment and the signal is uniform over the block,
// so every ring load and every accumulator store is one contiguous run of 64 words.  The mean-removed samples y[t] and the densities
// P[k] of the block's 64 environments live in static LDS, each lane in its own column (so no barrier is needed: a lane reads only what
// it wrote).  The DFT is direct, k outer and t inner as the header writes it; the twiddle address [k][t] is the same in every lane and
// nothing is stored to global memory before the last twiddle is read, so the compiler reads the tables with scalar loads.  Every word
// has one writer: no atomics, nothing depends on scheduling.
// spectrum_reduce_kernel: one workgroup per (group, row of the result table), then one per (group, signal, bin or count).  Thread t
// combines environments t, t + 256, ... in ascending order in fp64, then a binary tree of fixed shape in LDS.
// tests/spectrum_ref.py restates all of them in numpy from the header's text.
//
// The fold of a value into the six accumulators, the clear, the fixed-order reductions and the validation and launch helpers are
// go1_tables.h's, shared with the evaluation, foot, trunk and gait libraries.  The library's surface, symbols and stamp remain its own:
// the stamp covers that header.
#include "../../include/go1spectrum.h"
#include "go1_tables.h"

namespace {

constexpr int S = GO1SPECTRUM_SIGNALS, NM = GO1SPECTRUM_NUM, ROWS = S * NM;
constexpr int WMIN = GO1SPECTRUM_MIN_SEGMENT, WMAX = GO1SPECTRUM_MAX_SEGMENT, FMAX = WMAX / 2 + 1, FT = GO1SPECTRUM_FOLD_THREADS;
GO1_TABLES_MATCH(GO1SPECTRUM);
static_assert(FT == 64, "spectrum_fold_kernel: one wavefront per block, so its LDS columns need no barrier");
static_assert((WMAX + FMAX) * FT * sizeof(float) <= 65536, "spectrum_fold_kernel: y and P in static LDS");
static_assert(GO1SPECTRUM_POWER == 0 && GO1SPECTRUM_PEAK_FREQ == 1 && GO1SPECTRUM_PEAK_SHARE == 2 && GO1SPECTRUM_HIGH_SHARE == 3 &&
              GO1SPECTRUM_CENTROID == 4 && NM == 5, "spectrum_fold_kernel: five rows per signal");

using SpectrumArgs = Args<Go1SpectrumConfig, Go1SpectrumBuffers>;
struct RecordArgs {
  Go1SpectrumConfig c;
  Go1SpectrumBuffers b;
  int slot;
};

}  // namespace

extern "C" __global__ void __launch_bounds__(ACC_THREADS) spectrum_clear_kernel(const SpectrumArgs A) {
  const int N = A.c.num_envs, F = A.c.segment_steps / 2 + 1;
  const int e = (int)blockIdx.x * ACC_THREADS + (int)threadIdx.x;
  if (e >= N) return;
  const Go1SpectrumBuffers& b = A.b;
  clear_rows(b, 0, ROWS, N, e);
  for (int k = 0; k < S * F; k++) b.psd_sum[(size_t)k * N + e] = 0.0;
  for (int s = 0; s < S; s++) b.psd_segments[(size_t)s * N + e] = 0u;
  b.valid[e] = 0;
  b.steps[e] = 0u; b.resets[e] = 0u; b.segments[e] = 0u; b.segments_dropped[e] = 0u;
}

extern "C" __global__ void __launch_bounds__(ACC_THREADS) spectrum_record_kernel(const RecordArgs A) {
  const Go1SpectrumConfig& c = A.c;
  const Go1SpectrumBuffers& b = A.b;
  const int N = c.num_envs;
  int s, e;
  if (!row_thread(N, S, &s, &e)) return;
  const size_t n = (size_t)N;
  const float* src = s < 12 ? b.actions + s * n : s < 24 ? b.torques + (s - 12) * n : s < 36 ? b.dof_vel + (s - 24) * n
                   : s < 39 ? b.base_ang_vel + (s - 36) * n : b.base_lin_vel + 2 * n;
  b.ring[((size_t)A.slot * S + s) * n + e] = src[e];
  if (s != 0) return;
  const bool reset = b.reset_buf[e] != 0;
  b.steps[e] += 1u;
  if (reset) b.resets[e] += 1u;
  const bool live = !reset && b.episode_length_buf[e] > c.warmup_steps;
  b.valid[e] = (uint8_t)((A.slot == 0 ? true : b.valid[e] != 0) && live ? 1 : 0);
}

extern "C" __global__ void __launch_bounds__(FT) spectrum_fold_kernel(const SpectrumArgs A) {
  __shared__ float y[WMAX][FT];                                              // the segment's samples, then mean-removed: a column per lane
  __shared__ float P[FMAX][FT];                                              // the densities
  const Go1SpectrumConfig& c = A.c;
  const Go1SpectrumBuffers& b = A.b;
  const int N = c.num_envs, W = c.segment_steps, F = W / 2 + 1;
  const int per_row = (N + FT - 1) / FT;
  const int s = (int)blockIdx.x / per_row, lane = (int)threadIdx.x;
  const int e = ((int)blockIdx.x % per_row) * FT + lane;
  if (s >= S || e >= N) return;
  const size_t n = (size_t)N;
  if (b.valid[e] == 0) {
    if (s == 0) b.segments_dropped[e] += 1u;
    return;
  }

  // ---- 1. the mean, in ascending t, and the mean-removed samples
  const float* x = b.ring + s * n + e;
  float sum = 0.0f;
  for (int t = 0; t < W; t++) {
    const float v = x[(size_t)t * S * n];
    y[t][lane] = v;
    sum = sum + v;
  }
  const float mean = sum / (float)W;
  for (int t = 0; t < W; t++) y[t][lane] = y[t][lane] - mean;

  // ---- 2. the direct DFT, k outer and t inner; the twiddle address is wave-uniform
  for (int k = 0; k < F; k++) {
    const float* cr = b.tw_re + (size_t)k * W;
    const float* ci = b.tw_im + (size_t)k * W;
    float re = 0.0f, im = 0.0f;
    for (int t = 0; t < W; t++) {
      const float v = y[t][lane];
      re = re + v * cr[t];
      im = im + v * ci[t];
    }
    P[k][lane] = (re * re + im * im) * b.scale[k];
  }

  // ---- 3. the total and the peak: the smallest k >= 1 with the largest P; a NaN never wins
  float total = 0.0f;
  for (int k = 1; k < F; k++) total = total + P[k][lane];
  int kp = 1;
  float best = P[1][lane];
  for (int k = 2; k < F; k++) {
    const float p = P[k][lane];
    if (p > best) { kp = k; best = p; }
  }

  // ---- 4. the five rows
  const bool finite_total = isfinite(total);
  float peak_freq = NAN, peak_share = NAN, high_share = NAN, centroid = NAN;
  if (finite_total && total > 0.0f) {
    peak_freq = b.freq[kp];
    peak_share = best / total;
    float high = 0.0f, cen = 0.0f;
    for (int k = c.high_bin; k < F; k++) high = high + P[k][lane];
    high_share = high / total;
    for (int k = 1; k < F; k++) cen = cen + b.freq[k] * P[k][lane];
    centroid = cen / total;
  }
  const int row = s * NM;
  fold(b, row + GO1SPECTRUM_POWER, N, e, total * c.bin_width);
  fold(b, row + GO1SPECTRUM_PEAK_FREQ, N, e, peak_freq);
  fold(b, row + GO1SPECTRUM_PEAK_SHARE, N, e, peak_share);
  fold(b, row + GO1SPECTRUM_HIGH_SHARE, N, e, high_share);
  fold(b, row + GO1SPECTRUM_CENTROID, N, e, centroid);

  // ---- 5. the density sum
  if (finite_total) {
    double* psd = b.psd_sum + (size_t)s * F * n + e;
    for (int k = 0; k < F; k++) psd[(size_t)k * n] += (double)P[k][lane];
    b.psd_segments[s * n + e] += 1u;
  }
  if (s == 0) b.segments[e] += 1u;
}

extern "C" __global__ void __launch_bounds__(RT) spectrum_reduce_kernel(const SpectrumArgs A) {
  __shared__ double lds[NF][RT];
  constexpr int rows = ROWS + 1;
  const int N = A.c.num_envs, G = A.c.num_groups, F = A.c.segment_steps / 2 + 1;
  const int t = (int)threadIdx.x;
  const Go1SpectrumBuffers& b = A.b;
  if ((int)blockIdx.x < G * rows) {
    const int g = (int)blockIdx.x / rows, m = (int)blockIdx.x % rows;
    double* out = b.results + ((size_t)g * rows + m) * NF;
    if (m != rows - 1) { reduce_metric_row(b, g, m, N, lds, out); return; }
    // the group's own row: a[0] envs, a[1] steps, a[2] resets, a[3] segments, a[4] segments dropped
    group_sums<5>(b.group, g, N, lds, [&b](int e, double* a) {
      a[0] += 1.0; a[1] += (double)b.steps[e]; a[2] += (double)b.resets[e]; a[3] += (double)b.segments[e]; a[4] += (double)b.segments_dropped[e];
    });
    if (t != 0) return;
    out[GO1SPECTRUM_G_ENVS] = lds[0][0]; out[GO1SPECTRUM_G_STEPS] = lds[1][0]; out[GO1SPECTRUM_G_RESETS] = lds[2][0];
    out[GO1SPECTRUM_G_SEGMENTS] = lds[3][0]; out[GO1SPECTRUM_G_SEGMENTS_DROPPED] = lds[4][0]; out[5] = 0.0;
    return;
  }
  // (group, signal, j): bin j of the density sum, or for j = F the segments that entered it
  const int i = (int)blockIdx.x - G * rows;
  const int g = i / (S * (F + 1)), s = (i / (F + 1)) % S, j = i % (F + 1);
  if (j < F) {
    const double* psd = b.psd_sum + ((size_t)s * F + j) * N;
    group_sums<1>(b.group, g, N, lds, [psd](int e, double* a) { a[0] += psd[e]; });
    if (t == 0) b.psd_results[((size_t)g * S + s) * F + j] = lds[0][0];
  } else {
    const uint32_t* seg = b.psd_segments + (size_t)s * N;
    group_sums<1>(b.group, g, N, lds, [seg](int e, double* a) { a[0] += (double)seg[e]; });
    if (t == 0) b.psd_counts[(size_t)g * S + s] = lds[0][0];
  }
}

// ---- the entry points: validation in the order the header gives the codes, then one launch ---------------------------------------------
namespace {
// what every entry point asks first: -1, -2
int check(const Go1SpectrumConfig* cfg, const Go1SpectrumBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0) return -1;
  if (!has_accumulators(buf) || !buf->ring || !buf->valid || !buf->steps || !buf->resets || !buf->segments || !buf->segments_dropped ||
      !buf->psd_sum || !buf->psd_segments) return -2;
  return 0;
}
// the segment length sizes ring and psd_sum: refused (-12) by every entry point
bool bad_segment(const Go1SpectrumConfig* cfg) { return cfg->segment_steps < WMIN || cfg->segment_steps > WMAX || cfg->segment_steps % 2 != 0; }
}  // namespace

extern "C" int go1spectrum_clear(const Go1SpectrumConfig* cfg, const Go1SpectrumBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (bad_segment(cfg)) return -12;
  return launch(spectrum_clear_kernel, env_grid(cfg->num_envs), ACC_THREADS, stream, cfg, buf);
}

extern "C" int go1spectrum_record(const Go1SpectrumConfig* cfg, const Go1SpectrumBuffers* buf, int32_t slot, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->actions || !buf->torques || !buf->dof_vel || !buf->base_ang_vel || !buf->base_lin_vel || !buf->reset_buf ||
      !buf->episode_length_buf) return -3;
  if (slot < 0 || slot >= cfg->segment_steps) return -7;
  if (bad_segment(cfg)) return -12;
  RecordArgs A; A.c = *cfg; A.b = *buf; A.slot = slot;
  return launch_args(spectrum_record_kernel, row_grid(S, cfg->num_envs), ACC_THREADS, stream, A);
}

extern "C" int go1spectrum_fold(const Go1SpectrumConfig* cfg, const Go1SpectrumBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!buf->tw_re || !buf->tw_im || !buf->scale || !buf->freq) return -3;
  if (bad_segment(cfg) || cfg->high_bin < 1 || cfg->high_bin > cfg->segment_steps / 2 || !positive(cfg->bin_width)) return -12;
  const dim3 grid((unsigned)(S * ((cfg->num_envs + FT - 1) / FT)));
  return launch(spectrum_fold_kernel, grid, FT, stream, cfg, buf);
}

extern "C" int go1spectrum_reduce(const Go1SpectrumConfig* cfg, const Go1SpectrumBuffers* buf, void* stream) {
  if (int rc = check(cfg, buf)) return rc;
  if (!has_table(cfg, buf) || !buf->psd_results || !buf->psd_counts) return -5;
  if (bad_segment(cfg)) return -12;
  const int F = cfg->segment_steps / 2 + 1;
  return launch(spectrum_reduce_kernel, table_grid(cfg->num_groups, ROWS + 1 + S * (F + 1)), RT, stream, cfg, buf);
}

#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"
#endif
extern "C" const char* go1spectrum_version(void) { return "go1spectrum 0.1 (gfx950) go1-src:" GO1_SOURCE_HASH; }
