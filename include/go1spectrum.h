/* go1spectrum.h — C-ABI of libgo1spectrum.so: the power spectra of a policy rollout's actions, torques, joint speeds and trunk rates,
 * measured on the device (HIP, gfx950).
 *
 * Every other family reduces a rollout to per-step means or per-stride events.  None looks at a signal in the frequency domain: whether
 * a policy chatters, how much of the action and torque energy sits above what the actuators can follow, whether the motion is locked to
 * the commanded step frequency or is broadband.  This library is that family.  It keeps, per environment, a ring of the last
 * segment_steps samples of forty signals; at every close of a segment it transforms them (Welch's method without overlap: the mean
 * removed, a taper, a direct DFT of any even length) and folds five band figures per signal into the tables' accumulators and the power
 * spectral density (PSD) into a running sum.  It is a library of its own, as the evaluation, foot, trunk and gait libraries are: no other
 * binary, stamp or parity result depends on it.  The accumulators, the folding rule, the fixed-order reduction and the numbering of the
 * return codes are go1eval.h's, restated here (the device helpers are csrc/go1_tables.h's, shared with those libraries and covered by
 * this library's stamp).  This header is the specification: tests/spectrum_ref.py is written from its text.
 *
 * Layout: every buffer is SoA, [k][N] with the environment last, as the simulator's (go1sim.h).
 *
 * The S = GO1SPECTRUM_SIGNALS = 40 signals, read after the simulator's step:
 *   s  0 .. 11   actions[s]                the clipped action of the step
 *   s 12 .. 23   torques[s - 12]           N m, of the LAST SUBSTEP
 *   s 24 .. 35   dof_vel[s - 24]           rad/s
 *   s 36, 37, 38 base_ang_vel[s - 36]      roll, pitch and yaw rate, rad/s
 *   s 39         base_lin_vel[2]           vertical velocity, m/s
 *
 * Segments.  W = segment_steps is even, 8 <= W <= GO1SPECTRUM_MAX_SEGMENT = 128, and F = W / 2 + 1 bins.  The segments follow the
 * family's own clock, not the episodes': the host counts its go1spectrum_record calls since the clear and hands each one
 * slot = calls mod W; after the record of slot W - 1 it launches go1spectrum_fold.  No device-to-host read is involved.
 *
 * The device computes no trigonometric function.  The host computes four tables in fp64, rounds them to fp32 and uploads them:
 *   tw_re[k][t] = w[t] cos(2 pi k t / W)         [F][W]
 *   tw_im[k][t] = - w[t] sin(2 pi k t / W)       [F][W]
 *   scale[k]    = 2 / (fs sum_t w[t]^2), and 1 / (fs sum_t w[t]^2) for k = 0 and k = W / 2       [F]: the one-sided density scale
 *   freq[k]     = k fs / W                       [F], Hz
 * with fs = 1 / dt and w the taper (the host's choice: periodic Hann, w[t] = 0.5 - 0.5 cos(2 pi t / W), or boxcar; the device sees
 * tables only).  bin_width = fs / W is in the config.
 *
 * Every operation is an fp32 operation on fp32 values in the order written (the library is built with -ffp-contract=off), the
 * accumulators' and psd_sum's additions in fp64.  Only + - * /, conversions and comparisons are used.
 *
 * Five rows per signal (index = Go1SpectrumMetric m, accumulator row = s * GO1SPECTRUM_NUM + m, S * 5 = 200 rows):
 *   power       total * bin_width: the variance of the tapered signal, in the signal's units squared
 *   peak_freq   freq[kp], Hz
 *   peak_share  P[kp] / total
 *   high_share  (P[high_bin] + ... + P[F - 1]) / total
 *   centroid    (sum over k >= 1 of freq[k] * P[k]) / total, Hz
 * The folding rule is go1eval_accumulate's: a non-finite value adds 1 to nonfinite[row][e] and enters nothing else; a finite value v adds
 * 1 to count, (double)v to sum, (double)v * (double)v to sumsq, and enters min by fminf and max by fmaxf.
 *
 * State per environment: ring [W][S] (float: the samples of the open segment, slot first); valid (uint8: 1 while every step of the
 * open segment was live); steps, resets, segments and segments_dropped (uint32); psd_sum [S][F] (double: the sum of the densities of
 * the folded segments) and psd_segments [S] (uint32: how many entered it).
 *
 * go1spectrum_clear: one launch, one thread per environment: accumulators as go1eval_clear (count = nonfinite = 0, sum = sumsq = 0,
 *   min = +inf, max = -inf), psd_sum, psd_segments and the four counters 0, valid = 0.  The ring is left as it is: every word of it is
 *   written before a fold reads it.
 *
 * go1spectrum_record(cfg, buf, slot, stream): one launch per step, one thread per (signal, environment): S * ceil(N / 256) blocks of 256
 *   threads, block b is signal b / ceil(N / 256).  ring[slot][s][e] = the signal's value.  The s = 0 thread of an environment also keeps
 *   the segment's state, in this order:
 *     steps[e] += 1, and resets[e] += 1 if reset_buf[e] != 0
 *     live = reset_buf[e] == 0 && episode_length_buf[e] > warmup_steps
 *     valid[e] = live if slot == 0, else valid[e] & live
 *   So a segment that holds a reset or a warm-up step is spoiled as a whole, and the environment measures again from the next segment
 *   of the family's clock on.
 *
 * go1spectrum_fold(cfg, buf, stream): after slot W - 1 has been recorded.  One thread per (signal, environment): S * ceil(N / 64)
 *   blocks of GO1SPECTRUM_FOLD_THREADS = 64 threads (one wavefront: the lane is the environment), block b is signal b / ceil(N / 64).
 *   Every word has one writer; there are no atomics.  Per environment e: if valid[e] == 0, segments_dropped[e] += 1 (by the s = 0
 *   thread) and nothing else happens.  Otherwise segments[e] += 1 (the s = 0 thread), and per signal s, with x[t] = ring[t][s][e]:
 *     1. sum = 0; for t = 0 .. W - 1: sum = sum + x[t].  mean = sum / (float)W.  y[t] = x[t] - mean.
 *     2. for k = 0 .. F - 1 (k outer, t inner): re = im = 0; for t = 0 .. W - 1: re = re + y[t] * tw_re[k][t], im = im + y[t] * tw_im[k][t]
 *        (the product is rounded, then the sum).  P[k] = (re * re + im * im) * scale[k].
 *     3. total = 0; for k = 1 .. F - 1: total = total + P[k].  kp = 1, best = P[1]; for k = 2 .. F - 1: if P[k] > best then kp = k and
 *        best = P[k] (so the smallest k with the largest P wins a tie, and a NaN never wins a comparison).
 *     4. power = total * bin_width is folded.  If total is finite and total > 0:
 *          peak_freq = freq[kp]; peak_share = P[kp] / total;
 *          high = 0; for k = high_bin .. F - 1: high = high + P[k]; high_share = high / total;
 *          c = 0; for k = 1 .. F - 1: c = c + freq[k] * P[k]; centroid = c / total;
 *        otherwise (total is 0, infinite or a NaN) the four are NaN.  All four are folded: a robot that stands still adds a power of 0
 *        and four counts to nonfinite, and invents no peak.
 *     5. Only if total is finite: for k = 0 .. F - 1: psd_sum[s][k][e] += (double)P[k]; psd_segments[s][e] += 1.  (P[0] is the taper's
 *        leakage of the removed mean: near 0, kept for completeness.  A finite total does not make P[0] finite; a non-finite P[0] enters
 *        psd_sum as it is.)
 *   The twiddle index [k][t] is the same for every lane, so the tables are read through wave-uniform addresses; y and P of the 64
 *   environments of a block live in LDS (static: y [128][64] and P [65][64] floats, 48.25 KB), each lane in its own column.
 *
 * go1spectrum_reduce: ONE launch of GO1SPECTRUM_REDUCE_THREADS-thread workgroups, which leaves what it reads as it is:
 *   num_groups * (S * 5 + 1) workgroups write results[num_groups][S * 5 + 1][GO1SPECTRUM_NUM_FIELDS].
 *     Rows 0 .. S * 5 - 1: go1eval_reduce's metric rows in its fixed combination order: thread t combines the group's environments
 *     e = t, t + 256, ... in ascending order in fp64 (count, nonfinite, sum, sumsq as sums; min and max only of environments with
 *     count > 0), then a binary tree over the 256 partial results (thread t takes thread t + 128, then + 64, ... + 1).  Fields
 *     (index = Go1SpectrumField): count, mean = sum / count, std = sqrt(max(sumsq / count - mean * mean, 0)), min, max, nonfinite; with
 *     count = 0 the four in the middle are NaN.
 *     The last row of a group (index = Go1SpectrumGroupField): environments, steps (sum of steps[e]), resets, segments,
 *     segments_dropped, then 0, in the same order.
 *   num_groups * S * (F + 1) further workgroups, one per (group, signal, j): for j < F, psd_results[g][s][j] = the sum of
 *     psd_sum[s][j][e] over the group's environments; for j = F, psd_counts[g][s] = the sum of (double) psd_segments[s][e].  Both in the
 *     same order: thread t adds e = t, t + 256, ... ascending, then the binary tree.  The mean density is the host's division.
 *
 * Return codes: 0, or before any launch, tested in this order (where two conditions fail at once, the one listed first wins):
 *   -1   no config, no buffers, or num_envs <= 0
 *   -2   an accumulator or a state array (ring, valid, a counter, psd_sum, psd_segments) is missing
 *   -3   an input is missing: a simulator buffer (go1spectrum_record), or tw_re, tw_im, scale or freq (go1spectrum_fold)
 *   -5   no group, no table, no psd_results, no psd_counts, or num_groups <= 0 (go1spectrum_reduce only)
 *   -7   slot outside [0, segment_steps) (go1spectrum_record only)
 *   -12  segment_steps odd or outside [8, 128] (every entry point: it sizes ring and psd_sum); high_bin outside [1, F - 1], or bin_width
 *        not finite and positive (go1spectrum_fold only)
 *   -20  the launch itself failed
 *
 * What the figures are not.  The segments follow the family's clock: an environment that resets loses the rest of that segment and
 * does not start a new one at once.  actions are the clipped actions; torques are the last substep's, one sample in four.  Segments do
 * not overlap.  The Hann taper spreads a line that sits on a bin over three bins (1/4, 1/2, 1/4 in amplitude), so the peak_share of a
 * pure on-bin sine is 2/3, not 1.  The mean of a segment is removed, a trend is not.
 */
#ifndef GO1SPECTRUM_H
#define GO1SPECTRUM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1SPECTRUM_SIGNALS 40
#define GO1SPECTRUM_NUM 5
#define GO1SPECTRUM_MIN_SEGMENT 8
#define GO1SPECTRUM_MAX_SEGMENT 128
#define GO1SPECTRUM_FOLD_THREADS 64
#define GO1SPECTRUM_NUM_FIELDS 6
#define GO1SPECTRUM_REDUCE_THREADS 256

/* the five rows of a signal; the accumulator row of signal s is s * GO1SPECTRUM_NUM + m */
enum Go1SpectrumMetric { GO1SPECTRUM_POWER = 0, GO1SPECTRUM_PEAK_FREQ = 1, GO1SPECTRUM_PEAK_SHARE = 2, GO1SPECTRUM_HIGH_SHARE = 3, GO1SPECTRUM_CENTROID = 4 };
/* columns of a metric row */
enum Go1SpectrumField { GO1SPECTRUM_F_COUNT = 0, GO1SPECTRUM_F_MEAN = 1, GO1SPECTRUM_F_STD = 2, GO1SPECTRUM_F_MIN = 3, GO1SPECTRUM_F_MAX = 4, GO1SPECTRUM_F_NONFINITE = 5 };
/* columns of a group's own row (row GO1SPECTRUM_SIGNALS * GO1SPECTRUM_NUM) */
enum Go1SpectrumGroupField { GO1SPECTRUM_G_ENVS = 0, GO1SPECTRUM_G_STEPS = 1, GO1SPECTRUM_G_RESETS = 2, GO1SPECTRUM_G_SEGMENTS = 3, GO1SPECTRUM_G_SEGMENTS_DROPPED = 4 };

typedef struct Go1SpectrumConfig {
  int32_t num_envs;            /* N of the simulator's SoA buffers */
  int32_t warmup_steps;        /* a step with episode_length_buf <= warmup_steps spoils its segment */
  int32_t num_groups;          /* G of the result tables */
  int32_t segment_steps;       /* W: even, 8 .. 128; 100 is 2 s at a 0.02 s policy step */
  int32_t high_bin;            /* the first bin of high_share, 1 .. W / 2 */
  float bin_width;             /* fs / W, Hz */
} Go1SpectrumConfig;

typedef struct Go1SpectrumBuffers {
  /* read by go1spectrum_record */
  const float* actions;               /* [12][N] */
  const float* torques;               /* [12][N] */
  const float* dof_vel;               /* [12][N] */
  const float* base_ang_vel;          /* [3][N] */
  const float* base_lin_vel;          /* [3][N] */
  const uint8_t* reset_buf;           /* [N] */
  const int32_t* episode_length_buf;  /* [N] */
  /* read by go1spectrum_fold: the host's tables */
  const float* tw_re;                 /* [F][W] */
  const float* tw_im;                 /* [F][W] */
  const float* scale;                 /* [F] */
  const float* freq;                  /* [F] */
  /* accumulators, [GO1SPECTRUM_SIGNALS * GO1SPECTRUM_NUM][N] */
  uint32_t* count;
  double* sum;
  double* sumsq;
  float* min;
  float* max;
  uint32_t* nonfinite;
  /* state */
  float* ring;                        /* [W][GO1SPECTRUM_SIGNALS][N]: the open segment's samples */
  uint8_t* valid;                     /* [N]: every step of the open segment was live */
  uint32_t* steps;                    /* [N]: record launches since the clear */
  uint32_t* resets;                   /* [N]: of those, the steps that reset the environment */
  uint32_t* segments;                 /* [N]: segments folded */
  uint32_t* segments_dropped;         /* [N]: segments closed with valid = 0 */
  double* psd_sum;                    /* [GO1SPECTRUM_SIGNALS][F][N]: the sum of the folded segments' densities */
  uint32_t* psd_segments;             /* [GO1SPECTRUM_SIGNALS][N]: the segments that entered psd_sum */
  /* go1spectrum_reduce */
  const int32_t* group;               /* [N]: the group an environment counts towards; outside [0, num_groups): none */
  double* results;                    /* [num_groups][GO1SPECTRUM_SIGNALS * GO1SPECTRUM_NUM + 1][GO1SPECTRUM_NUM_FIELDS] */
  double* psd_results;                /* [num_groups][GO1SPECTRUM_SIGNALS][F] */
  double* psd_counts;                 /* [num_groups][GO1SPECTRUM_SIGNALS] */
} Go1SpectrumBuffers;

/* empty accumulators and density sums, no valid segment.  One launch, one thread per environment. */
int go1spectrum_clear(const Go1SpectrumConfig* cfg, const Go1SpectrumBuffers* buf, void* stream);

/* after a simulator step: the step's forty samples into slot `slot` of the ring.  One launch, one thread per (signal, environment). */
int go1spectrum_record(const Go1SpectrumConfig* cfg, const Go1SpectrumBuffers* buf, int32_t slot, void* stream);

/* after the record of slot segment_steps - 1: transform and fold the segment.  One launch, one thread per (signal, environment). */
int go1spectrum_fold(const Go1SpectrumConfig* cfg, const Go1SpectrumBuffers* buf, void* stream);

/* at the end: the result tables from the accumulators, the density sums and the state (which it leaves as they are).  One launch. */
int go1spectrum_reduce(const Go1SpectrumConfig* cfg, const Go1SpectrumBuffers* buf, void* stream);

/* "go1spectrum <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1spectrum_version(void);

#ifdef __cplusplus
}
#endif

#endif
