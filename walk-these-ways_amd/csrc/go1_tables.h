// go1_tables.h — what the metric-table libraries share, written once: the six accumulators of a metric row, the fixed-order reduction
// of a group's members into a row of a result table, and the validation and launch helpers of the entry points.
//
// Included exactly once by each library's one .hip (so everything lives in an anonymous namespace), listed in each library's sources
// (so each stamp covers it), and tied to each public header by GO1_TABLES_MATCH.  It includes no public header and names no library:
// a buffer type is whatever has the members a function touches.
//
// Device side: Args (a kernel's one argument: config and buffers by value), Row (a row of an SoA buffer at the thread's environment),
// row_thread (the launch of one thread per (row, environment)), clear_rows and fold (the accumulators of a metric row), tree_reduce
// (the binary tree of fixed shape in LDS), group_sums and reduce_metric_row (the strided pass in front of it: sums over a group's members,
// and a metric row), bin_sums (the same for sixteen bins at once).  Nothing here decides an order of additions twice.
// Host side: env_grid, row_grid, table_grid, launch_args / launch, has_accumulators, has_table, finite, positive.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int ACC_THREADS = 256, RT = 256, NF = 6;
constexpr int F_COUNT = 0, F_MEAN = 1, F_STD = 2, F_MIN = 3, F_MAX = 4, F_NONFINITE = 5;       // the fields of a metric row
constexpr int BINS = 16, SLICES = RT / BINS;                                                   // bin_sums: slices of members per bin
static_assert(RT == 256 && BINS * SLICES == RT, "bin_sums: sixteen slices of members per bin");

// a library's public macros (prefix P) are this header's constants
#define GO1_TABLES_MATCH(P)                                                                                                         \
  static_assert(P##_NUM_FIELDS == NF && P##_REDUCE_THREADS == RT && P##_F_COUNT == F_COUNT && P##_F_MEAN == F_MEAN &&              \
                P##_F_STD == F_STD && P##_F_MIN == F_MIN && P##_F_MAX == F_MAX && P##_F_NONFINITE == F_NONFINITE,                  \
                #P ": the public header and go1_tables.h disagree about a metric row")

// a kernel's one argument: the caller's config and buffers, by value
template <class C, class B>
struct Args {
  C c;
  B b;
};

// row k of an SoA buffer ([k][N]) at environment e
struct Row {
  int N, e;
  __device__ __forceinline__ float operator()(const float* p, int k) const { return p[(size_t)k * N + e]; }
};

// the launch of one thread per (row, environment): block k is row k / blocks_per_row, its lanes consecutive environments
__device__ __forceinline__ bool row_thread(int N, int rows, int* r, int* e) {
  const int per_row = (N + ACC_THREADS - 1) / ACC_THREADS;
  *r = (int)blockIdx.x / per_row;
  *e = ((int)blockIdx.x % per_row) * ACC_THREADS + (int)threadIdx.x;
  return *r < rows && *e < N;
}

// rows first_row ... first_row + rows - 1 of the accumulators of environment e: nothing folded yet
template <class Buffers>
__device__ __forceinline__ void clear_rows(const Buffers& b, int first_row, int rows, int N, int e) {
  for (int m = 0; m < rows; m++) {
    const size_t i = (size_t)(first_row + m) * N + e;
    b.count[i] = 0u; b.nonfinite[i] = 0u; b.sum[i] = 0.0; b.sumsq[i] = 0.0; b.min[i] = INFINITY; b.max[i] = -INFINITY;
  }
}

template <class Buffers>
__device__ __forceinline__ void fold(const Buffers& b, int m, int N, int e, float v) {
  const size_t i = (size_t)m * N + e;
  if (!isfinite(v)) { b.nonfinite[i] += 1u; return; }
  b.count[i] += 1u;
  b.sum[i] += (double)v;
  b.sumsq[i] += (double)v * (double)v;
  b.min[i] = fminf(b.min[i], v);
  b.max[i] = fmaxf(b.max[i], v);
}

// the binary tree of fixed shape over the partial results of a workgroup of RT threads, thread t's in lds[f][t]: sums in rows
// 0 ... F - 1 and, with MinMax, a minimum in row F and a maximum in row F + 1.  Afterwards lds[f][0] holds the workgroup's; a tree
// that stops at Width leaves Width results, lds[f][k] the one over the threads t with t % Width == k.
template <int F, bool MinMax = false, int Width = 1>
__device__ __forceinline__ void tree_reduce(double (*lds)[RT], int t) {
  __syncthreads();
  for (int s = RT / 2; s >= Width; s >>= 1) {
    if (t < s) {
      for (int f = 0; f < F; f++) lds[f][t] += lds[f][t + s];
      if (MinMax) { lds[F][t] = fmin(lds[F][t], lds[F][t + s]); lds[F + 1][t] = fmax(lds[F + 1][t], lds[F + 1][t + s]); }
    }
    __syncthreads();
  }
}

// F sums over the members of group g, by one workgroup of RT threads: thread t adds term(e, a) for the members e = t, t + RT, ...
// in ascending order, then the tree; lds[f][0] holds sum f
template <int F, class Term>
__device__ __forceinline__ void group_sums(const int32_t* group, int g, int N, double (*lds)[RT], Term term) {
  const int t = (int)threadIdx.x;
  double a[F] = {};
  for (int e = t; e < N; e += RT) {
    if (group[e] != g) continue;
    term(e, a);
  }
  for (int f = 0; f < F; f++) lds[f][t] = a[f];
  tree_reduce<F>(lds, t);
}

// F sums per bin over the members of group g, for BINS bins at once: thread t owns bin t % BINS and adds term(e, a) for the members
// e = t / BINS, t / BINS + SLICES, ... in ascending order, then the tree down to BINS; lds[f][bin] holds sum f of the bin
template <int F, class Term>
__device__ __forceinline__ void bin_sums(const int32_t* group, int g, int N, double (*lds)[RT], Term term) {
  const int t = (int)threadIdx.x;
  double a[F] = {};
  for (int e = t / BINS; e < N; e += SLICES) {
    if (group[e] != g) continue;
    term(e, a);
  }
  for (int f = 0; f < F; f++) lds[f][t] = a[f];
  tree_reduce<F, false, BINS>(lds, t);
}

// one metric row of a result table, by one workgroup of RT threads: thread t combines the group's environments t, t + RT, ... in
// ascending order, then the binary tree in LDS; thread 0 writes the six fields.  a0 count, a1 nonfinite, a2 sum, a3 sumsq, a4 min, a5 max
template <class Buffers>
__device__ __forceinline__ void reduce_metric_row(const Buffers& b, int g, int m, int N, double (*lds)[RT], double* out) {
  const int t = (int)threadIdx.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = (double)INFINITY, a5 = -(double)INFINITY;
  for (int e = t; e < N; e += RT) {
    if (b.group[e] != g) continue;
    const size_t i = (size_t)m * N + e;
    a0 += (double)b.count[i]; a1 += (double)b.nonfinite[i]; a2 += b.sum[i]; a3 += b.sumsq[i];
    if (b.count[i] > 0u) { a4 = fmin(a4, (double)b.min[i]); a5 = fmax(a5, (double)b.max[i]); }
  }
  lds[0][t] = a0; lds[1][t] = a1; lds[2][t] = a2; lds[3][t] = a3; lds[4][t] = a4; lds[5][t] = a5;
  tree_reduce<4, true>(lds, t);
  if (t != 0) return;
  const double nan = (double)NAN;
  const double n = lds[0][0];
  const double mean = n > 0.0 ? lds[2][0] / n : nan;
  const double var = n > 0.0 ? lds[3][0] / n - mean * mean : nan;
  out[F_COUNT] = n; out[F_MEAN] = mean; out[F_STD] = n > 0.0 ? sqrt(fmax(var, 0.0)) : nan;
  out[F_MIN] = n > 0.0 ? lds[4][0] : nan; out[F_MAX] = n > 0.0 ? lds[5][0] : nan; out[F_NONFINITE] = lds[1][0];
}

// ---- the entry points' side: grids, the launch, and what more than one validation asks
dim3 env_grid(int n) { return dim3((unsigned)((n + ACC_THREADS - 1) / ACC_THREADS)); }                  // one thread per environment
dim3 row_grid(int rows, int n) { return dim3((unsigned)(rows * ((n + ACC_THREADS - 1) / ACC_THREADS))); }   // row_thread's
dim3 table_grid(int groups, int rows) { return dim3((unsigned)(groups * rows)); }                       // one workgroup per row of a table

template <class A>
int launch_args(void (*kernel)(A), dim3 grid, int block, void* stream, const A& args) {
  hipLaunchKernelGGL(kernel, grid, dim3(block), 0, (hipStream_t)stream, args);
  return hipGetLastError() == hipSuccess ? 0 : -20;
}
template <class C, class B>
int launch(void (*kernel)(Args<C, B>), dim3 grid, int block, void* stream, const C* cfg, const B* buf) {
  Args<C, B> A; A.c = *cfg; A.b = *buf;
  return launch_args(kernel, grid, block, stream, A);
}

template <class B> bool has_accumulators(const B* buf) { return buf->count && buf->sum && buf->sumsq && buf->min && buf->max && buf->nonfinite; }
template <class C, class B> bool has_table(const C* cfg, const B* buf) { return cfg->num_groups > 0 && buf->group && buf->results; }      // else -5
bool finite(float x) { return x >= -3.402823466e38f && x <= 3.402823466e38f; }          // (a NaN fails both)
bool positive(float x) { return x > 0.0f && x <= 3.402823466e38f; }                     // finite and positive (a NaN fails both)

}  // namespace
