// go1ppo_mlp.h — the 256 -> 128 -> 64 end of the three MLPs (actor / critic behind their 512 -> 256 layer, the
// adaptation module behind the shared first layer), forward and backward, with BOTH weight matrices resident in LDS.
//
// In the reference these are two nn.Linear + ELU per net (actor_critic.py:51-92); as separate launches they are, per
// net and direction, two small GEMMs and two element-wise passes over (rows x 256/128) activations that are all
// launch / latency bound (6-11 us each at 24576 rows).  Here one workgroup owns 64 rows:
//   forward : h0 = elu(x) (x: the pre-activation the previous GEMM left, activated IN PLACE for the backward pass),
//             z2 = elu(h0 W2^T + b2) (kept on chip and written out for the backward pass), out = z2 W3^T + b3;
//   backward: dz2 = (d_out W3) * elu'(z2), dx = (dz2 W2) * elu'(h0); dz2 and dx are what the weight-gradient kernel
//             and the layer in front need, nothing else is written.
// bf16 MFMA 16x16x32 throughout.  LDS images have 256-byte rows (128 bf16; wider matrices = several images side by
// side) with the 16-byte chunk index XOR-swizzled: by (row & 15) for operands whose reduction index is contiguous
// (ds_read_b128 fragments), by 2 ((row & 3) | ((row >> 3) & 1) << 2) for the backward pass's weights, whose reduction
// index is the ROW (ds_read_b64_tr_b16 fragments, as in the weight-gradient kernel).  Weights arrive by LDS-DMA with
// the swizzle applied on the source address; the weight operand is always the MFMA "A" side, so a lane ends up with 4
// consecutive output columns of one row and all global traffic is 8/16-byte wide.
//
// mlp2_tail_ppo_kernel / mlp2_tail_mse_kernel (further down) run forward, loss and backward of a 64-row tile in ONE launch, bit for bit what
// the three launches compute.  Their LDS map, 153.5 KB of the CU's 160:
//   W2i 64 KB + W3i 16 KB   ONE image per weight matrix (chunk swizzle by row & 15) for both fragment kinds: ds_read_b128 forward (reduction
//                           index contiguous), ds_read_tr16_b64 backward (reduction index = row)
//   Ai  32 KB               x -> h = elu(x) -> dx, each in the slot of the value it replaces
//   Z2i 16 KB               z2 -> dz2
//   D3i 16 KB               64 rows x 16 chunks of 16 B: chunk c < 8 of d_out at slot c ^ (row & 15), chunk c of the head at slot (c | 8) ^ (row & 15)
//   Gi  9.5 KB              the loss's gathers from the rollout storage, by LDS-DMA a stage ahead; later z[j] and the per-action terms
#pragma once

#define MLP2_K1 256
#define MLP2_N2 128
#define MLP2_N3 64
#define MLP2_BM 64
#define MLP2_WAVES 16
#define MLP2_THREADS (64 * MLP2_WAVES)
#define MLP2_IMG (128 * 128)          // elements of a [128 rows][128 columns] image (weights); row tiles use the first 64 rows

struct Mlp2FwdArgs { Go1PpoMlp2Fwd net[GO1PPO_MLP2_MAX_NETS]; };
struct Mlp2BwdArgs { Go1PpoMlp2Bwd net[GO1PPO_MLP2_MAX_NETS]; };

__device__ __forceinline__ int swz_row(int row) { return row & 15; }
__device__ __forceinline__ int swz_red(int row) { return 2 * ((row & 3) | (((row >> 3) & 1) << 2)); }

// W [rows][cols] row-major bf16 -> cols/128 images [rows][128], chunk swizzle by `RED ? swz_red : swz_row`; all waves
template <bool RED>
__device__ __forceinline__ void dma_weights(const bf16_t* W, int rows, int cols, bf16_t* img, int wave, int lane) {
  const int windows = cols >> 7, count = (rows >> 2) * windows;         // one DMA instruction = 4 rows of one window
  for (int idx = wave; idx < count; idx += MLP2_WAVES) {
    const int win = idx % windows, blk = idx / windows;
    const int row = blk * 4 + (lane >> 4);
    const int chunk = (lane & 15) ^ (RED ? swz_red(row) : swz_row(row));
    glds16(W + (int64_t)row * cols + win * 128 + chunk * 8, img + win * MLP2_IMG + blk * 4 * 128);
  }
}

__device__ __forceinline__ uint2 pack_bf4(const float (&v)[4]) {
  f32x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
  uint2 o;
  o.x = __builtin_bit_cast(uint32_t, __builtin_convertvector(lo, bf16x2_t));
  o.y = __builtin_bit_cast(uint32_t, __builtin_convertvector(hi, bf16x2_t));
  return o;
}
__device__ __forceinline__ void unpack_bf4(uint2 r, float (&v)[4]) {
  v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
  v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
}
__device__ __forceinline__ bf16x8_t lds_b128(const bf16_t* img, int byte_off) {
  return *reinterpret_cast<const bf16x8_t*>(reinterpret_cast<const char*>(img) + byte_off);
}
// transpose-read operand: rows (reduction) 8g + (i16 >> 2) [+4] of a 32-row slab, 16 columns starting at `col`
__device__ __forceinline__ bf16x8_t lds_tr_operand(const bf16_t* img, int byte_off) {
  typedef __attribute__((address_space(3))) s16x4_t lds_s16x4_t;
  const char* p = reinterpret_cast<const char*>(img) + byte_off;
  s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(p));
  s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(p + 4 * 256));
  s16x8_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8_t, v);
}

// ------------------------------------------------------------------------------------------------------------ forward
// 16 waves per workgroup (one workgroup per CU: the weights take 80 KB of its LDS), so that the element-wise stages and
// the LDS / MFMA latencies of a tile overlap across 4 waves per SIMD; the workgroup keeps the weights and walks over
// row tiles with the next tile's rows in flight during the MFMAs.
__global__ __launch_bounds__(MLP2_THREADS, 1) void mlp2_fwd_kernel(Mlp2FwdArgs A) {
  __shared__ __attribute__((aligned(1024))) bf16_t W2i[2 * MLP2_IMG];     // [k window][n2][128 k]      64 KB
  __shared__ __attribute__((aligned(1024))) bf16_t W3i[64 * 128];         // [n3][128 k]                16 KB
  __shared__ __attribute__((aligned(1024))) bf16_t Ai[2 * 64 * 128];      // [k window][m][128 k]       32 KB
  __shared__ __attribute__((aligned(1024))) bf16_t Z2i[64 * 128];         // [m][128 k]                 16 KB
  const Go1PpoMlp2Fwd& N = A.net[blockIdx.y];
  const int tiles = (int)((N.rows + MLP2_BM - 1) / MLP2_BM);
  if ((int)blockIdx.x >= tiles) return;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 15, g = lane >> 4;
  dma_weights<false>((const bf16_t*)N.W2, MLP2_N2, MLP2_K1, W2i, wave, lane);
  dma_weights<false>((const bf16_t*)N.W3, MLP2_N3, MLP2_N2, W3i, wave, lane);
  bf16_t* x = (bf16_t*)N.x;
  bf16_t* z2 = (bf16_t*)N.z2;
  bf16_t* out = (bf16_t*)N.out;
  // lane offset of a b128 fragment read: row r of the fragment, chunk (4 (ks & 3) + g) ^ r = (4 (ks & 3)) ^ (g ^ r)
  const int tx = g ^ r;
  int foff[4];
#pragma unroll
  for (int a = 0; a < 4; a++) foff[a] = r * 256 + (((4 * a) ^ tx) << 4);
  // hidden layer: wave -> n fragment wave >> 1, row fragments 2 (wave & 1), +1; head: n3 fragment wave & 3, row fragment wave >> 2
  const int nf2 = wave >> 1, mp = (wave & 1) * 2, nf3 = wave & 3, m3 = wave >> 2;
  float bias2[4], bias3[4];
  unpack_bf4(*reinterpret_cast<const uint2*>((const bf16_t*)N.b2 + nf2 * 16 + 4 * g), bias2);
  unpack_bf4(*reinterpret_cast<const uint2*>((const bf16_t*)N.b3 + nf3 * 16 + 4 * g), bias3);

  Bf8 v[2];
  auto fetch = [&](int tile) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int p = t + MLP2_THREADS * j, row = p >> 5, ch = p & 31;
      int64_t grow = (int64_t)tile * MLP2_BM + row;
      grow = grow < N.rows ? grow : N.rows - 1;
      v[j] = *reinterpret_cast<const Bf8*>(x + grow * N.ld_x + ch * 8);
    }
  };
  fetch(blockIdx.x);
  bool first = true;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = (int64_t)tile * MLP2_BM;
    // ---- input rows: ELU, write-back, swizzled LDS image
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int p = t + MLP2_THREADS * j, row = p >> 5, ch = p & 31;
      if (N.elu_input) {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; e++) f[e] = elu1(bf2f(v[j].v[e]));
        v[j] = pack_bf8(f);
        if (row0 + row < N.rows) *reinterpret_cast<Bf8*>(x + (row0 + row) * N.ld_x + ch * 8) = v[j];
      }
      *reinterpret_cast<Bf8*>(reinterpret_cast<char*>(Ai + (ch >> 4) * 64 * 128) + row * 256 + (((ch & 15) ^ swz_row(row)) << 4)) = v[j];
    }
    if (first) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the weights
    first = false;
    __syncthreads();
    if (tile + (int)gridDim.x < tiles) fetch(tile + gridDim.x);
    // ---- hidden layer
    {
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ks = 0; ks < MLP2_K1 / 32; ks++) {
        const int win = ks >> 2, off = foff[ks & 3];
        const bf16x8_t w = lds_b128(W2i + win * MLP2_IMG + nf2 * 16 * 128, off);
#pragma unroll
        for (int m = 0; m < 2; m++)
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, lds_b128(Ai + win * 64 * 128 + (mp + m) * 16 * 128, off), acc[m], 0, 0, 0);
      }
      const int n0 = nf2 * 16 + 4 * g;
#pragma unroll
      for (int m = 0; m < 2; m++) {
        const int row = (mp + m) * 16 + r;
        float o4[4];
#pragma unroll
        for (int e = 0; e < 4; e++) o4[e] = elu1(acc[m][e] + bias2[e]);
        const uint2 o = pack_bf4(o4);
        if (row0 + row < N.rows) *reinterpret_cast<uint2*>(z2 + (row0 + row) * N.ld_z2 + n0) = o;
        *reinterpret_cast<uint2*>(reinterpret_cast<char*>(Z2i) + row * 256 + (((n0 >> 3) ^ swz_row(row)) << 4) + ((n0 >> 2) & 1) * 8) = o;
      }
    }
    __syncthreads();
    // ---- head
    {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < MLP2_N2 / 32; ks++)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_b128(W3i + nf3 * 16 * 128, foff[ks]), lds_b128(Z2i + m3 * 16 * 128, foff[ks]), acc, 0, 0, 0);
      const int n0 = nf3 * 16 + 4 * g, row = m3 * 16 + r;
      float o4[4];
#pragma unroll
      for (int e = 0; e < 4; e++) o4[e] = acc[e] + bias3[e];
      if (row0 + row < N.rows) *reinterpret_cast<uint2*>(out + (row0 + row) * N.ld_out + n0) = pack_bf4(o4);
    }
    // the next iteration's Ai / Z2i writes sit behind barriers every wave only reaches once it is done reading here
  }
}

// ----------------------------------------------------------------------------------------------------------- backward
// All global traffic of a tile is whole rows (16 bytes per lane, consecutive lanes on consecutive addresses): d_out, z2
// and h come in through registers one tile ahead and are laid out in LDS; the MFMA epilogues read the activation they
// multiply by from LDS and write the gradient back INTO THE SAME LDS SLOT; the finished dz2 / dx tiles then leave LDS
// row by row.  (Fragment-shaped 8-byte global accesses — 16 rows x 32 B per instruction — made this kernel 3x slower.)
__global__ __launch_bounds__(MLP2_THREADS, 1) void mlp2_bwd_kernel(Mlp2BwdArgs A) {
  __shared__ __attribute__((aligned(1024))) bf16_t W3t[64 * 128];         // [n3][128 k2], reduction = row        16 KB
  __shared__ __attribute__((aligned(1024))) bf16_t W2t[2 * MLP2_IMG];     // [k1 window][n2][128 k1]             64 KB
  __shared__ __attribute__((aligned(1024))) bf16_t D3i[64 * 128];         // [m][64 n3 (of 128)]                 16 KB
  __shared__ __attribute__((aligned(1024))) bf16_t D2i[64 * 128];         // [m][128]: z2, then dz2              16 KB
  __shared__ __attribute__((aligned(1024))) bf16_t Hi[2 * 64 * 128];      // [k1 window][m][128]: h, then dx     32 KB
  const Go1PpoMlp2Bwd& N = A.net[blockIdx.y];
  const int tiles = (int)((N.rows + MLP2_BM - 1) / MLP2_BM);
  if ((int)blockIdx.x >= tiles) return;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 15, g = lane >> 4;
  dma_weights<true>((const bf16_t*)N.W3, MLP2_N3, MLP2_N2, W3t, wave, lane);
  dma_weights<true>((const bf16_t*)N.W2, MLP2_N2, MLP2_K1, W2t, wave, lane);
  const bf16_t* d = (const bf16_t*)N.d_out;
  const bf16_t* z2 = (const bf16_t*)N.z2;
  const bf16_t* hin = (const bf16_t*)N.h;
  bf16_t* dz2 = (bf16_t*)N.d_z2;
  bf16_t* dx = (bf16_t*)N.d_x;
  const int tx = g ^ r;
  int foff[4];                                                            // b128 fragments (activation gradients)
#pragma unroll
  for (int a = 0; a < 4; a++) foff[a] = r * 256 + (((4 * a) ^ tx) << 4);
  // transpose-read pieces (weights): row 8g + (r >> 2) of a 32-row slab, 8 bytes at column 16 f + 4 (r & 3)
  const int troff = (g * 8 + (r >> 2)) * 256 + ((r & 3) >> 1) * 16 + (r & 1) * 8;
  const int swb = 32 * ((r >> 2) | ((g & 1) << 2));
  // dz2: wave -> k2 fragment wave >> 1, row fragments 2 (wave & 1), +1; dx: k1 fragment wave, all 4 row fragments
  const int kf2 = wave >> 1, mp = (wave & 1) * 2;
  const int w3off = troff + (((kf2 * 16) * 2) ^ swb);
  const bf16_t* w2img = W2t + (wave >> 3) * MLP2_IMG;                     // 8 fragments per 128-column window
  const int w2off = troff + ((((wave & 7) * 16) * 2) ^ swb);
  // whole-row pieces of this thread: h / dx rows (32 chunks each): pieces t, t + 1024; z2 / dz2 rows (16 chunks): piece t;
  // d_out rows (8 chunks): piece t of the first 512 threads.  LDS slot of chunk c of row q: q * 256 + ((c ^ q) & 15) * 16
  const int hch = t & 31;
#define MLP2_HROW(j) ((t + (j) * MLP2_THREADS) >> 5)
  const int zrow = t >> 4, zch = t & 15, drow = (t >> 3) & 63, dch = t & 7;
#define MLP2_HSLOT(j) ((hch >> 4) * (64 * 128 * 2) + MLP2_HROW(j) * 256 + (((hch & 15) ^ swz_row(MLP2_HROW(j))) << 4))
  const int zslot = zrow * 256 + ((zch ^ swz_row(zrow)) << 4), dslot = drow * 256 + ((dch ^ swz_row(drow)) << 4);

  uint4 dv = make_uint4(0, 0, 0, 0), zv, hv0, hv1;
#define MLP2_BWD_FETCH(tile_)                                                                                          \
  {                                                                                                                    \
    const int64_t base = (int64_t)(tile_) * MLP2_BM, last = N.rows - 1;                                                \
    int64_t q = base + drow; q = q < last ? q : last;                                                                  \
    if (t < 512) dv = *reinterpret_cast<const uint4*>(d + q * N.ld_dout + dch * 8);                                      \
    q = base + zrow; q = q < last ? q : last;                                                                          \
    zv = *reinterpret_cast<const uint4*>(z2 + q * N.ld_z2 + zch * 8);                                                    \
    q = base + MLP2_HROW(0); q = q < last ? q : last;                                                                  \
    hv0 = *reinterpret_cast<const uint4*>(hin + q * N.ld_h + hch * 8);                                                   \
    q = base + MLP2_HROW(1); q = q < last ? q : last;                                                                  \
    hv1 = *reinterpret_cast<const uint4*>(hin + q * N.ld_h + hch * 8);                                                   \
  }
  MLP2_BWD_FETCH(blockIdx.x);
  bool first = true;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = (int64_t)tile * MLP2_BM;
    if (t < 512) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(D3i) + dslot) = dv;
    *reinterpret_cast<uint4*>(reinterpret_cast<char*>(D2i) + zslot) = zv;
    *reinterpret_cast<uint4*>(reinterpret_cast<char*>(Hi) + MLP2_HSLOT(0)) = hv0;
    *reinterpret_cast<uint4*>(reinterpret_cast<char*>(Hi) + MLP2_HSLOT(1)) = hv1;
    if (first) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the weights
    first = false;
    __syncthreads();
    if (tile + (int)gridDim.x < tiles) MLP2_BWD_FETCH(tile + gridDim.x);
    // ---- dz2[m][k2] = (d_out W3) * elu'(z2)
    {
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kk = 0; kk < MLP2_N3 / 32; kk++) {
        const bf16x8_t w = lds_tr_operand(W3t, kk * 32 * 256 + w3off);
#pragma unroll
        for (int m = 0; m < 2; m++) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, lds_b128(D3i + (mp + m) * 16 * 128, foff[kk]), acc[m], 0, 0, 0);
      }
      const int k0 = kf2 * 16 + 4 * g;
#pragma unroll
      for (int m = 0; m < 2; m++) {
        const int row = (mp + m) * 16 + r;
        uint2* slot = reinterpret_cast<uint2*>(reinterpret_cast<char*>(D2i) + row * 256 + (((k0 >> 3) ^ swz_row(row)) << 4) + ((k0 >> 2) & 1) * 8);
        float h[4], o4[4];
        unpack_bf4(*slot, h);
#pragma unroll
        for (int e = 0; e < 4; e++) o4[e] = acc[m][e] * (h[e] > 0.f ? 1.f : h[e] + 1.f);
        *slot = pack_bf4(o4);
      }
    }
    __syncthreads();
    // ---- dx[m][k1] = (dz2 W2) * elu'(h)
    {
      f32x4 acc[4];
#pragma unroll
      for (int m = 0; m < 4; m++) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < MLP2_N2 / 32; kk++) {
        const bf16x8_t w = lds_tr_operand(w2img, kk * 32 * 256 + w2off);
#pragma unroll
        for (int m = 0; m < 4; m++) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, lds_b128(D2i + m * 16 * 128, foff[kk]), acc[m], 0, 0, 0);
      }
      const int k0 = (wave & 7) * 16 + 4 * g;                             // column inside the wave's 128-column window
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const int row = m * 16 + r;
        uint2* slot = reinterpret_cast<uint2*>(reinterpret_cast<char*>(Hi + (wave >> 3) * 64 * 128) + row * 256 +
                                               (((k0 >> 3) ^ swz_row(row)) << 4) + ((k0 >> 2) & 1) * 8);
        float h[4], o4[4];
        unpack_bf4(*slot, h);
#pragma unroll
        for (int e = 0; e < 4; e++) o4[e] = acc[m][e] * (h[e] > 0.f ? 1.f : h[e] + 1.f);
        *slot = pack_bf4(o4);
      }
    }
    __syncthreads();
    // ---- the finished tiles leave row by row
    // (written through, go1ppo.hip put16_wt; dz2 / dx may be the z2 / h buffers: a tile's rows are fetched by these same lanes, a tile ahead)
    if (row0 + zrow < N.rows) put16_wt(dz2 + (row0 + zrow) * N.ld_dz2 + zch * 8, *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(D2i) + zslot));
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (row0 + MLP2_HROW(j) < N.rows)
        put16_wt(dx + (row0 + MLP2_HROW(j)) * N.ld_dx + hch * 8, *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Hi) + MLP2_HSLOT(j)));
    __syncthreads();                                                      // before the next tile's rows overwrite D2i / Hi
  }
}

// ------------------------------------------------------------------------------------- forward + loss + backward, one launch
// A 64-row tile stays on chip from x to d_x: mlp2_fwd_kernel's stages, the loss (or the adaptation MSE) of the tile's rows with a row per
// lane, mlp2_bwd_kernel's stages — the same fragment mapping, MFMA order and roundings, so every output is bit for bit what the
// three launches write.  LDS map (153.5 KB + the ticket word):
//   W2i  64 KB  [k window][n2][128 k1]   ONE copy of W2 for the forward pass's ds_read_b128 fragments (reduction index contiguous) and the
//   W3i  16 KB  [n3][128 k2]             backward pass's ds_read_tr16_b64 fragments (reduction index = row); chunk swizzle swz_row (by row & 15):
//                                        the swizzle moves bank conflicts only (MLP2_TAIL_SWZ_RED builds the swz_red image for comparison)
//   Ai   32 KB  [k window][m][128]       x -> h = elu(x) -> dx (in the slot of the h it is multiplied by)
//   Z2i  16 KB  [m][128]                 z2 -> dz2
//   Gi  9.5 KB                           the loss's storage gathers (LDS-DMA, issued before the hidden layer through an index fetched a
//                                        tile ahead); then z[j] and the per-action terms of the policy loss, and dlogp
//   D3i  16 KB  [m][16 chunks]           chunk c < 8 of row q at slot c ^ (q & 15): d_out (the rows as they are in memory, then the loss's
//                                        columns on top); the head's chunk c at slot (c | 8) ^ (q & 15), read by the loss wave
// Sums: a wave reduces the tile's 64 rows with the __shfl_xor butterfly of block_reduce_store and stores one slab row per TILE; the last
// workgroup to arrive (det_last) adds, per column, the 256-row groups in order, each as (((0 + p[4b]) + p[4b+1]) + p[4b+2]) + p[4b+3] — the
// additions loss_kernel / mse_kernel make in their 256-thread workgroups and over their slab rows.
#ifndef MLP2_TAIL_SWZ_RED
#define MLP2_TAIL_SWZ_RED 0
#endif
#define TAIL_AMAX GO1PPO_TAIL_MAX_ACTIONS
#define DET_TAIL_MAX_TILES (4 * DET_MAX_BLOCKS)
#define DET_TAIL_PPO_W (4 + 2 * TAIL_AMAX)                      // [sur, vl, kl, dvb], dstd[TAIL_AMAX], dmb[TAIL_AMAX]
__device__ float det_tail_ppo_slab[DET_TAIL_MAX_TILES * DET_TAIL_PPO_W];
__device__ float det_tail_mse_slab[DET_TAIL_MAX_TILES * DET_MSE_W];
__device__ unsigned det_tail_count[2];                          // [0] PPO tail, [1] adaptation tail

struct Mlp2TailPpoArgs { Go1PpoMlp2Tail net[2]; Go1PpoLossArgs loss; };
struct Mlp2TailMseArgs { Go1PpoMlp2Tail net; Go1PpoMseArgs mse; };

__device__ __forceinline__ int swz_w(int row) { return MLP2_TAIL_SWZ_RED ? swz_red(row) : swz_row(row); }
__device__ __forceinline__ bf16x8_t lds_tr_operand2(const bf16_t* img, int off_lo, int off_hi) {
  typedef __attribute__((address_space(3))) s16x4_t lds_s16x4_t;
  const char* p = reinterpret_cast<const char*>(img);
  s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(p + off_lo));
  s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(p + off_hi));
  s16x8_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8_t, v);
}
#define TAIL_G0 (3 * TAIL_AMAX * 64)                             // floats of the gathered per-action values in front of the two scalars
#define TAIL_MSE_PRE 8                                           // target columns gathered ahead (the others are loaded where they are used)
__device__ __forceinline__ void glds4(const float* g, float* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((global_cvoid_t*)g, (lds_void_t*)lds_wave_base, 4, 0, 0);
}
__device__ __forceinline__ float wave_sum(float x) {            // block_reduce_store's butterfly
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// the last arriver: t[c] = sum over the 256-row groups b, in order, of (((0 + p[4b][c]) + p[4b+1][c]) + p[4b+2][c]) + p[4b+3][c] (a tile past the
// last one: 0, the wave of loss_kernel whose rows are all past the end); publish(c, t[c]) in thread c.  scratch: `floats` floats of LDS
template <typename F>
__device__ __forceinline__ void tail_sums(const float* slab, int W, int ncols, int tiles, float* scratch, int floats, F&& publish) {
  const int groups = (tiles + 3) >> 2, per = floats / ncols;
  float t = 0.f;
  for (int b0 = 0; b0 < groups; b0 += per) {
    const int nb = groups - b0 < per ? groups - b0 : per;
    for (int i = threadIdx.x; i < nb * ncols; i += MLP2_THREADS) {
      const int b = b0 + i / ncols, c = i % ncols;
      float bs = 0.f;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int tile = 4 * b + q;
        bs += tile < tiles ? slab[(int64_t)tile * W + c] : 0.f;
      }
      scratch[i] = bs;
    }
    __syncthreads();
    if ((int)threadIdx.x < ncols)
      for (int i = 0; i < nb; i++) t += scratch[i * ncols + threadIdx.x];
    __syncthreads();
  }
  if ((int)threadIdx.x < ncols) publish((int)threadIdx.x, t);
}

// MODE 0: PPO (blockIdx.y 0 = actor: the policy half of loss_sample, 1 = critic: the value half), AMAX = num_actions rounded up to 4;
// MODE 1: adaptation MSE
template <int MODE, int AMAX>
__device__ __forceinline__ void mlp2_tail_body(const Go1PpoMlp2Tail& N, const Go1PpoLossArgs& L, const Go1PpoMseArgs& Q) {
  __shared__ __attribute__((aligned(1024))) bf16_t W2i[2 * MLP2_IMG];
  __shared__ __attribute__((aligned(1024))) bf16_t W3i[64 * 128];
  __shared__ __attribute__((aligned(1024))) bf16_t Ai[2 * 64 * 128];
  __shared__ __attribute__((aligned(1024))) bf16_t Z2i[64 * 128];
  __shared__ __attribute__((aligned(1024))) bf16_t D3i[64 * 128];
  __shared__ __attribute__((aligned(16))) float Gi[TAIL_G0 + 2 * 64];
  const int tiles = (int)((N.rows + MLP2_BM - 1) / MLP2_BM);                 // gridDim.x <= tiles: every workgroup has a tile and takes a ticket
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 15, g = lane >> 4;
  dma_weights<MLP2_TAIL_SWZ_RED != 0>((const bf16_t*)N.W2, MLP2_N2, MLP2_K1, W2i, wave, lane);
  dma_weights<MLP2_TAIL_SWZ_RED != 0>((const bf16_t*)N.W3, MLP2_N3, MLP2_N2, W3i, wave, lane);
  bf16_t* x = (bf16_t*)N.x;
  bf16_t* z2 = (bf16_t*)N.z2;
  bf16_t* out = (bf16_t*)N.out;
  bf16_t* dout = (bf16_t*)N.d_out;
  bf16_t* dz2 = (bf16_t*)N.d_z2;
  bf16_t* dx = (bf16_t*)N.d_x;
  const int tx = g ^ r;
  int foff[4], woff[4];                                                      // b128 fragments: activations (swz_row), weights (swz_w)
#pragma unroll
  for (int a = 0; a < 4; a++) {
    foff[a] = r * 256 + (((4 * a) ^ tx) << 4);
    woff[a] = r * 256 + (((4 * a + g) ^ swz_w(r)) << 4);
  }
  // forward: as mlp2_fwd_kernel
  const int nf2 = wave >> 1, mp = (wave & 1) * 2, nf3 = wave & 3, m3 = wave >> 2;
  float bias2[4], bias3[4];
  unpack_bf4(*reinterpret_cast<const uint2*>((const bf16_t*)N.b2 + nf2 * 16 + 4 * g), bias2);
  unpack_bf4(*reinterpret_cast<const uint2*>((const bf16_t*)N.b3 + nf3 * 16 + 4 * g), bias3);
  // backward: as mlp2_bwd_kernel; transpose-read pieces of the weights: rows (reduction) 8g + (r >> 2) and + 4 of a 32-row slab, 8 bytes at
  // column 16 f + 4 (r & 3) = chunk 2 f + ((r & 3) >> 1), half r & 1
  const int trow = g * 8 + (r >> 2), tsub = (r & 3) >> 1, thalf = (r & 1) * 8;
  const int kf2 = wave >> 1;
  const int w3lo = trow * 256 + (((2 * kf2 + tsub) ^ swz_w(trow)) << 4) + thalf;
  const int w3hi = (trow + 4) * 256 + (((2 * kf2 + tsub) ^ swz_w(trow + 4)) << 4) + thalf;
  const bf16_t* w2img = W2i + (wave >> 3) * MLP2_IMG;
  const int w2lo = trow * 256 + (((2 * (wave & 7) + tsub) ^ swz_w(trow)) << 4) + thalf;
  const int w2hi = (trow + 4) * 256 + (((2 * (wave & 7) + tsub) ^ swz_w(trow + 4)) << 4) + thalf;
  const int hch = t & 31;
  const int zrow = t >> 4, zch = t & 15, drow = (t >> 3) & 63, dch = t & 7;
  const int zslot = zrow * 256 + ((zch ^ swz_row(zrow)) << 4), dslot = drow * 256 + ((dch ^ swz_row(drow)) << 4);
  // the loss wave: lane = row of the tile
  const bool lw = wave == 0;
  const int lrow = lane * 256, lsw = lane & 15;
  const bool actor = MODE == 0 && blockIdx.y == 0;
  const int A = MODE == 0 ? L.num_actions : 0;
  const bool vec4 = MODE == 0 && (A & 3) == 0 && ((reinterpret_cast<uintptr_t>(L.actions) | reinterpret_cast<uintptr_t>(L.old_mu) |
                                                  reinterpret_cast<uintptr_t>(L.old_sigma)) & 15) == 0;
  const int64_t* idx = MODE == 0 ? L.idx : Q.idx;
  const int ncol = MODE == 1 ? (Q.selective ? 1 : Q.npv) : 0;
  float* slab = MODE == 0 ? det_tail_ppo_slab : det_tail_mse_slab;
  const int slabw = MODE == 0 ? DET_TAIL_PPO_W : DET_MSE_W;

  Bf8 v[2];
  uint4 dv = make_uint4(0, 0, 0, 0);
  int64_t s = 0;
  auto fetch = [&](int tile) {
    const int64_t base = (int64_t)tile * MLP2_BM, last = N.rows - 1;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int p = t + MLP2_THREADS * j, row = p >> 5, ch = p & 31;
      int64_t grow = base + row;
      grow = grow < N.rows ? grow : last;
      v[j] = *reinterpret_cast<const Bf8*>(x + grow * N.ld_x + ch * 8);
    }
    int64_t q = base + drow;
    q = q < last ? q : last;
    if (t < 512) dv = *reinterpret_cast<const uint4*>(dout + q * N.ld_dout + dch * 8);
    q = base + lane;
    q = q < last ? q : last;
    if (lw) s = idx[q];
  };
  fetch(blockIdx.x);
  bool first = true;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row0 = (int64_t)tile * MLP2_BM;
    const bool on = row0 + lane < N.rows;
    // ---- input rows: ELU, write-back, swizzled LDS image; d_out rows as they are
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int p = t + MLP2_THREADS * j, row = p >> 5, ch = p & 31;
      if (N.elu_input) {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; e++) f[e] = elu1(bf2f(v[j].v[e]));
        v[j] = pack_bf8(f);
        if (row0 + row < N.rows) *reinterpret_cast<Bf8*>(x + (row0 + row) * N.ld_x + ch * 8) = v[j];
      }
      *reinterpret_cast<Bf8*>(reinterpret_cast<char*>(Ai + (ch >> 4) * 64 * 128) + row * 256 + (((ch & 15) ^ swz_row(row)) << 4)) = v[j];
    }
    if (t < 512) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(D3i) + dslot) = dv;
    // ---- the loss wave's storage gathers, in flight during the layers: global -> LDS past the registers (a lane's 16 or 4 bytes land at
    //      slot + lane * size); Gi: [actions | old_mu | old_sigma][chunk][lane][4] (16-byte gathers) or [..][action][lane], then two scalars
    if (lw) {
      if (MODE == 0 && actor) {
        if (vec4) {
#pragma unroll
          for (int j = 0; j < AMAX; j += 4) {
            if (j < A) {
              glds16((const bf16_t*)(L.actions + s * A + j), (bf16_t*)(Gi + (j >> 2) * 256));
              glds16((const bf16_t*)(L.old_mu + s * A + j), (bf16_t*)(Gi + (3 + (j >> 2)) * 256));
              glds16((const bf16_t*)(L.old_sigma + s * A + j), (bf16_t*)(Gi + (6 + (j >> 2)) * 256));
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < AMAX; j++) {
            if (j < A) {
              glds4(L.actions + s * A + j, Gi + j * 64);
              glds4(L.old_mu + s * A + j, Gi + (TAIL_AMAX + j) * 64);
              glds4(L.old_sigma + s * A + j, Gi + (2 * TAIL_AMAX + j) * 64);
            }
          }
        }
        glds4(L.advantages + s, Gi + TAIL_G0);
        glds4(L.old_logp + s, Gi + TAIL_G0 + 64);
      } else if (MODE == 0) {
        glds4(L.returns + s, Gi + TAIL_G0);
        if (L.use_clipped_value_loss) glds4(L.old_values + s, Gi + TAIL_G0 + 64);
      } else {
#pragma unroll
        for (int j = 0; j < TAIL_MSE_PRE; j++)
          if (j < ncol) glds4(Q.target + s * Q.npv + j, Gi + j * 64);
      }
    }
    const int64_t s_cur = s;
    if (first) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the weights
    first = false;
    __syncthreads();
    if (tile + (int)gridDim.x < tiles) fetch(tile + gridDim.x);
    // ---- hidden layer
    {
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ks = 0; ks < MLP2_K1 / 32; ks++) {
        const int win = ks >> 2;
        const bf16x8_t w = lds_b128(W2i + win * MLP2_IMG + nf2 * 16 * 128, woff[ks & 3]);
#pragma unroll
        for (int m = 0; m < 2; m++)
          acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, lds_b128(Ai + win * 64 * 128 + (mp + m) * 16 * 128, foff[ks & 3]), acc[m], 0, 0, 0);
      }
      const int n0 = nf2 * 16 + 4 * g;
#pragma unroll
      for (int m = 0; m < 2; m++) {
        const int row = (mp + m) * 16 + r;
        float o4[4];
#pragma unroll
        for (int e = 0; e < 4; e++) o4[e] = elu1(acc[m][e] + bias2[e]);
        const uint2 o = pack_bf4(o4);
        if (row0 + row < N.rows) *reinterpret_cast<uint2*>(z2 + (row0 + row) * N.ld_z2 + n0) = o;
        *reinterpret_cast<uint2*>(reinterpret_cast<char*>(Z2i) + row * 256 + (((n0 >> 3) ^ swz_row(row)) << 4) + ((n0 >> 2) & 1) * 8) = o;
      }
    }
    __syncthreads();
    // ---- head: to memory and beside d_out for the loss wave
    {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < MLP2_N2 / 32; ks++)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_b128(W3i + nf3 * 16 * 128, woff[ks]), lds_b128(Z2i + m3 * 16 * 128, foff[ks]), acc, 0, 0, 0);
      const int n0 = nf3 * 16 + 4 * g, row = m3 * 16 + r;
      float o4[4];
#pragma unroll
      for (int e = 0; e < 4; e++) o4[e] = acc[e] + bias3[e];
      const uint2 o = pack_bf4(o4);
      if (row0 + row < N.rows) *reinterpret_cast<uint2*>(out + (row0 + row) * N.ld_out + n0) = o;
      *reinterpret_cast<uint2*>(reinterpret_cast<char*>(D3i) + row * 256 + ((((n0 >> 3) | 8) ^ swz_row(row)) << 4) + ((n0 >> 2) & 1) * 8) = o;
    }
    if (lw) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the loss wave's gathers have landed in Gi (every wave reads them)
    __syncthreads();
    // ---- loss; d_out's columns to memory and to D3i, the 64-row sums to the tile's slab row.  Critic and adaptation MSE: one wave, a row per
    //      lane.  Policy: a row per lane as well, but its 12 actions are 12 chains of two logarithms and three divisions, and 26 butterflies:
    //      on one wave that is ~10 us per tile with 15 waves waiting.  The per-action terms go to wave j = action (the terms are the same
    //      numbers whoever computes them); wave 0 then adds them IN loss_sample's ORDER and finishes the row; wave j makes the gradient
    //      column j and its two sums.
    // (bit for bit: where loss_kernel / mse_kernel contract a product into the addition behind it is the compiler's choice there, and another
    //  one here, in other surroundings; so these blocks are compiled without contraction and spell out the fused multiply-adds those two
    //  kernels are built with — tests/test_gpu_ppo_tail_fused.py holds the two forms together)
    auto gat = [&](int which, int j) -> float& { return vec4 ? Gi[(which * 3 + (j >> 2)) * 256 + lane * 4 + (j & 3)] : Gi[(which * TAIL_AMAX + j) * 64 + lane]; };
    if (MODE == 0 && actor) {
#pragma clang fp contract(off)
      // the policy half of loss_sample, its expressions as they stand.  Every lane computes (a lane past the last row on the last row's
      // inputs); only a lane with a row contributes.  z[j] and the two terms of action j wait in the LDS slots of its three gathers.
      const Go1PpoLossArgs& a = L;
      char* d3 = reinterpret_cast<char*>(D3i) + lrow;
      float* prow = slab + (int64_t)tile * slabw;
      const float invM = 1.f / (float)a.rows;
      const float HALF_LOG_2PI = 0.9189385332046727f;
      const int j = wave;
      if (j < A) {
        const float mu = bf2f(*reinterpret_cast<const bf16_t*>(d3 + ((((j >> 3) | 8) ^ lsw) << 4) + (j & 7) * 2));
        float sg = a.std[j];
        float isg = 1.f / sg;
        const float zj = (gat(0, j) - mu) * isg;
        float so = gat(2, j), dm = gat(1, j) - mu;
        gat(0, j) = zj;
        gat(1, j) = fmaf(-0.5f * zj, zj, -logf(sg)) - HALF_LOG_2PI;
        gat(2, j) = logf(sg / so + 1.e-5f) + fmaf(dm, dm, so * so) / (2.f * sg * sg) - 0.5f;
      }
      __syncthreads();
      if (lw) {
        float logp = 0.f, kl = 0.f;
        for (int q = 0; q < A; q++) {
          logp += gat(1, q);
          kl += gat(2, q);
        }
        float adv = Gi[TAIL_G0 + lane];
        float ratio = expf(logp - Gi[TAIL_G0 + 64 + lane]);
        float lo = 1.f - a.clip_param, hi = 1.f + a.clip_param;
        float rc = fminf(fmaxf(ratio, lo), hi);
        float s1 = -adv * ratio, s2 = -adv * rc;
        float sur = fmaxf(s1, s2) * invM;
        float dratio = (ratio >= lo && ratio <= hi) ? -adv : (s1 > s2 ? -adv : 0.f);
        float dlogp = dratio * ratio * invM;
        kl *= invM;
        Gi[TAIL_G0 + lane] = dlogp;
        sur = wave_sum(on ? sur : 0.f);
        kl = wave_sum(on ? kl : 0.f);
        if (lane == 0) { det_put(prow, sur); det_put(prow + 2, kl); }
      }
      __syncthreads();
      if (j < A) {
        const float dlogp = Gi[TAIL_G0 + lane];
        const float isg = 1.f / a.std[j], zj = gat(0, j);
        const bf16_t gq = f2bf(dlogp * zj * isg);
        if (on) *reinterpret_cast<bf16_t*>(d3 + (((j >> 3) ^ lsw) << 4) + (j & 7) * 2) = gq;      // to memory with the row, below
        float dmb = bf2f(gq);
        float dstd = dlogp * fmaf(zj, zj, -1.f) * isg;
        dstd = wave_sum(on ? dstd : 0.f);
        dmb = wave_sum(on ? dmb : 0.f);
        if (lane == 0) { det_put(prow + 4 + j, dstd); det_put(prow + 4 + TAIL_AMAX + j, dmb); }
      }
    } else if (lw) {
#pragma clang fp contract(off)
      char* d3 = reinterpret_cast<char*>(D3i) + lrow;
      const int64_t rr = row0 + lane;
      float* prow = slab + (int64_t)tile * slabw;
      const float g0 = Gi[TAIL_G0 + lane], g1 = Gi[TAIL_G0 + 64 + lane];     // critic: return, old value
      if (MODE == 0) {
        // the value half of loss_sample
        const Go1PpoLossArgs& a = L;
        const float invM = 1.f / (float)a.rows;
        float vl = 0.f, dvb = 0.f;
        if (on) {
          float v = bf2f(*reinterpret_cast<const bf16_t*>(d3 + ((8 ^ lsw) << 4)));
          float R = g0, dval;
          if (a.use_clipped_value_loss) {
            float vo = g1;
            float dlt = v - vo;
            float vc = vo + fminf(fmaxf(dlt, -a.clip_param), a.clip_param);
            float l1 = (v - R) * (v - R), l2 = (vc - R) * (vc - R);
            vl = fmaxf(l1, l2) * invM;
            bool inside = dlt >= -a.clip_param && dlt <= a.clip_param;
            dval = inside ? 2.f * (v - R) : (l1 > l2 ? 2.f * (v - R) : 0.f);
          } else {
            vl = (R - v) * (R - v) * invM;
            dval = 2.f * (v - R);
          }
          bf16_t gv = f2bf(a.value_loss_coef * dval * invM);
          dout[rr * N.ld_dout] = gv;
          *reinterpret_cast<bf16_t*>(d3 + (lsw << 4)) = gv;
          dvb = bf2f(gv);
        }
        vl = wave_sum(vl);
        dvb = wave_sum(dvb);
        if (lane == 0) { det_put(prow + 1, vl); det_put(prow + 3, dvb); }
      } else {
        // mse_kernel's arithmetic
        const int npv = Q.npv;
        const int64_t rows = N.rows, num_train = Q.num_train;
        float ltrain = 0.f, ltest = 0.f;
        float inv_train = 1.f / ((float)num_train * ncol), inv_test = 1.f / ((float)(rows - num_train) * ncol);
        bf16_t* d_pred = dout + rr * N.ld_dout;
        for (int j = 0; j < ncol; j++) {
          float vj = 0.f;
          if (on) {
            const float tj = j < TAIL_MSE_PRE ? Gi[j * 64 + lane] : Q.target[s_cur * npv + j];
            float e = bf2f(*reinterpret_cast<const bf16_t*>(d3 + ((((j >> 3) | 8) ^ lsw) << 4) + (j & 7) * 2)) - tj;
            bf16_t gj = 0;
            if (rr < num_train) {
              ltrain = fmaf(e * e, inv_train, ltrain);
              gj = f2bf(2.f * e * inv_train);
              vj = bf2f(gj);
            } else {
              ltest = fmaf(e * e, inv_test, ltest);
            }
            d_pred[j] = gj;
            *reinterpret_cast<bf16_t*>(d3 + (((j >> 3) ^ lsw) << 4) + (j & 7) * 2) = gj;
          }
          vj = wave_sum(vj);
          if (lane == 0) det_put(prow + j, vj);
        }
        ltrain = wave_sum(ltrain);
        ltest = wave_sum(ltest);
        if (lane == 0) { det_put(prow + ncol, ltrain); det_put(prow + ncol + 1, ltest); }
        if (Q.selective && on)                                               // columns the selective loss ignores carry no gradient
          for (int j = 1; j < npv; j++) {
            d_pred[j] = 0;
            *reinterpret_cast<bf16_t*>(d3 + (((j >> 3) ^ lsw) << 4) + (j & 7) * 2) = 0;
          }
      }
    }
    __syncthreads();
    // (the policy gradient's rows: the loss's columns with the others as they were read, so the bytes in memory are the three launches')
    if (MODE == 0 && actor && t < 512 && row0 + drow < N.rows)
      *reinterpret_cast<uint4*>(dout + (row0 + drow) * N.ld_dout + dch * 8) = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(D3i) + dslot);
    // ---- dz2[m][k2] = (d_out W3) * elu'(z2)
    {
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kk = 0; kk < MLP2_N3 / 32; kk++) {
        const bf16x8_t w = lds_tr_operand2(W3i, kk * 32 * 256 + w3lo, kk * 32 * 256 + w3hi);
#pragma unroll
        for (int m = 0; m < 2; m++) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, lds_b128(D3i + (mp + m) * 16 * 128, foff[kk]), acc[m], 0, 0, 0);
      }
      const int k0 = kf2 * 16 + 4 * g;
#pragma unroll
      for (int m = 0; m < 2; m++) {
        const int row = (mp + m) * 16 + r;
        uint2* slot = reinterpret_cast<uint2*>(reinterpret_cast<char*>(Z2i) + row * 256 + (((k0 >> 3) ^ swz_row(row)) << 4) + ((k0 >> 2) & 1) * 8);
        float h[4], o4[4];
        unpack_bf4(*slot, h);
#pragma unroll
        for (int e = 0; e < 4; e++) o4[e] = acc[m][e] * (h[e] > 0.f ? 1.f : h[e] + 1.f);
        *slot = pack_bf4(o4);
      }
    }
    __syncthreads();
    // ---- dx[m][k1] = (dz2 W2) * elu'(h)
    {
      f32x4 acc[4];
#pragma unroll
      for (int m = 0; m < 4; m++) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < MLP2_N2 / 32; kk++) {
        const bf16x8_t w = lds_tr_operand2(w2img, kk * 32 * 256 + w2lo, kk * 32 * 256 + w2hi);
#pragma unroll
        for (int m = 0; m < 4; m++) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, lds_b128(Z2i + m * 16 * 128, foff[kk]), acc[m], 0, 0, 0);
      }
      const int k0 = (wave & 7) * 16 + 4 * g;
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const int row = m * 16 + r;
        uint2* slot = reinterpret_cast<uint2*>(reinterpret_cast<char*>(Ai + (wave >> 3) * 64 * 128) + row * 256 +
                                               (((k0 >> 3) ^ swz_row(row)) << 4) + ((k0 >> 2) & 1) * 8);
        float h[4], o4[4];
        unpack_bf4(*slot, h);
#pragma unroll
        for (int e = 0; e < 4; e++) o4[e] = acc[m][e] * (h[e] > 0.f ? 1.f : h[e] + 1.f);
        *slot = pack_bf4(o4);
      }
    }
    __syncthreads();
    // ---- the finished tiles leave row by row, written through
    if (row0 + zrow < N.rows) put16_wt(dz2 + (row0 + zrow) * N.ld_dz2 + zch * 8, *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Z2i) + zslot));
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (row0 + MLP2_HROW(j) < N.rows)
        put16_wt(dx + (row0 + MLP2_HROW(j)) * N.ld_dx + hch * 8, *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Ai) + MLP2_HSLOT(j)));
    __syncthreads();                                                        // before the next tile's rows overwrite Ai / D3i
  }
  // ---- the sums: the ticket protocol as it stands
  if (!det_last(&det_tail_count[MODE], gridDim.x * gridDim.y)) return;
  float* scratch = reinterpret_cast<float*>(Ai);
  if (MODE == 0) {
    const Go1PpoLossArgs& a = L;
    tail_sums(slab, slabw, DET_TAIL_PPO_W, tiles, scratch, 2 * 64 * 128 / 2, [&](int c, float tsum) {
      const int j = c < 4 ? 0 : (c - 4) % TAIL_AMAX;
      if (c >= 4 && j >= A) return;
      float* dst = c < 4 ? (c == 0 ? a.surrogate_loss : c == 1 ? a.value_loss : c == 2 ? a.kl : a.d_value_bias)
                         : c < 4 + TAIL_AMAX ? (a.d_std ? a.d_std + j : nullptr) : (a.d_mean_bias ? a.d_mean_bias + j : nullptr);
      if (!dst) return;
      float sres = *dst + tsum;
      // entropy term: loss -= entropy_coef * (sum log sigma + const)  ->  d/d sigma_j = -entropy_coef / sigma_j  (once)
      if (c >= 4 && c < 4 + TAIL_AMAX) sres += -a.entropy_coef / a.std[j];
      *dst = sres;
    });
  } else {
    tail_sums(slab, slabw, ncol + 2, tiles, scratch, 2 * 64 * 128 / 2, [&](int c, float tsum) {
      float* dst = c < ncol ? (Q.d_pred_bias ? Q.d_pred_bias + c : nullptr) : c == ncol ? Q.train_loss : Q.test_loss;
      if (dst) *dst += tsum;
    });
  }
}

template <int AMAX>
__global__ __launch_bounds__(MLP2_THREADS, 1) void mlp2_tail_ppo_kernel(Mlp2TailPpoArgs A) {
  mlp2_tail_body<0, AMAX>(A.net[blockIdx.y], A.loss, Go1PpoMseArgs{});
}
__global__ __launch_bounds__(MLP2_THREADS, 1) void mlp2_tail_mse_kernel(Mlp2TailMseArgs A) {
  mlp2_tail_body<1, 4>(A.net, Go1PpoLossArgs{}, A.mse);
}

static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

extern "C" int go1ppo_mlp2_fwd(const Go1PpoMlp2Fwd* nets, int count, void* stream) {
  if (!nets || count <= 0 || count > GO1PPO_MLP2_MAX_NETS) return -1;
  Mlp2FwdArgs A;
  int64_t max_rows = 0;
  for (int i = 0; i < count; i++) {
    const Go1PpoMlp2Fwd& N = nets[i];
    if (!N.x || !N.W2 || !N.b2 || !N.W3 || !N.b3 || !N.z2 || !N.out || N.rows <= 0) return -1;
    if ((N.ld_x & 7) || (N.ld_z2 & 3) || (N.ld_out & 3) || N.ld_x < MLP2_K1 || N.ld_z2 < MLP2_N2 || N.ld_out < MLP2_N3 || !aligned16(N.x) ||
        !aligned16(N.W2) || !aligned16(N.W3) || !aligned8(N.b2) || !aligned8(N.b3) || !aligned8(N.z2) || !aligned8(N.out))
      return -2;
    A.net[i] = N;
    if (N.rows > max_rows) max_rows = N.rows;
  }
  int64_t wgs = (max_rows + MLP2_BM - 1) / MLP2_BM;                       // one workgroup per CU (the weights take 80 KB of
  if (wgs > 256 / count) wgs = 256 / count;                               // its LDS), each walking over its row tiles
  mlp2_fwd_kernel<<<dim3((unsigned)wgs, count), dim3(MLP2_THREADS), 0, (hipStream_t)stream>>>(A);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

extern "C" int go1ppo_mlp2_bwd(const Go1PpoMlp2Bwd* nets, int count, void* stream) {
  if (!nets || count <= 0 || count > GO1PPO_MLP2_MAX_NETS) return -1;
  Mlp2BwdArgs A;
  int64_t max_rows = 0;
  for (int i = 0; i < count; i++) {
    const Go1PpoMlp2Bwd& N = nets[i];
    if (!N.d_out || !N.z2 || !N.h || !N.W2 || !N.W3 || !N.d_z2 || !N.d_x || N.rows <= 0) return -1;
    if ((N.ld_dout & 7) || (N.ld_z2 & 7) || (N.ld_h & 7) || (N.ld_dz2 & 7) || (N.ld_dx & 7) || N.ld_dout < MLP2_N3 || N.ld_z2 < MLP2_N2 ||
        N.ld_h < MLP2_K1 || N.ld_dz2 < MLP2_N2 || N.ld_dx < MLP2_K1 || !aligned16(N.d_out) || !aligned16(N.W2) || !aligned16(N.W3) ||
        !aligned16(N.z2) || !aligned16(N.h) || !aligned16(N.d_z2) || !aligned16(N.d_x))
      return -2;
    A.net[i] = N;
    if (N.rows > max_rows) max_rows = N.rows;
  }
  int64_t wgs = (max_rows + MLP2_BM - 1) / MLP2_BM;
  if (wgs > 256 / count) wgs = 256 / count;
  mlp2_bwd_kernel<<<dim3((unsigned)wgs, count), dim3(MLP2_THREADS), 0, (hipStream_t)stream>>>(A);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

// leading dimensions and alignment of one net of a fused launch (the union of go1ppo_mlp2_fwd's and go1ppo_mlp2_bwd's conditions; the head
// and its gradient in 64-column rows, as the LDS tile holds them)
static int mlp2_tail_check(const Go1PpoMlp2Tail& N) {
  if (!N.x || !N.W2 || !N.b2 || !N.W3 || !N.b3 || !N.z2 || !N.out || !N.d_out || !N.d_z2 || !N.d_x || N.rows <= 0) return -1;
  if ((N.rows + MLP2_BM - 1) / MLP2_BM > DET_TAIL_MAX_TILES) return -1;      // one slab row per tile
  return 0;
}
static int mlp2_tail_check_shape(const Go1PpoMlp2Tail& N) {
  if ((N.ld_x & 7) || (N.ld_z2 & 7) || (N.ld_dz2 & 7) || (N.ld_dx & 7) || N.ld_x < MLP2_K1 || N.ld_z2 < MLP2_N2 || N.ld_dz2 < MLP2_N2 ||
      N.ld_dx < MLP2_K1 || N.ld_out != MLP2_N3 || N.ld_dout != MLP2_N3 || !aligned16(N.x) || !aligned16(N.W2) || !aligned16(N.W3) ||
      !aligned8(N.b2) || !aligned8(N.b3) || !aligned16(N.z2) || !aligned16(N.out) || !aligned16(N.d_out) || !aligned16(N.d_z2) ||
      !aligned16(N.d_x) || N.d_z2 == N.z2 || N.d_x == N.x)
    return -2;
  return 0;
}

extern "C" int go1ppo_mlp2_tail_ppo(const Go1PpoMlp2Tail* nets, const Go1PpoLossArgs* loss, void* stream) {
  if (!nets || !loss) return -1;
  for (int i = 0; i < 2; i++)
    if (mlp2_tail_check(nets[i])) return -1;
  const Go1PpoLossArgs& a = *loss;
  if (!a.std || !a.idx || !a.actions || !a.old_mu || !a.old_sigma || !a.old_logp || !a.advantages || !a.returns ||
      (a.use_clipped_value_loss && !a.old_values) || a.rows <= 0 || a.num_actions <= 0 || a.num_actions > GO1PPO_TAIL_MAX_ACTIONS)
    return -1;
  for (int i = 0; i < 2; i++)
    if (mlp2_tail_check_shape(nets[i])) return -2;
  if (a.head_ld != MLP2_N3 || a.rows != nets[0].rows || a.rows != nets[1].rows || a.mean != nets[0].out || a.value != nets[1].out ||
      a.d_mean != nets[0].d_out || a.d_value != nets[1].d_out)
    return -2;
  Mlp2TailPpoArgs A;
  A.net[0] = nets[0];
  A.net[1] = nets[1];
  A.loss = a;
  int64_t wgs = (a.rows + MLP2_BM - 1) / MLP2_BM;                            // one workgroup per CU, half of them per net
  if (wgs > 128) wgs = 128;
  const dim3 grid((unsigned)wgs, 2), block(MLP2_THREADS);
  if (a.num_actions <= 4) mlp2_tail_ppo_kernel<4><<<grid, block, 0, (hipStream_t)stream>>>(A);
  else if (a.num_actions <= 8) mlp2_tail_ppo_kernel<8><<<grid, block, 0, (hipStream_t)stream>>>(A);
  else mlp2_tail_ppo_kernel<12><<<grid, block, 0, (hipStream_t)stream>>>(A);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}

extern "C" int go1ppo_mlp2_tail_mse(const Go1PpoMlp2Tail* net, const Go1PpoMseArgs* mse, void* stream) {
  if (!net || !mse) return -1;
  if (mlp2_tail_check(*net)) return -1;
  if (!mse->target || !mse->idx || !mse->train_loss || !mse->test_loss || mse->num_train <= 0 || mse->num_train >= net->rows || mse->npv <= 0 ||
      mse->npv > GO1PPO_HEAD)
    return -1;
  if (mlp2_tail_check_shape(*net)) return -2;
  Mlp2TailMseArgs A;
  A.net = *net;
  A.mse = *mse;
  int64_t wgs = (net->rows + MLP2_BM - 1) / MLP2_BM;
  if (wgs > 256) wgs = 256;
  mlp2_tail_mse_kernel<<<dim3((unsigned)wgs), dim3(MLP2_THREADS), 0, (hipStream_t)stream>>>(A);
  return hipGetLastError() == hipSuccess ? 0 : -9;
}
