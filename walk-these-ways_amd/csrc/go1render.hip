// go1render.hip — headless ray caster of one Go1 environment (include/go1render.h), gfx950.
//
// Scene: the collision geometry the physics uses (csrc/go1_model_data.h) — trunk box, 4 hip capsules, 4 thigh boxes, 4 calf
// boxes, 4 foot spheres — placed by forward kinematics from root_states / dof_pos exactly as go1_physics.h places them, over
// the terrain the physics samples: the plane z = 0, or the bilinear surface of the int16 height samples with the simulator's
// `(x + border) / hscale` cell convention (go1_physics.h terrain_fetch / terrain_eval).  The 'trimesh' instance's vertical
// faces (include/go1sim.h hf_wall_units) are not drawn as walls: they appear as the one-cell steep patch the field already
// has between the two sample rows (the physics lowers that cell's surface; the picture keeps the samples' interpolation).
// Outside the sampled area there is no ground: such rays show the sky.  Only the recorded environment's robot is drawn
// (Isaac Gym draws every actor in view; the neighbours are left out here).
//
// Layout: one thread per pixel, workgroups of 64 x 4 pixels, so a wavefront's 64 RGBA stores are one contiguous 256-byte run
// of a row; blockIdx.z = camera.  The 17 body transforms are computed once per workgroup (4 lanes, one leg each) into LDS.
// Shading: Lambert with one fixed directional light plus an ambient term, a fixed per-part palette, a 1 m checker on the
// ground, a flat sky.  tests/render_ref.py restates all of it in fp64 numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GO1_CONST static __device__ __constant__ const
#define GO1_REAL float
#include "../../include/go1render.h"
#include "go1_math.h"
#include "go1_model_data.h"

namespace {

constexpr int TILE_X = 64, TILE_Y = 4;
constexpr float TAN_HALF_FOV = 1.0f;                              // horizontal FOV 90 degrees
constexpr float ROBOT_BOUND = 0.8f;                               // every primitive lies within this radius of the base origin
// light direction (unit, towards the light) and the two shading weights
__device__ __constant__ const float LIGHT[3] = {0.36f, -0.48f, 0.8f};
constexpr float AMBIENT = 0.35f, DIFFUSE = 0.65f;
// palette: sky, ground (light / dark checker square), trunk, hip, thigh, calf, foot
__device__ __constant__ const float SKY[3] = {0.62f, 0.75f, 0.90f};
__device__ __constant__ const float GROUND[2][3] = {{0.80f, 0.80f, 0.78f}, {0.55f, 0.56f, 0.55f}};
__device__ __constant__ const float PART[5][3] = {{0.85f, 0.55f, 0.15f}, {0.25f, 0.25f, 0.28f}, {0.35f, 0.45f, 0.75f},
                                                  {0.30f, 0.30f, 0.32f}, {0.10f, 0.10f, 0.10f}};

struct Body { float R[9]; float p[3]; };          // rotation (columns) and origin relative to the base origin, world axes
DEV M3 body_R(const Body& b) { M3 R; R.c0 = v3(b.R[0], b.R[1], b.R[2]); R.c1 = v3(b.R[3], b.R[4], b.R[5]); R.c2 = v3(b.R[6], b.R[7], b.R[8]); return R; }
DEV void put_body(Body& b, const M3& R, V3 p) {
  b.R[0] = R.c0.x; b.R[1] = R.c0.y; b.R[2] = R.c0.z; b.R[3] = R.c1.x; b.R[4] = R.c1.y; b.R[5] = R.c1.z;
  b.R[6] = R.c2.x; b.R[7] = R.c2.y; b.R[8] = R.c2.z; b.p[0] = p.x; b.p[1] = p.y; b.p[2] = p.z;
}
DEV V3 tab3(const float (*t)[3], int i) { return v3(t[i][0], t[i][1], t[i][2]); }

// forward kinematics of one leg (go1_physics.h foot_state): hip about x, thigh and calf about y; the foot is the calf frame
// moved to GO1_FOOT_OFFSET.  Lane `leg` of the workgroup writes bodies 1 + 4 leg .. 4 + 4 leg, lane 0 also the base.
DEV void leg_fk(const float* root, const float* dof, int N, int env, int leg, Body* bodies) {
  const M3 R0 = quat_to_mat(root[3 * N + env], root[4 * N + env], root[5 * N + env], root[6 * N + env]);
  if (leg == 0) put_body(bodies[0], R0, v3(0.f, 0.f, 0.f));
  M3 R = R0;
  V3 p = v3(0.f, 0.f, 0.f);
  for (int j = 0; j < 3; j++) {
    const int ji = 3 * leg + j;
    p = p + mul(R, tab3(GO1_JOINT_ORIGIN, ji));
    float sn, cs;
    sincosf(dof[ji * N + env], &sn, &cs);
    R = (j == 0) ? rot_x(R, sn, cs) : rot_y(R, sn, cs);
    put_body(bodies[1 + 4 * leg + j], R, p);
  }
  put_body(bodies[4 + 4 * leg], R, p + mul(R, tab3(GO1_FOOT_OFFSET, leg)));
}

// ---- primitives: nearest hit t in (0, tbest) with its world normal ---------------------------------------------------------
DEV void hit_box(const Body& b, V3 c_local, const float* half, V3 o, V3 d, float& tbest, V3& nbest, int id, int& idbest) {
  const M3 R = body_R(b);
  const V3 c = v3(b.p[0], b.p[1], b.p[2]) + mul(R, c_local);
  const V3 ol = mulT(R, o - c), dl = mulT(R, d);
  const float oo[3] = {ol.x, ol.y, ol.z}, dd[3] = {dl.x, dl.y, dl.z};
  float tn = -1e30f, tf = 1e30f;
  int ax = 0;
  for (int k = 0; k < 3; k++) {
    if (fabsf(dd[k]) < 1e-12f) {
      if (fabsf(oo[k]) > half[k]) return;
      continue;
    }
    const float inv = 1.f / dd[k];
    float t1 = (-half[k] - oo[k]) * inv, t2 = (half[k] - oo[k]) * inv;
    if (t1 > t2) { const float s = t1; t1 = t2; t2 = s; }
    if (t1 > tn) { tn = t1; ax = k; }
    tf = fminf(tf, t2);
  }
  if (tn > tf || tn <= 0.f || tn >= tbest) return;
  tbest = tn; idbest = id;
  const float s = dd[ax] > 0.f ? -1.f : 1.f;
  nbest = s * (ax == 0 ? R.c0 : ax == 1 ? R.c1 : R.c2);
}

DEV void hit_sphere(V3 c, float r, V3 o, V3 d, float& tbest, V3& nbest, int id, int& idbest) {
  const V3 oc = o - c;
  const float b = dot(oc, d), cc = dot(oc, oc) - r * r, h = b * b - cc;
  if (h < 0.f) return;
  const float t = -b - sqrtf(h);
  if (t <= 0.f || t >= tbest) return;
  tbest = t; idbest = id;
  nbest = (1.f / r) * (o + t * d - c);
}

// capsule = segment a..b swept by radius r
DEV void hit_capsule(V3 a, V3 b, float r, V3 o, V3 d, float& tbest, V3& nbest, int id, int& idbest) {
  const V3 ba = b - a, oa = o - a;
  const float baba = dot(ba, ba), bard = dot(ba, d), baoa = dot(ba, oa), rdoa = dot(d, oa), oaoa = dot(oa, oa);
  float t = -1.f;
  const float A = baba - bard * bard;
  if (A > 1e-12f * baba) {                         // the cylinder, unless the ray runs along the axis
    const float B = baba * rdoa - baoa * bard, C = baba * oaoa - baoa * baoa - r * r * baba;
    const float h = B * B - A * C;
    if (h >= 0.f) {
      const float tc = (-B - sqrtf(h)) / A, y = baoa + tc * bard;
      if (y > 0.f && y < baba) t = tc;
    }
  }
  if (t < 0.f) {                                   // the two end spheres
    float ts = 1e30f;
    V3 ns;
    int is = -1;
    hit_sphere(a, r, o, d, ts, ns, 0, is);
    hit_sphere(b, r, o, d, ts, ns, 0, is);
    if (is < 0) return;
    t = ts;
  }
  if (t <= 0.f || t >= tbest) return;
  tbest = t; idbest = id;
  const V3 pa = o + t * d - a;
  const float s = fminf(fmaxf(dot(pa, ba) / baba, 0.f), 1.f);
  nbest = (1.f / r) * (pa - s * ba);
}

// the 17 primitives, in body order: ids 3 + body (trunk 3, then per leg hip, thigh, calf, foot)
DEV void hit_robot(const Body* bodies, V3 o, V3 d, float& tbest, V3& nbest, int& idbest) {
  { const float b = dot(o, d), h = b * b - (dot(o, o) - ROBOT_BOUND * ROBOT_BOUND); if (h < 0.f || -b + sqrtf(h) <= 0.f) return; }
  hit_box(bodies[0], v3(0.f, 0.f, 0.f), GO1_TRUNK_BOX_HALF, o, d, tbest, nbest, 3, idbest);
  for (int leg = 0; leg < 4; leg++) {
    const Body& hip = bodies[1 + 4 * leg];
    const M3 Rh = body_R(hip);
    const V3 hc = v3(hip.p[0], hip.p[1], hip.p[2]) + mul(Rh, tab3(GO1_HIP_CAPSULE_CENTER, leg));
    const V3 ax = (float)GO1_HIP_CAPSULE_HALF * Rh.c1;
    hit_capsule(hc - ax, hc + ax, (float)GO1_HIP_CAPSULE_RADIUS, o, d, tbest, nbest, 4 + 4 * leg, idbest);
    hit_box(bodies[2 + 4 * leg], v3(GO1_THIGH_BOX_CENTER[0], GO1_THIGH_BOX_CENTER[1], GO1_THIGH_BOX_CENTER[2]), GO1_THIGH_BOX_HALF,
            o, d, tbest, nbest, 5 + 4 * leg, idbest);
    hit_box(bodies[3 + 4 * leg], v3(GO1_CALF_BOX_CENTER[0], GO1_CALF_BOX_CENTER[1], GO1_CALF_BOX_CENTER[2]), GO1_CALF_BOX_HALF,
            o, d, tbest, nbest, 6 + 4 * leg, idbest);
    const Body& ft = bodies[4 + 4 * leg];
    hit_sphere(v3(ft.p[0], ft.p[1], ft.p[2]), (float)GO1_FOOT_RADIUS, o, d, tbest, nbest, 7 + 4 * leg, idbest);
  }
}

// ---- terrain ---------------------------------------------------------------------------------------------------------------
// first root in [0, L] of  A s^2 + B s + C  (C > 0: the ray starts above the surface); -1 if none
DEV float first_root(float A, float B, float C, float L) {
  if (fabsf(A) < 1e-12f) {
    if (B >= 0.f) return -1.f;
    const float s = -C / B;
    return s <= L ? s : -1.f;
  }
  const float disc = B * B - 4.f * A * C;
  if (disc < 0.f) return -1.f;
  const float q = -0.5f * (B + copysignf(sqrtf(disc), B));
  float r1 = q / A, r2 = (q != 0.f) ? C / q : r1;
  if (r1 > r2) { const float s = r1; r1 = r2; r2 = s; }
  if (r1 >= 0.f && r1 <= L) return r1;
  if (r2 >= 0.f && r2 <= L) return r2;
  return -1.f;
}

// world ray O + t D (|D| = 1) against the bilinear height field, t in [0, tmax): 2D DDA over the cells, the ray-vs-patch
// quadratic in each.  Returns t of the hit (or -1) and the surface normal.  The walk is monotone in both cell indices, so it
// visits at most hf_rows + hf_cols cells: that bounds the loop.
DEV float hit_field(const Go1RenderConfig& cfg, const int16_t* __restrict__ hs, V3 O, V3 D, float tmax, V3& n) {
  const float hsc = cfg.hf_hscale, vs = cfg.hf_vscale;
  const int rows = cfg.hf_rows, cols = cfg.hf_cols;
  const float gx0 = (O.x + cfg.hf_border) / hsc, gy0 = (O.y + cfg.hf_border) / hsc;
  const float dgx = D.x / hsc, dgy = D.y / hsc;
  float t0 = 0.f, t1 = tmax;
  // clip to the sampled area [0, rows - 1] x [0, cols - 1] (grid units) and to the samples' height range
  const float lo[3] = {0.f, 0.f, cfg.hf_zmin}, hi[3] = {(float)(rows - 1), (float)(cols - 1), cfg.hf_zmax};
  const float og[3] = {gx0, gy0, O.z}, dg[3] = {dgx, dgy, D.z};
  for (int k = 0; k < 3; k++) {
    if (dg[k] == 0.f) {
      if (og[k] < lo[k] || og[k] > hi[k]) return -1.f;
      continue;
    }
    float ta = (lo[k] - og[k]) / dg[k], tb = (hi[k] - og[k]) / dg[k];
    if (ta > tb) { const float s = ta; ta = tb; tb = s; }
    t0 = fmaxf(t0, ta); t1 = fminf(t1, tb);
  }
  if (!(t0 < t1)) return -1.f;
  int ix = min(max((int)floorf(gx0 + t0 * dgx), 0), rows - 2);
  int iy = min(max((int)floorf(gy0 + t0 * dgy), 0), cols - 2);
  const int sx = dgx > 0.f ? 1 : -1, sy = dgy > 0.f ? 1 : -1;
  const float tdx = dgx != 0.f ? fabsf(1.f / dgx) : 1e30f, tdy = dgy != 0.f ? fabsf(1.f / dgy) : 1e30f;
  float tnx = dgx != 0.f ? ((float)(ix + (dgx > 0.f)) - gx0) / dgx : 1e30f;
  float tny = dgy != 0.f ? ((float)(iy + (dgy > 0.f)) - gy0) / dgy : 1e30f;
  float t = t0;
  for (int k = 0; k < rows + cols; k++) {
    const float tn = fminf(fminf(tnx, tny), t1);
    const int16_t* p = hs + (size_t)ix * cols + iy;
    const float h00 = p[0] * vs, h01 = p[1] * vs, h10 = p[cols] * vs, h11 = p[cols + 1] * vs;
    const float c1 = h10 - h00, c2 = h01 - h00, c3 = h00 - h10 - h01 + h11;
    const float a0 = gx0 + t * dgx - (float)ix, b0 = gy0 + t * dgy - (float)iy;
    const float C = (O.z + t * D.z) - (h00 + c1 * a0 + c2 * b0 + c3 * a0 * b0);
    const float s = C <= 0.f ? 0.f : first_root(-c3 * dgx * dgy, D.z - c1 * dgx - c2 * dgy - c3 * (a0 * dgy + b0 * dgx), C, fmaxf(tn - t, 0.f));
    if (s >= 0.f) {
      const float th = t + s;
      const float a = fminf(fmaxf(gx0 + th * dgx - (float)ix, 0.f), 1.f), b = fminf(fmaxf(gy0 + th * dgy - (float)iy, 0.f), 1.f);
      const float dhdx = (c1 + c3 * b) / hsc, dhdy = (c2 + c3 * a) / hsc;
      const float inv = rsqrtf(dhdx * dhdx + dhdy * dhdy + 1.f);
      n = v3(-dhdx * inv, -dhdy * inv, inv);
      return th;
    }
    if (tn >= t1) break;
    if (tnx <= tny) { ix += sx; tnx += tdx; if (ix < 0 || ix > rows - 2) break; }
    else { iy += sy; tny += tdy; if (iy < 0 || iy > cols - 2) break; }
    t = tn;
  }
  return -1.f;
}

DEV uint32_t to_u8(float c) { return (uint32_t)fminf(fmaxf(c * 255.f + 0.5f, 0.f), 255.f); }

struct DrawArgs {
  Go1RenderConfig cfg;
  const float* root;
  const float* dof;
  const int16_t* hs;
  const Go1RecordControl* control;          // recording: camera z reads env / slot here; NULL: env[z] into dst[z]
  uint8_t* dst[GO1RENDER_MAX_CAMERAS];
  int32_t env[GO1RENDER_MAX_CAMERAS];
};

}  // namespace

// state launch: one lane per camera (a single workgroup: nothing is exchanged between workgroups)
extern "C" __global__ void __launch_bounds__(64) render_advance_kernel(Go1RecordControl* __restrict__ ctl, int ncam,
                                                                          const uint8_t* __restrict__ reset_buf, int num_envs) {
  const int c = threadIdx.x;
  if (c >= ncam) return;
  Go1RecordControl k = ctl[c];
  if (k.env < 0 || k.env >= num_envs) return;
  const bool reset = reset_buf[k.env] != 0;
  int slot = -1;
  if (k.state == GO1REC_WAITING && reset) {          // the post-reset state of this step is frame 0
    k.state = GO1REC_RECORDING; k.frames = 0;
  } else if (k.state == GO1REC_RECORDING && reset) {  // the next reset completes the recording: no frame at this step
    k.state = GO1REC_COMPLETE;
  }
  if (k.state == GO1REC_RECORDING && k.frames < k.capacity) {
    slot = k.frames++;
    if (k.frames == k.capacity) k.state = GO1REC_COMPLETE;   // a full ring completes the recording (this frame included)
  }
  ctl[c].state = k.state;
  ctl[c].frames = k.frames;
  ctl[c].slot = slot;
}

// host reset_idx(ids) of the recorded env: WAITING -> RECORDING (the next step's frame is frame 0), RECORDING -> COMPLETE
extern "C" __global__ void __launch_bounds__(256) render_note_reset_kernel(Go1RecordControl* __restrict__ ctl, int ncam,
                                                                              const int32_t* __restrict__ ids, int n) {
  __shared__ int hit[GO1RENDER_MAX_CAMERAS];
  if (threadIdx.x < GO1RENDER_MAX_CAMERAS) hit[threadIdx.x] = (ids == nullptr) ? 1 : 0;
  __syncthreads();
  if (ids != nullptr) {
    for (int c = 0; c < ncam; c++) {
      const int e = ctl[c].env;
      for (int i = threadIdx.x; i < n; i += blockDim.x)
        if (ids[i] == e) hit[c] = 1;                 // (benign: every writer stores the same value)
    }
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)ncam && hit[threadIdx.x]) {
    Go1RecordControl& k = ctl[threadIdx.x];
    if (k.state == GO1REC_WAITING) { k.state = GO1REC_RECORDING; k.frames = 0; }
    else if (k.state == GO1REC_RECORDING) k.state = GO1REC_COMPLETE;
    k.slot = -1;
  }
}

// frame launch: grid (ceil(W / 64), H / 4, cameras), 64 x 4 threads, one pixel each
extern "C" __global__ void __launch_bounds__(TILE_X * TILE_Y) render_draw_kernel(const DrawArgs A) {
  __shared__ Body bodies[GO1_NBODY_REPORT];
  const int cam = blockIdx.z;
  int env = A.env[cam];
  uint8_t* dst = A.dst[cam];
  if (A.control != nullptr) {                        // recording: the state launch decided which slot (if any) this step fills
    const int slot = A.control[cam].slot;
    if (slot < 0 || slot >= A.control[cam].capacity || dst == nullptr) return;
    env = A.control[cam].env;
    dst += (size_t)slot * GO1RENDER_FRAME_BYTES;
  }
  const int N = A.cfg.num_envs;
  if (env < 0 || env >= N) return;
  const int tid = threadIdx.y * TILE_X + threadIdx.x;
  if (tid < 4) leg_fk(A.root, A.dof, N, env, tid, bodies);
  __syncthreads();
  const int px = blockIdx.x * TILE_X + threadIdx.x, py = blockIdx.y * TILE_Y + threadIdx.y;
  if (px >= GO1RENDER_W || py >= GO1RENDER_H) return;

  const V3 base = v3(A.root[0 * N + env], A.root[1 * N + env], A.root[2 * N + env]);
  // camera: eye at base + (0, -1, 1) looking at the base; rays relative to the base origin
  const V3 o = v3(0.f, -1.f, 1.f);
  const V3 f = (1.f / sqrtf(2.f)) * v3(0.f, 1.f, -1.f);
  const V3 right = v3(1.f, 0.f, 0.f);                // normalize(f x z)
  const V3 up = cross(right, f);
  const float u = (2.f * (px + 0.5f) / GO1RENDER_W - 1.f) * TAN_HALF_FOV;
  const float v = (1.f - 2.f * (py + 0.5f) / GO1RENDER_H) * TAN_HALF_FOV * ((float)GO1RENDER_H / GO1RENDER_W);
  V3 d = f + u * right + v * up;
  d = (1.f / norm(d)) * d;

  float t = GO1RENDER_MAX_DIST;
  V3 n = v3(0.f, 0.f, 1.f);
  int id = 0;
  hit_robot(bodies, o, d, t, n, id);
  const V3 O = base + o;
  if (A.cfg.terrain_type == 0 || A.hs == nullptr) {
    if (d.z < 0.f) {
      const float tg = -O.z / d.z;
      if (tg > 0.f && tg < t) { t = tg; n = v3(0.f, 0.f, 1.f); id = 1; }
    }
  } else {
    V3 ng;
    const float tg = hit_field(A.cfg, A.hs, O, d, t, ng);
    if (tg >= 0.f && tg < t) { t = tg; n = ng; id = 1; }
  }
  float rgb[3];
  if (id == 0) {
    rgb[0] = SKY[0]; rgb[1] = SKY[1]; rgb[2] = SKY[2];
  } else {
    const float* alb;
    if (id == 1) {
      const V3 h = O + t * d;
      const int sq = ((int)floorf(h.x) + (int)floorf(h.y)) & 1;
      alb = GROUND[sq];
    } else {
      const int b = id - 3;
      alb = PART[b == 0 ? 0 : 1 + (b - 1) % 4];
    }
    const float lam = AMBIENT + DIFFUSE * fmaxf(dot(n, v3(LIGHT[0], LIGHT[1], LIGHT[2])), 0.f);
    for (int k = 0; k < 3; k++) rgb[k] = alb[k] * lam;
  }
  const uint32_t px32 = to_u8(rgb[0]) | (to_u8(rgb[1]) << 8) | (to_u8(rgb[2]) << 16) | (255u << 24);
  reinterpret_cast<uint32_t*>(dst)[py * GO1RENDER_W + px] = px32;
}

namespace {
bool config_ok(const Go1RenderConfig* cfg, const Go1RenderBuffers* buf) {
  if (!cfg || !buf || cfg->num_envs <= 0 || cfg->num_cameras < 1 || cfg->num_cameras > GO1RENDER_MAX_CAMERAS) return false;
  if (!buf->root_states || !buf->dof_pos) return false;
  if (cfg->terrain_type != 0 && (!buf->height_samples || cfg->hf_rows < 2 || cfg->hf_cols < 2 || !(cfg->hf_hscale > 0.f))) return false;
  return true;
}
DrawArgs draw_args(const Go1RenderConfig* cfg, const Go1RenderBuffers* buf) {
  DrawArgs A = {};
  A.cfg = *cfg;
  A.root = buf->root_states;
  A.dof = buf->dof_pos;
  A.hs = cfg->terrain_type != 0 ? buf->height_samples : nullptr;
  return A;
}
const dim3 DRAW_BLOCK(TILE_X, TILE_Y);
dim3 draw_grid(int ncam) { return dim3((GO1RENDER_W + TILE_X - 1) / TILE_X, GO1RENDER_H / TILE_Y, ncam); }
static_assert(GO1RENDER_H % TILE_Y == 0, "rows tile exactly");
}  // namespace

extern "C" int go1render_record(const Go1RenderConfig* cfg, const Go1RenderBuffers* buf, void* stream) {
  if (!config_ok(cfg, buf) || !buf->reset_buf || !buf->control) return -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(render_advance_kernel, dim3(1), dim3(64), 0, st, buf->control, cfg->num_cameras, buf->reset_buf, cfg->num_envs);
  if (hipGetLastError() != hipSuccess) return -20;
  DrawArgs A = draw_args(cfg, buf);
  A.control = buf->control;
  for (int c = 0; c < cfg->num_cameras; c++) A.dst[c] = buf->frames[c];
  hipLaunchKernelGGL(render_draw_kernel, draw_grid(cfg->num_cameras), DRAW_BLOCK, 0, st, A);
  return hipGetLastError() == hipSuccess ? 0 : -21;
}

extern "C" int go1render_note_reset(const Go1RenderConfig* cfg, const Go1RenderBuffers* buf, const int32_t* ids, int32_t n, void* stream) {
  if (!config_ok(cfg, buf) || !buf->control || n < 0 || (ids == nullptr && n != 0)) return -1;
  hipLaunchKernelGGL(render_note_reset_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, buf->control, cfg->num_cameras, ids, (int)n);
  return hipGetLastError() == hipSuccess ? 0 : -20;
}

extern "C" int go1render_image(const Go1RenderConfig* cfg, const Go1RenderBuffers* buf, int32_t env, uint8_t* dst, void* stream) {
  if (!config_ok(cfg, buf) || !dst || env < 0 || env >= cfg->num_envs) return -1;
  DrawArgs A = draw_args(cfg, buf);
  A.env[0] = env;
  A.dst[0] = dst;
  hipLaunchKernelGGL(render_draw_kernel, draw_grid(1), DRAW_BLOCK, 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? 0 : -20;
}

#define GO1RENDER_STR2(x) #x
#define GO1RENDER_STR(x) GO1RENDER_STR2(x)
#ifndef GO1_SOURCE_HASH
#define GO1_SOURCE_HASH "unstamped"      // __graft_entry__.build_render_hip passes the sha256 of the sources + flags
#endif
extern "C" const char* go1render_version(void) { return "go1render 0.1 (gfx950, " GO1RENDER_STR(GO1RENDER_W) "x" GO1RENDER_STR(GO1RENDER_H) ") go1-src:" GO1_SOURCE_HASH; }
