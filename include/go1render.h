/* go1render.h — C-ABI of the headless Go1 renderer (libgo1render.so).
 *
 * Replaces the Isaac Gym camera sensor the reference records videos with (go1_gym/envs/base/legged_robot.py:1591-1653,
 * recording boundaries :1003-1015): a ray caster that draws ONE environment's robot — the collision geometry of
 * csrc/go1_model_data.h placed by forward kinematics — and the terrain the physics samples, from the reference's camera.
 *
 * Conventions (as include/go1sim.h)
 *   - plain C; every pointer in Go1RenderBuffers is a DEVICE pointer owned by the caller.  The library never allocates,
 *     never copies between host and device and never synchronises the stream.  Return value 0 = ok, < 0 = error code.
 *   - root_states / dof_pos are the simulator's SoA buffers: component c of environment e at index c*N + e.
 *   - frames: RGBA uint8, GO1RENDER_H rows of GO1RENDER_W pixels, row 0 at the top.
 *
 * Camera: horizontal field of view 90 degrees (the Isaac Gym camera default), eye at base + (0, -1, +1) m looking at the base
 * position, world z up (reference render() / _render_headless(), :1612-1630), re-placed for every frame.
 *
 * Recording (reference start_recording / _render_headless / reset_idx, :1003-1015, :1622-1664), per camera:
 *   IDLE -> (start) WAITING -> (the env resets: the post-reset state of that step is frame 0) RECORDING
 *        -> (every later step adds a frame) -> (the env's next reset: no frame at that step) COMPLETE.
 *   A complete recording of an env that reset at steps r1 and r2 holds r2 - r1 frames.  A full ring also completes it.
 *   The state lives in a device control block, so the step loop never waits for the host: go1render_record runs two
 *   launches after a step (advance the state from reset_buf, then draw the frame the state asks for); the decision crosses
 *   the kernel boundary in Go1RecordControl.slot.  The caller launches nothing while no camera is armed.
 */
#ifndef GO1RENDER_H_INCLUDED
#define GO1RENDER_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1RENDER_W 360
#define GO1RENDER_H 240
#define GO1RENDER_FRAME_BYTES (GO1RENDER_W * GO1RENDER_H * 4)
#define GO1RENDER_MAX_CAMERAS 2
#define GO1RENDER_MAX_DIST 30.0f    /* ray length; a ray that meets nothing within it shows the sky */

enum Go1RecordState { GO1REC_IDLE = 0, GO1REC_WAITING = 1, GO1REC_RECORDING = 2, GO1REC_COMPLETE = 3 };

/* one per camera, device memory, 32 bytes.  The caller writes env / state / frames / capacity to arm a camera
 * (frames = 0, state = GO1REC_WAITING) and reads state / frames back to collect a recording. */
typedef struct Go1RecordControl {
  int32_t env;        /* recorded environment (index into the simulator's buffers) */
  int32_t state;      /* Go1RecordState */
  int32_t frames;     /* frames written to the ring so far */
  int32_t capacity;   /* frames the ring holds */
  int32_t slot;       /* written by the state launch of go1render_record: ring slot the frame launch draws, -1 = none */
  int32_t pad[3];
} Go1RecordControl;

typedef struct Go1RenderConfig {
  int32_t num_envs;       /* N of the simulator's SoA buffers */
  int32_t num_cameras;    /* 1 or 2 (train env 0, and the first evaluation env) */
  int32_t terrain_type;   /* 0 = plane z = 0, 1 = height field */
  int32_t hf_rows, hf_cols;                 /* height_samples is [hf_rows][hf_cols] int16 */
  float hf_hscale, hf_vscale, hf_border;    /* the simulator's cell convention: cell of x = (x + border) / hscale */
  float hf_zmin, hf_zmax;                   /* lowest / highest sample times vscale (bounds the rays' march) */
} Go1RenderConfig;

typedef struct Go1RenderBuffers {
  const float* root_states;        /* [13][N]: pos xyz, quat xyzw, lin vel, ang vel */
  const float* dof_pos;            /* [12][N] */
  const uint8_t* reset_buf;        /* [N]: 1 where the last step reset the environment */
  const int16_t* height_samples;   /* [hf_rows][hf_cols] or NULL (plane) */
  Go1RecordControl* control;       /* [num_cameras] */
  uint8_t* frames[GO1RENDER_MAX_CAMERAS];   /* per camera: capacity * GO1RENDER_FRAME_BYTES bytes (NULL: never armed) */
} Go1RenderBuffers;

/* after a step, while a camera is armed: advance every camera's state from reset_buf[env], then draw the frame it asks for
 * into its ring.  Two launches on `stream`. */
int go1render_record(const Go1RenderConfig* cfg, const Go1RenderBuffers* buf, void* stream);

/* a host reset_idx(ids) while a camera is armed (reference :1003: a reset of the recorded env is a recording boundary).
 * ids = NULL: every environment.  Otherwise n device int32 ids, scanned on the device.  One launch, draws nothing. */
int go1render_note_reset(const Go1RenderConfig* cfg, const Go1RenderBuffers* buf, const int32_t* ids, int32_t n, void* stream);

/* render(): draw environment `env` now into dst (GO1RENDER_FRAME_BYTES device bytes).  One launch; reads no control block. */
int go1render_image(const Go1RenderConfig* cfg, const Go1RenderBuffers* buf, int32_t env, uint8_t* dst, void* stream);

/* "go1render <version> (gfx950) go1-src:<16 hex digits of the source hash>" */
const char* go1render_version(void);

#ifdef __cplusplus
}
#endif

#endif
