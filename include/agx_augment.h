/*
 * agx_augment.h — random-shift augmentation on the frame history's observe: draw -> gather -> observe -> learn, the last stage.
 *
 * Why: the pixel-RL learners this library serves (DrQ, DrQ-v2 and what is built on them) pad every replayed observation by
 * `pad` pixels with edge replication and crop it back at a random offset, independently for obs and next_obs.  Written in the
 * caller's framework that is another full read and write of the batch agx_history_observe has just produced, plus an index
 * tensor and a host RNG per call.  The read path already decides where every output element comes from: the shift is folded
 * into it, and the shifts are drawn on the device as a pure integer function of (seed, call number).
 *
 * Exported by libagx.so next to agx.h, agx_loop.h, agx_hostout.h, agx_history.h, agx_glimpse.h, agx_replay.h, agx_steplog.h and
 * agx_priority.h; those headers, their structs and the ABI version are unchanged.  Errors are reported through agx_last_error
 * of the history's context (agx_last_error(NULL) when there is none).  Every call except create / destroy only enqueues on
 * `stream`: no allocation, no synchronisation, no host copy, stream-capture safe.  AGX_E_STATE while agx_env_range is narrowed.
 *
 * THE SHIFT MAP.
 *     shift_src(i, d, pad, n) = min(max(i + d - pad, 0), n - 1)        for d in 0 .. 2 * pad
 * For a sample with shift (dy, dx), every plane U[h][w] of the row agx_history_observe would have written becomes
 *     S[y][x] = U[shift_src(y, dy, pad, h)][shift_src(x, dx, pad, w)].
 * A plane is one stacked frame: [obs_h][obs_w] for AGX_HIST_FULL, for resize and for mask-out, [fov_h][fov_w] for the raw crop.
 * All frame_stack planes of a sample share one shift.  This is DrQ's replicate pad followed by a crop, and DrQ-v2's grid_sample
 * at integer shifts.  It is a pure move of elements: the output is bit for bit the gather of the unshifted output, at every
 * element type (the one rounding at the store commutes with a move).  pad = 0, or dy = dx = pad, gives agx_history_observe's
 * output bit for bit.
 *
 * WHAT THE SHIFT DOES NOT TOUCH.  d_fov_loc receives what agx_history_observe writes: the shift is not reflected in it.
 * Validity, d_valid, "rows of invalid samples are left untouched", repeats, any order, B = 0, the read-time absolute action and
 * the launches of at most 65535 samples are agx_history_observe's.
 *
 * SHIFT VALUES.  d_shift is i32 [B][2] as (dy, dx).  The device clamps each component into 0 .. 2 * pad: a wrong value is
 * defined, not wrong.  pad may exceed the plane; the clamp of shift_src then saturates.
 *
 * THE DRAW.  With mix / SM of agx_replay.h (splitmix64), a shift source holds (seed, calls) as u64 [2] on the device, and next to
 * them one u64 of bookkeeping for the draw's launch (a ticket counter, zero between launches).  Per draw:
 *     key = SM(seed, calls); then calls += 1, on the device, by the draw's launch
 *     z   = SM(key, b)                                                  sample b = 0 .. B - 1
 *     dy  = ((z >> 32) * (2 * pad + 1)) >> 32
 *     dx  = ((z & 0xFFFFFFFF) * (2 * pad + 1)) >> 32
 * Integers only, reproducible by any binding; a captured graph draws fresh shifts at every replay.
 */
#ifndef AGX_AUGMENT_H
#define AGX_AUGMENT_H

#include "agx_history.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct agx_shift agx_shift;

#define AGX_SHIFT_PAD_LIMIT 32

/*
 * A shift source on `h` for pads of `pad` pixels, 0 .. AGX_SHIFT_PAD_LIMIT; anything else, or a null argument, is
 * AGX_E_INVALID.  Allocates the source's own scratch - u64 [3]: seed, calls and the draw launch's ticket counter - outside the
 * history's block: agx_history_bytes is unchanged.  A new source has seed 0, calls 0.  Destroy the source before its history.
 */
AGX_API int agx_shift_create(agx_history *h, int32_t pad, agx_shift **out);
AGX_API int agx_shift_destroy(agx_shift *s);

/* (seed, calls = 0), enqueued on `stream`; the seed travels by value. */
AGX_API int agx_shift_seed(agx_shift *s, uint64_t seed, void *stream);

/*
 * Draw B shifts into d_shift (i32 [B][2]), one launch.  B is not bound by a grid dimension.  B = 0: AGX_OK, no launch, and
 * the call counter does not advance.  B < 0 or a null d_shift with B > 0: AGX_E_INVALID.
 */
AGX_API int agx_shift_draw(agx_shift *s, int32_t B, int32_t *d_shift, void *stream);

/*
 * agx_history_observe with the shift (d_shift[b][0], d_shift[b][1]) applied to sample b at pad `pad` (0 .. AGX_SHIFT_PAD_LIMIT).
 * Every other argument, every refusal and every output is agx_history_observe's; a null d_shift with B > 0 is AGX_E_INVALID.
 * Needs no shift source: the shifts may come from agx_shift_draw or from the caller.
 */
AGX_API int agx_history_observe_shifted(agx_history *h, int what, const int32_t *d_env, const int64_t *d_index, int32_t B,
                                        const void *d_action, int action_dtype, int32_t pad, const int32_t *d_shift,
                                        float *d_obs, int32_t *d_fov_loc, uint8_t *d_valid, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_AUGMENT_H */
