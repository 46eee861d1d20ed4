/*
 * agx_history.h — an on-device frame history that re-creates past observations.
 *
 * Why: an observation batch is [N][fs][h][w] elements (113 KB per env-step at float32 84 x 84 x 4) - too large to keep.
 * But every observation a step returns is a pure function of the env's last `fs` u8 frames (7 KB each, one new one per
 * env-step) and its fov_loc (8 bytes).  The history keeps exactly those in HBM, T env-steps per env, and
 * agx_history_observe re-materialises the observation of any retained env-step - bit for bit what the step wrote - or,
 * with an absolute sensory action supplied at read time, what the env would have seen had it looked there instead.  A
 * replay buffer stores the (env, index) pair next to its actions and rewards instead of the observation.
 *
 * Everything here is exported by libagx.so next to include/agx.h, agx_loop.h and agx_hostout.h; those headers, their
 * structs and the ABI version are unchanged.  Errors are reported through agx_last_error of the history's context
 * (agx_last_error(NULL) when there is none).
 *
 * Scope: gray contexts of kind AGX_KIND_BASE and AGX_KIND_FIXED, every output mode, action mode and AGX_OBS_* type.
 * Peripheral, flexible and AGX_FRAME_RGB contexts: AGX_E_STATE.
 */
#ifndef AGX_HISTORY_H
#define AGX_HISTORY_H

#include "agx_loop.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct agx_history agx_history;

/*
 * A history of `capacity` = T env-steps per env for `ctx` (T >= frame_stack, else AGX_E_INVALID).  Device storage, all
 * allocated here, rows indexed [t][n] with t = index mod T:
 *     u8  [T][N][obs_h * obs_w]  frames        u8  [T][N]  age (appends since the env's last CLEAR, saturating at 255)
 *     i32 [T][N][2]              fov_loc       i64 [N]     per-env append count
 * AGX_E_NOMEM when the allocation fails; AGX_E_STATE for a peripheral, flexible or AGX_FRAME_RGB context and while
 * agx_env_range is narrowed.  Destroy the history before its context.
 *
 * A new history takes the frames before an env's first append to be zero, which is what a new context's ring holds:
 * create it before the first ingest (or start every env with an AGX_CMD_CLEAR ingest, as a reset does).
 */
AGX_API int agx_history_create(agx_ctx *ctx, int32_t capacity, agx_history **out);
AGX_API int agx_history_destroy(agx_history *h);

/*
 * Every index becomes invalid and the per-env counts go back to 0 (enqueued on `stream`).  The frames an env ingested
 * before the clear are gone: until its next AGX_CMD_CLEAR ingest, samples whose stack would reach behind the clear
 * (the env's first frame_stack - 1 appends) are invalid rather than wrong.  agx_set_stack_u8 is not tracked: clear
 * the history after it.
 */
AGX_API int agx_history_clear(agx_history *h, void *stream);

/* Device bytes the history holds. */
AGX_API int64_t agx_history_bytes(const agx_history *h);

/*
 * After a step's ingest (and its fovea call, if the context has one): append each env's NEWEST ring frame and its
 * CURRENT fov_loc.  d_cmd: the command bytes that ingest was given, read as it reads them -
 *     AGX_CMD_SKIP   nothing is appended, d_index[n] = -1;
 *     AGX_CMD_CLEAR  append with age 0;
 *     otherwise      append with age = min(previous age + 1, 255).
 * d_index (i64 [N], may be NULL) receives the env's append count before the increment: the index of this append,
 * monotone per env and never reused until agx_history_clear.
 * One push follows one ingest.  A second push without an ingest between appends the same frame again with a larger
 * age - the history then no longer mirrors the ring: do not.
 * Only enqueues on `stream`: no allocation, no synchronisation, no host copy.  AGX_E_STATE while agx_env_range is
 * narrowed.
 */
AGX_API int agx_history_push(agx_history *h, const uint8_t *d_cmd, int64_t *d_index, void *stream);

/* The index of each env's newest append, count - 1 (-1: none yet), into d_index i64 [N]: after a step's push and the
 * push of its autoreset pass this is the index of the observation that step returned for every env. */
AGX_API int agx_history_last_index(agx_history *h, int64_t *d_index, void *stream);

#define AGX_HIST_FOVEA 0   /* the context's own observation (raw crop / mask-out / resize as configured) */
#define AGX_HIST_FULL  1   /* the base observation: the stack, oldest -> newest, k/255: [fs][obs_h][obs_w] */

/*
 * Re-create the observations of B samples b = (env d_env[b], index d_index[b]) into d_obs [B] rows of agx_obs_shape
 * (AGX_HIST_FULL: [B][fs][obs_h][obs_w]) in the context's AGX_OBS_* element type.
 *     Stacked frame j (0 = oldest) is row k - (fs-1-j) of env n when fs-1-j <= age[k], zeros otherwise - what the ring
 *     held after that ingest.
 *     d_action == NULL: the position is the recorded fov_loc[k], and the output of a valid sample equals BIT FOR BIT
 *     the observation (and fov_loc) the step's own agx_fovea_fixed / agx_observe_full wrote right before that push.
 *     d_action != NULL ([B][2], action_dtype AGX_DT_*): the position is rint(clip(a, 0, obs - fov)) of the given
 *     ABSOLUTE action, whatever the context's action mode.  It does not change AGX_HIST_FULL's image.
 *     A sample is valid iff 0 <= env < N, 0 <= k < count[n] and every row it needs is still retained:
 *     k - min(age[k], fs-1) >= max(count[n] - T, 0).  An invalid sample gets d_valid[b] = 0 and its d_obs /
 *     d_fov_loc rows are left untouched, like a masked env; a valid one d_valid[b] = 1.
 * Samples may repeat and come in any order.  d_fov_loc (i32 [B][2]) and d_valid (u8 [B]) may be NULL; d_fov_loc is
 * not written on a base context.  B = 0: AGX_OK, no launch.  On a base context only AGX_HIST_FULL is valid
 * (AGX_E_STATE otherwise).  Only enqueues on `stream`.
 */
AGX_API int agx_history_observe(agx_history *h, int what, const int32_t *d_env, const int64_t *d_index, int32_t B,
                                const void *d_action, int action_dtype, float *d_obs, int32_t *d_fov_loc,
                                uint8_t *d_valid, void *stream);

/*
 * The native loop keeps `h` (a history of the loop's context; NULL detaches): agx_loop_step / agx_loop_step_host push
 * after the step's observation, and every reset pass (agx_loop_reset, agx_loop_reset_envs, the autoreset inside a
 * step) pushes after its re-observation with the pass's own command bytes - the reset envs CLEAR, the others SKIP.
 * For an env that was autoreset in a step, the terminal observation is the index before its newest.
 */
AGX_API int agx_loop_set_history(agx_loop *loop, agx_history *h);

#ifdef __cplusplus
}
#endif
#endif /* AGX_HISTORY_H */
