/*
 * agx_steplog.h — a step log next to the frame history: reward, end flags and an opaque payload (the action) per retained
 * env-step, and one device gather that turns drawn samples into learner rows with n-step targets.
 *
 * Why: the frame history (agx_history.h) re-creates observations and the replay sampler (agx_replay.h) draws (env, index)
 * pairs on the device.  A learner also needs the action taken, the reward, whether the episode ended and, for n-step targets,
 * the discounted reward sum up to the episode's end.  A caller who keeps [T][N] arrays of its own has to get the row reuse
 * index mod T, the two pushes of an autoreset step, the stop at a reset and the rows that were never written right - all of
 * which depend on state only the device holds.  The log keeps those columns in the history's own row order and gathers them by
 * the history's own counts and ages: a sample it cannot serve comes back invalid rather than wrong.
 *
 * Exported by libagx.so next to agx.h, agx_loop.h, agx_hostout.h, agx_history.h, agx_glimpse.h and agx_replay.h; those headers,
 * their structs and the ABI version are unchanged.  Errors are reported through agx_last_error of the history's context
 * (agx_last_error(NULL) when there is none).  Every call except create / destroy only enqueues on `stream` (record, gather:
 * kernels; clear: one hipMemsetAsync): no allocation, no synchronisation, no host copy, stream-capture safe.  create, record and
 * gather are AGX_E_STATE while agx_env_range is narrowed.
 *
 * A ROW.  Row k of env n holds the data of the step that PRODUCED observation k: the action taken on seeing k - 1 (in the
 * payload), the reward received, and the end flags of observation k.  A reset observation (age 0) has no such step; its row is
 * never read.
 *
 * THE WALK.  For sample b = (n, k), with cnt = count[n], age[j] the history's age byte and stamp[j] the log's stamp of row j:
 *     ok0 = 0 <= n < N and 0 <= k < cnt and k >= cnt - T
 *     m = 0; G = 0.0f; disc = 1.0f; last = 0
 *     for i = 1 .. nstep while ok0:
 *         j = k + i
 *         stop if j >= cnt, or age[j] == 0 (another episode), or stamp[j] != j (never recorded)
 *         G = fadd(G, fmul(disc, reward[j])); disc = fmul(disc, gamma); m = i; last = flags[j]
 *         stop after this row if last & (AGX_STEP_TERMINATED | AGX_STEP_TRUNCATED)
 * fadd and fmul are single precision, round to nearest, one rounding each and never contracted into a fused multiply-add: a
 * float32 model that rounds after every operation gives the same bits.
 *
 * Why k >= cnt - T is enough: every j in (k, cnt) is then retained as well (j > k >= cnt - T), so age[j] and row j mod T are
 * j's own.  If j was never recorded, row j mod T holds -1 or the stamp of an index congruent to j that was retained when it
 * was recorded - j - T or older - which can never equal j.  A stamp therefore equals j only if row j was recorded for j, and
 * nothing has overwritten it since (only an index >= j + T could, and that is not retained before j is evicted).
 */
#ifndef AGX_STEPLOG_H
#define AGX_STEPLOG_H

#include "agx_history.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct agx_steplog agx_steplog;

#define AGX_STEPLOG_PAYLOAD_LIMIT 64   /* payload bytes per row */
#define AGX_STEPLOG_NSTEP_LIMIT   64
#define AGX_STEP_TERMINATED 1          /* flag bits of a row */
#define AGX_STEP_TRUNCATED  2

/*
 * A log on `h` with W = payload_bytes per row: 0 .. AGX_STEPLOG_PAYLOAD_LIMIT and a multiple of 4, anything else or a null
 * argument is AGX_E_INVALID.  One device allocation of the log's own, outside the history's block (agx_history_bytes is
 * unchanged), rows indexed [t][n] with t = index mod T like the history's:
 *     f32 [T][N] reward      u8 [T][N] flags      i64 [T][N] stamp (the index the row was recorded for; -1 after create / clear)
 *     u8  [T][N][W] payload (opaque to the library)
 * AGX_E_NOMEM / AGX_E_HIP as agx_history_create reports them.  Destroy the log before its history.
 */
AGX_API int agx_steplog_create(agx_history *h, int32_t payload_bytes, agx_steplog **out);
AGX_API int agx_steplog_destroy(agx_steplog *s);

/*
 * Every row becomes unrecorded (the stamps go to -1).  It MUST follow agx_history_clear: the history's indices restart at 0
 * there, and a stamp left from before the clear could equal a new index.
 */
AGX_API int agx_steplog_clear(agx_steplog *s, void *stream);

/* Device bytes the log holds. */
AGX_API int64_t agx_steplog_bytes(const agx_steplog *s);

/*
 * For each env n with d_index[n] >= 0 and count[n] - T <= d_index[n] < count[n]: write d_reward[n] (f32 [N]), d_flags[n]
 * (u8 [N]), the W payload bytes at d_payload + n * W (4-byte aligned; ignored when W = 0) and stamp = d_index[n] into row
 * d_index[n].  Every other env is skipped silently: d_index[n] = -1 is how the caller skips one.  Recording a row again
 * overwrites it.  The counts are read on `stream`: call on the stream that pushes, or order the calls against it.
 */
AGX_API int agx_steplog_record(agx_steplog *s, const int64_t *d_index, const float *d_reward, const uint8_t *d_flags,
                               const void *d_payload, void *stream);

/*
 * The walk above for B samples b = (d_env[b], d_index[b]), nstep in 1 .. AGX_STEPLOG_NSTEP_LIMIT.  With m the rows folded:
 *     m > 0:   d_steps[b] = m, d_next_index[b] = k + m (the observation to bootstrap from), d_return[b] = G,
 *              d_discount[b] = (last & AGX_STEP_TERMINATED) ? 0 : disc, d_flags[b] = last, and the W payload bytes of row k + 1
 *              (the action taken on seeing k) at d_payload + b * W.
 *     m == 0:  d_steps[b] = 0, d_next_index[b] = -1; the sample's other outputs are left untouched, like a masked env
 *              (agx_history_observe leaves index -1 untouched too).
 * Every output except d_steps (i32 [B]) may be NULL; d_payload is ignored when W = 0.  Samples may repeat and come in any
 * order.  B is not bound by a grid dimension.  B = 0: AGX_OK, no launch.  B < 0, nstep out of range or a null d_env /
 * d_index / d_steps with B > 0: AGX_E_INVALID.
 */
AGX_API int agx_steplog_gather(agx_steplog *s, const int32_t *d_env, const int64_t *d_index, int32_t B, int32_t nstep, float gamma,
                               float *d_return, float *d_discount, int32_t *d_steps, int64_t *d_next_index, uint8_t *d_flags,
                               void *d_payload, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_STEPLOG_H */
