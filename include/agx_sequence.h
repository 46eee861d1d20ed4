/*
 * agx_sequence.h — sequence replay on the frame history: L consecutive steps of one episode per sample, padded and masked, for
 * recurrent learners (R2D2 and its family).
 *
 * Why: the replay stack on the history (agx_history.h, agx_glimpse.h, agx_replay.h, agx_steplog.h, agx_priority.h,
 * agx_augment.h) hands out independent transitions.  An agent that looks through a fovea solves a partially observed problem,
 * and its recurrent learner trains on sequences: L consecutive env-steps of one episode, the steps past the episode's end
 * padded and masked, each step with its action, reward, end flag and n-step target.  Where a sequence has to stop is device
 * state - the per-env append counts, the age byte of every row, which rows were recorded - so the rules are applied on the
 * device, and the padded steps receive defined values: a padded batch needs no memset.
 *
 * Exported by libagx.so next to agx.h, agx_loop.h, agx_hostout.h, agx_history.h, agx_glimpse.h, agx_replay.h, agx_steplog.h,
 * agx_priority.h and agx_augment.h; those headers, their structs and the ABI version are unchanged.  Errors are reported through
 * agx_last_error of the history's context (agx_last_error(NULL) when there is none).  Every call only enqueues on `stream`: no
 * allocation, no synchronisation, no host copy, stream-capture safe.  AGX_E_STATE while agx_env_range is narrowed.
 *
 * A SEQUENCE is (env n, start index k, length L), 1 <= L <= AGX_SEQUENCE_LIMIT; sample b of a call is (d_env[b], d_index[b]) and
 * all B samples of a call share L.  Step l = 0 .. L - 1 of sample b is the env-step (n, k + l).
 *
 * LAYOUT.  A [B][L] output has row b * L + l, or l * B + b when time_major != 0; the flag holds for every per-step output of a
 * call.  d_len is [B].
 *
 * LENGTH.  With cnt = count[n] and age[j] the age byte of row j of env n:
 *     len(b) = 0                      if (n, k) is not valid by agx_history_observe's own rule;
 *     len(b) = 1 + f                  otherwise, f the largest value <= L - 1 with k + f < cnt and no age == 0 row in (k, k + f].
 * Put differently len(b) = 1 + min(ahead, L - 1) with agx_replay_inspect's `ahead`, which saturates at 255: hence the limit of
 * 256 = 1 + 255.  Step l is LIVE iff l < len(b).  A sequence never crosses a reset (an AGX_CMD_CLEAR append has age 0), stops at
 * the end of the history and starts only where the history can re-create the observation.
 *     Every live (n, k + l) is valid by the history's rule (the argument of agx_replay.h): inside an episode the ages count up by
 *     one per append, so the oldest row (n, k + l) needs is k + l - min(age[k] + l, fs - 1), which is never older than
 *     k - min(age[k], fs - 1), the one k needs; a saturated age of 255 exceeds fs - 1 either way.
 *
 * The existing samplers already guarantee a minimum length: a start drawn with forward = m - 1 has len >= min(m, L).
 */
#ifndef AGX_SEQUENCE_H
#define AGX_SEQUENCE_H

#include "agx_history.h"
#include "agx_steplog.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_SEQUENCE_LIMIT 256   /* L: 1 + the 255 at which agx_replay_inspect's `ahead` saturates */

/*
 * d_len[b] (i32 [B]) = len(b) of the sequences (d_env[b], d_index[b], L).  Needs only a history.  One launch, B is not bound by a
 * grid dimension.  AGX_E_INVALID: L outside 1 .. AGX_SEQUENCE_LIMIT, B < 0, B * L above INT32_MAX, a null buffer with B > 0, a
 * null history (checked in this order).  B = 0: AGX_OK, no launch.
 */
AGX_API int agx_sequence_lengths(agx_history *h, const int32_t *d_env, const int64_t *d_index, int32_t B, int32_t L,
                                 int32_t *d_len, void *stream);

/*
 * The step-log rows of every step of the sequences, one launch.  For a live step (b, l) the outputs are bit for bit what
 * agx_steplog_gather(nstep, gamma) writes for the sample (n, k + l) - the same walk, which may run past the sequence's last
 * step: the target of a late step lies outside the sequence.  Where a step is not live, or its walk folds no row:
 * steps = 0, next_index = -1, and ret, discount, flags and payload are all-zero bytes.  Every element of every output that is
 * passed is written.
 *     d_len        i32 [B]          len(b); may be NULL
 *     d_steps      i32 [B][L]       required with B > 0
 *     d_next_index i64 [B][L]       k + l + steps, or -1
 *     d_ret        f32 [B][L]       d_discount f32 [B][L]      d_flags u8 [B][L]
 *     d_payload    u8  [B][L][W]    W = the log's payload_bytes (ignored when W = 0)
 * Every output except d_steps may be NULL.  nstep in 1 .. AGX_STEPLOG_NSTEP_LIMIT.  AGX_E_INVALID: L, nstep, B < 0, B * L above
 * INT32_MAX, a null d_env / d_index / d_steps with B > 0, a null log (in this order).  B = 0: AGX_OK, no launch.
 */
AGX_API int agx_sequence_gather(agx_steplog *log, const int32_t *d_env, const int64_t *d_index, int32_t B, int32_t L, int32_t nstep,
                                float gamma, int time_major, int32_t *d_len, int32_t *d_steps, int64_t *d_next_index, float *d_ret,
                                float *d_discount, uint8_t *d_flags, void *d_payload, void *stream);

/*
 * The observations of every step of the sequences.  d_obs is [rows][planes][h][w], rows = B * L in the layout above, in the
 * context's AGX_OBS_* element type; h and w are agx_history_observe's for `what` (AGX_HIST_FOVEA / AGX_HIST_FULL) and the
 * context's mode.  Plane p is stack position frame_stack - planes + p: planes = frame_stack gives the whole observation,
 * planes = 1 the newest frame alone - what a recurrent network usually wants.
 *     A step (b, l) is written as live iff l < min(d_len[b], L) and (n, k + l) is valid by the history's rule: the kernel checks
 *     validity itself, so a wrong d_len gives a defined result.  d_len (i32 [B]) is required: agx_sequence_lengths or
 *     agx_sequence_gather wrote it, on this stream or one ordered before it.
 *     A live step's planes are bit for bit the planes of agx_history_observe(what, d_action = NULL) at (n, k + l), at the
 *     recorded fov_loc; d_fov_loc (i32 [rows][2], fixed contexts only, may be NULL) receives it and d_live (u8 [rows], may be
 *     NULL) receives 1.
 *     Every other step receives all-zero bytes, d_fov_loc (0, 0) and d_live 0.  Every element of every output that is passed is
 *     written.
 * More than 65535 rows go out as several launches.  Read-time actions, shifts and the glimpse memory are not served here.
 * AGX_E_INVALID: L, what, planes < 1, B < 0, B * L above INT32_MAX, a null d_env / d_index / d_len / d_obs with B > 0, a null
 * history (in this order); planes > frame_stack once the history is known.  AGX_E_STATE: AGX_HIST_FOVEA on a base context.
 * B = 0: AGX_OK, no launch, in front of the range check as in agx_history_observe.
 */
AGX_API int agx_sequence_observe(agx_history *h, int what, const int32_t *d_env, const int64_t *d_index, const int32_t *d_len,
                                 int32_t B, int32_t L, int32_t planes, int time_major, void *d_obs, int32_t *d_fov_loc,
                                 uint8_t *d_live, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_SEQUENCE_H */
