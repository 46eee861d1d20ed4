/*
 * agx_rollout.h — on-policy rollouts on the frame history's step log: the last L transitions of EVERY env, cut at episode ends,
 * and GAE(lambda) over them, for PPO / A2C and their family.
 *
 * Why: the replay stack on the history (agx_replay.h, agx_steplog.h, agx_priority.h, agx_sequence.h) serves drawn samples.  An
 * on-policy learner wants no draw: it wants what every env did since the last update, it crosses episode ends, and it has to know
 * where.  Which rows those are is device state - an autoreset step pushes two rows, row reuse is index mod T, a row written by a
 * reset is never recorded, the retained range differs per env - and at a truncation, or at a reset that no end flag announced, the
 * return has to bootstrap from V(last observation of the old episode): not from 0 and not from the reset observation.  The
 * history retains that observation (the terminal observation is a row of its own) and the step log tells TERMINATED from
 * TRUNCATED, so the rule is stated here once, with invalid-rather-than-wrong semantics like the other readers.
 *
 * Exported by libagx.so next to agx.h, agx_loop.h, agx_hostout.h, agx_history.h, agx_glimpse.h, agx_replay.h, agx_steplog.h,
 * agx_priority.h, agx_augment.h and agx_sequence.h; those headers, their structs and the ABI version are unchanged.  Errors are
 * reported through agx_last_error of the history's context (agx_last_error(NULL) when there is none).  Every call only enqueues on
 * `stream`: no allocation, no synchronisation, no host copy, stream-capture safe.  AGX_E_STATE while agx_env_range is narrowed.
 *
 * LAYOUT.  Every per-step array is time-major [L][N], element t * N + n, N the context's num_envs; t = L - 1 is the newest slot.
 * 1 <= L <= AGX_ROLLOUT_LIMIT and L * N <= INT32_MAX.  d_len is [N].
 *
 * THE RULE.  One function of the env decides its rollout.  With cnt = count[n], lo = max(cnt - T, 0), and age[j], stamp[j] the
 * history's age byte and the log's stamp of row j of env n: walk j = cnt - 1 downward while j > lo, filling slots from t = L - 1
 * down:
 *     age[j] == 0                                        a reset observation: no transition; skip it and go on with j - 1;
 *     else stamp[j] != j                                 the row was never recorded: stop;
 *     else observation j - 1 is not valid by agx_history_observe's own rule (its stack reaches an evicted row): stop;
 *     else slot t is the transition (obs_index = j - 1, next_index = j), with row j's reward, payload and an `ends` byte; t -= 1;
 *     stop once L slots are filled.
 * len(n) = the number of slots filled; slot t is LIVE iff t >= L - len(n).  Every live obs_index and next_index is valid for
 * agx_history_observe: j - 1 by the third line, and j because inside an episode the oldest row j needs is never older than the
 * one j - 1 needs (the argument of agx_replay.h).
 *
 * THE `ends` BYTE of a live slot, from row j:
 *     AGX_STEP_TERMINATED (1), AGX_STEP_TRUNCATED (2)    the row's recorded flags;
 *     AGX_ROLLOUT_CUT (4)     j + 1 < cnt, age[j + 1] == 0 and neither end flag: the env was reset behind this step unannounced;
 *     AGX_ROLLOUT_BOOT (8)    TERMINATED is not set and (t == L - 1 or TRUNCATED or CUT): the learner's value of observation
 *                             next_index will be read (agx_rollout_gae's d_boot_value).
 * Where a live slot t < L - 1 has none of the bits, next_index[t] == obs_index[t + 1], so V(next) is the next slot's value and
 * needs no evaluation of its own.  The argument: slot t + 1 was filled from the row j' > j the walk took just before j, and
 * every row between them was skipped, which takes age == 0.  Were j' > j + 1, row j + 1 would be such a row, and with
 * j + 1 < j' < cnt slot t carries an end flag or CUT.  It carries none, so j' = j + 1 and obs_index[t + 1] = j' - 1 = j.
 */
#ifndef AGX_ROLLOUT_H
#define AGX_ROLLOUT_H

#include "agx_history.h"
#include "agx_steplog.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_ROLLOUT_LIMIT 4096   /* L */
#define AGX_ROLLOUT_CUT 4        /* ends: a reset behind this step that no end flag announced */
#define AGX_ROLLOUT_BOOT 8       /* ends: the return bootstraps from d_boot_value, the learner's V(next_index) */

/*
 * The rollout of every env, one launch.
 *     d_len        i32 [N]          len(n)
 *     d_obs_index  i64 [L][N]       required
 *     d_next_index i64 [L][N]
 *     d_reward     f32 [L][N]       d_ends u8 [L][N]
 *     d_payload    u8  [L][N][W]    W = the log's payload_bytes (ignored when W = 0): the action taken on seeing obs_index
 * Every output except d_obs_index may be NULL.  Every element of every output that is passed is written: a slot that is not
 * live gets obs_index = next_index = -1, reward 0, ends 0 and all-zero payload bytes, so no output needs a memset.  The env of
 * element (t, n) is n: (n, obs_index) and (n, next_index) are samples for agx_history_observe.
 * AGX_E_INVALID: a null log, L outside 1 .. AGX_ROLLOUT_LIMIT, L * N above INT32_MAX, a null d_obs_index (in this order).
 */
AGX_API int agx_rollout_gather(agx_steplog *log, int32_t L, int32_t *d_len, int64_t *d_obs_index, int64_t *d_next_index,
                               float *d_reward, uint8_t *d_ends, void *d_payload, void *stream);

/*
 * GAE(lambda) over a gathered rollout, one launch.  The history supplies only N, the device and the error channel.
 *     d_len, d_reward, d_ends     what agx_rollout_gather wrote, on this stream or one ordered before it
 *     d_value      f32 [L][N]     the learner's V(obs_index)
 *     d_boot_value f32 [L][N]     the learner's V(next_index); its values are used only where BOOT is set - anything else,
 *                                 a NaN included, never reaches an output - and it may be NULL only if the caller passes no
 *                                 row with BOOT (a NULL reads as 0)
 *     d_adv, d_ret f32 [L][N]     the advantage and the return adv + value
 * Per env, with gl = fmul(gamma, lambda) and A = 0, for t = L - 1 down to L - len:
 *     e      = ends[t]
 *     nv     = (e & BOOT) ? boot_value[t] : (e & TERMINATED) ? 0.0f : value[t + 1]
 *     delta  = fadd(fadd(reward[t], fmul(gamma, nv)), -value[t])
 *     carry  = (t == L - 1 || (e & 7)) ? 0.0f : fmul(gl, A)
 *     A      = fadd(delta, carry)
 *     adv[t] = A
 *     ret[t] = fadd(A, value[t])
 * (agx_rollout_gather's newest slot carries BOOT or TERMINATED; for an ends byte of another origin with neither, value[L] reads
 * as 0: nothing outside [L][N] is ever loaded.)  A slot that is not live gets adv = ret = 0;
 * len is clamped to 0 .. L.  fadd and fmul are single-precision with one rounding each, never contracted into a multiply-add
 * and never reassociated: a float32 model that rounds after every operation gives the same bits.
 * AGX_E_INVALID: a null history, L outside 1 .. AGX_ROLLOUT_LIMIT, L * N above INT32_MAX, a null buffer other than d_boot_value
 * (in this order).
 */
AGX_API int agx_rollout_gae(agx_history *h, int32_t L, const int32_t *d_len, const float *d_reward, const uint8_t *d_ends,
                            const float *d_value, const float *d_boot_value, float gamma, float lambda, float *d_adv,
                            float *d_ret, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_ROLLOUT_H */
