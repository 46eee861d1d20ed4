/*
 * agx_retrace.h — Retrace-family Q-returns over a sequence-replay batch: the lambda-weighted, importance-corrected Q-return
 * folded backward along each sequence and cut where the sequence is cut.  One fold serves Retrace (Munos et al. 2016; Reactor,
 * ACER, MPO, Agent57), Peng's / Harutyunyan's Q(lambda) and Tree-backup: they differ only in the trace coefficient, which the
 * caller supplies per step.
 *
 * Why: agx_sequence_gather hands a recurrent learner L consecutive steps per sample with n-step targets.  The off-policy learners
 * that train on sequences want the return that looks through the whole sequence instead, and where that return has to stop is
 * the same device state the gather already resolved: where the sequence ends (d_len), which step's row was never recorded
 * (d_steps) and where the bootstrap lies outside the sequence (next_index of the last step).  A Python loop over l with a dozen
 * indexed operations per step is what this one launch replaces.
 *
 * Exported by libagx.so next to the other headers; their structs, entry points and the ABI version are unchanged.  Errors are
 * reported through agx_last_error of the history's context (agx_last_error(NULL) when there is none).  The call only enqueues on
 * `stream`: no allocation, no synchronisation, no host copy, stream-capture safe.  AGX_E_STATE while agx_env_range is narrowed.
 *
 * LAYOUT.  agx_sequence_gather's: a [B][L] array has element b * L + l, or l * B + b when time_major != 0; the flag holds for
 * every per-step array of a call.  1 <= L <= AGX_SEQUENCE_LIMIT, B >= 0, B * L <= INT32_MAX; B is not bound by a grid dimension.
 */
#ifndef AGX_RETRACE_H
#define AGX_RETRACE_H

#include "agx_history.h"
#include "agx_sequence.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The Q-return targets of B sequences, one launch.  The history supplies only the device and the error channel.
 *     d_len      i32 [B]      agx_sequence_gather's (or agx_sequence_lengths')
 *     d_steps    i32 [B][L]   agx_sequence_gather's d_steps, d_ret and d_discount of a gather with nstep = 1: the step's
 *     d_reward   f32 [B][L]   reward and the discount behind it (0 behind a terminated step)
 *     d_discount f32 [B][L]
 *     d_q        f32 [B][L]   the learner's Q of the action taken at step l
 *     d_v        f32 [B][L]   its expected value under the target policy at step l's observation
 *     d_c        f32 [B][L]   the trace coefficient of step l's action - Retrace: lambda min(1, pi / mu); Q(lambda): lambda;
 *                             Tree-backup: lambda pi(a | x)
 *     d_boot     f32 [B]      the expected value at the observation behind the last step, next_index[b][L - 1]; may be NULL
 *                             (it then reads as 0)
 *     d_target   f32 [B][L]   the return T;  d_td f32 [B][L]  T - q, may be NULL;  d_valid u8 [B][L]  may be NULL
 * With len' = clamp(len[b], 0, L) and has(l) = l < len' and steps[l] == 1 - any other steps value is "no row": a padded step, a
 * step whose row was never recorded, the terminal observation's own step, a batch gathered with nstep > 1 - and has(L) = false,
 * per sequence for l = L - 1 down to 0:
 *     vnext = (l + 1 < len') ? v[l + 1] : boot[b]
 *     carry = has(l + 1) ? fmul(c[l + 1], fsub(T[l + 1], q[l + 1])) : 0
 *     T[l]  = fadd(reward[l], fmul(discount[l], fadd(vnext, carry)))
 * (In a batch as the gather writes it the last step of a sequence that stops short of L has no row - it is the terminal
 * observation's own step, or the newest observation, whose step is not recorded yet - so boot is read iff len = L and step L - 1
 * has a row; for arrays of another origin the rule above holds as it stands.)
 * If has(l): target = T[l], td = fsub(T[l], q[l]), valid = 1.  Otherwise all three are 0 - a select, not a product: garbage or a
 * NaN in a step without a row never shows, and a chain never crosses such a step.  Every element of every output that is passed
 * is written: no output needs a memset.  fadd, fsub and fmul are single-precision, round-to-nearest, one rounding each, never
 * contracted into a multiply-add and never reassociated: a float32 model that rounds after every operation gives the same bits.
 *
 * AGX_E_INVALID: L outside 1 .. AGX_SEQUENCE_LIMIT, B < 0, B * L above INT32_MAX, a null d_len / d_steps / d_reward /
 * d_discount / d_q / d_v / d_c / d_target with B > 0, a null history (in this order).  B = 0: AGX_OK, no launch, in front of the
 * range check as in agx_sequence_observe.
 */
AGX_API int agx_sequence_retrace(agx_history *h, int32_t B, int32_t L, int time_major, const int32_t *d_len, const int32_t *d_steps,
                                 const float *d_reward, const float *d_discount, const float *d_q, const float *d_v, const float *d_c,
                                 const float *d_boot, float *d_target, float *d_td, uint8_t *d_valid, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_RETRACE_H */
