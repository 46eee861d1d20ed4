/*
 * agx_vtrace.h — V-trace returns (Espeholt et al. 2018, IMPALA) over a gathered on-policy rollout of the frame history's step
 * log, for actor-learner training: IMPALA, APPO and the PPO variants whose actors run a policy a few updates behind the learner.
 *
 * Why: the rollout gather hands a learner the last L transitions of every env, time-major, with an `ends` byte per slot, and the
 * GAE entry point next to it folds them for a learner that is strictly on-policy.  A learner whose behaviour policy mu lags its
 * target policy pi corrects for that with truncated importance ratios; the recurrence is the same backward walk over the same
 * arrays, with the same rule at episode ends: a truncated or unannounced-reset step bootstraps from the learner's value of the
 * terminal observation, a terminated one from 0.  Only the fold differs, so only the fold is here.
 *
 * Exported by libagx.so next to the other headers; their structs, entry points and the ABI version are unchanged.  Errors are
 * reported through agx_last_error of the history's context (agx_last_error(NULL) when there is none).  The call only enqueues on
 * `stream`: no allocation, no synchronisation, no host copy, stream-capture safe.  AGX_E_STATE while agx_env_range is narrowed.
 *
 * LAYOUT.  Every per-step array is time-major [L][N], element t * N + n, N the context's num_envs; t = L - 1 is the newest slot.
 * 1 <= L <= AGX_VTRACE_LIMIT and L * N <= INT32_MAX.  d_len is [N]; slot t of env n is LIVE iff t >= L - len[n].
 *
 * THE `ends` BYTE, as the rollout gather writes it; this header reads these bits, by value:
 *     1  (AGX_STEP_TERMINATED)  the episode ended behind this step: the value behind it is 0;
 *     2  (AGX_STEP_TRUNCATED), 4 (AGX_ROLLOUT_CUT)  the episode was cut behind this step; with 1 these are the bits (e & 7) that
 *                               break the chain: nothing of slot t + 1 is carried into slot t;
 *     8  (AGX_ROLLOUT_BOOT)     the value behind this step is d_boot_value[t], the learner's V(next_index).
 */
#ifndef AGX_VTRACE_H
#define AGX_VTRACE_H

#include "agx_history.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_VTRACE_LIMIT 4096   /* L: the limit of a gathered rollout */

/*
 * V-trace targets and policy-gradient advantages over a gathered rollout, one launch.  The history supplies only N, the device
 * and the error channel.
 *     d_len, d_reward, d_ends     what the rollout gather wrote, on this stream or one ordered before it
 *     d_value      f32 [L][N]     the learner's V(obs_index)
 *     d_boot_value f32 [L][N]     the learner's V(next_index); it is loaded for every slot but used only where bit 8 (BOOT) is
 *                                 set - anything else, a NaN included, never reaches an output - and it may be NULL (it then
 *                                 reads as 0)
 *     d_rho        f32 [L][N]     the importance ratio pi(a | x) / mu(a | x) of the slot's action; required.  The learner
 *                                 exponentiates: the fold takes ratios, not log-ratios, so that it holds no transcendental
 *                                 and stays bit-reproducible.  Its value in a slot that is not live reaches no output.
 *     rho_bar, c_bar, pg_rho_bar  the truncation levels of the paper's rho, c and of the ratio of the policy gradient; each
 *                                 must be > 0, +inf is legal and means no clipping
 *     d_vs, d_pg_adv f32 [L][N]   the V-trace target v_s and the advantage rho_pg (r + gamma v_(s+1) - V(x_s))
 * Per env, with A = 0, for t = L - 1 down to L - len:
 *     e      = ends[t];  newest = (t == L - 1)
 *     nv     = (e & 8) ? boot_value[t] : ((e & 1) || newest) ? 0.0f : value[t + 1]
 *     carry  = (newest || (e & 7)) ? 0.0f : A                    (vs[t + 1] - value[t + 1])
 *     td     = fadd(fadd(reward[t], fmul(gamma, nv)), -value[t])
 *     cc     = fmul(lambda, vmin(rho[t], c_bar))
 *     A      = fadd(fmul(vmin(rho[t], rho_bar), td), fmul(fmul(gamma, cc), carry))
 *     vs[t]     = fadd(A, value[t])
 *     pg_adv[t] = fmul(vmin(rho[t], pg_rho_bar), fadd(fadd(reward[t], fmul(gamma, fadd(nv, carry))), -value[t]))
 * vmin(x, bar) is x < bar ? x : bar, so a NaN ratio reads as the bar.  fadd(nv, carry) is vs[t + 1] as stored: inside an episode
 * the next slot's target, at a BOOT slot the boot value, behind TERMINATED 0.  (The gather's newest slot carries BOOT or
 * TERMINATED; for an ends byte of another origin with neither, value[L] reads as 0: nothing outside [L][N] is ever loaded.)
 * A slot that is not live gets vs = pg_adv = 0; len is clamped to 0 .. L.  fadd and fmul are single-precision with one rounding
 * each, never contracted into a multiply-add and never reassociated: a float32 model that rounds after every operation gives
 * the same bits.
 *
 * ON-POLICY.  With rho == 1 in every live slot and all three levels >= 1, A and vs are the GAE entry point's adv and ret for the
 * same finite gamma, lambda >= 0, bit for bit: vmin gives 1, the products by 1 are exact, cc = lambda, and
 * fmul(fmul(gamma, lambda), A) is GAE's carry (at a chain break it is +0 here and 0 there).  pg_adv is then the one-step advantage
 * against the V-trace target, which GAE does not compute.
 *
 * AGX_E_INVALID: a null history, L outside 1 .. AGX_VTRACE_LIMIT, L * N above INT32_MAX, a null buffer other than d_boot_value,
 * a level that is not > 0 (NaN, zero, negative) - in this order.
 */
AGX_API int agx_vtrace_returns(agx_history *h, int32_t L, const int32_t *d_len, const float *d_reward, const uint8_t *d_ends,
                               const float *d_value, const float *d_boot_value, const float *d_rho, float gamma, float lambda,
                               float rho_bar, float c_bar, float pg_rho_bar, float *d_vs, float *d_pg_adv, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_VTRACE_H */
