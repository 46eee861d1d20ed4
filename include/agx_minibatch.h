/*
 * agx_minibatch.h — device-side minibatches on a gathered on-policy rollout: the list of its LIVE or BOOT slots, a seeded
 * permutation of that list, and one launch per minibatch that writes everything a PPO learner reads for S list positions, at
 * fixed shapes and with defined padding.
 *
 * Why: the rollout gather and the GAE / V-trace folds only enqueue on the caller's stream.  What a learner does next did not:
 * finding the live slots, and the slots whose value bootstraps, is a nonzero() - the count is data, so the host waits for it -
 * and every minibatch of every epoch is a host-made permutation and a dozen indexed reads.  The replay side draws on the device
 * as a pure integer function of (seed, call number) and the host never sees a count; this header is the on-policy counterpart.
 *
 * Exported by libagx.so next to the other headers; their structs, entry points and the ABI version are unchanged.  Errors are
 * reported through agx_last_error of the history's context (agx_last_error(NULL) when there is none).  Every call except create
 * and destroy only enqueues on `stream`: no allocation, no synchronisation, no host copy, stream-capture safe.  AGX_E_STATE
 * while agx_env_range is narrowed.
 *
 * LAYOUT.  Every per-slot array is the rollout gather's: time-major [L][N], slot element e = t * N + n, N the context's
 * num_envs; t = L - 1 is the newest slot.  1 <= L <= AGX_MB_LIMIT and L * N <= INT32_MAX.  d_len is [N].
 *
 * THE RULE.  With len'(n) = clamp(len[n], 0, L) as in the folds, slot (t, n) is SELECTED when
 *     AGX_MB_LIVE    t >= L - len'(n);
 *     AGX_MB_BOOT    the same, and ends[t][n] & 8 (the gather's BOOT bit: the learner's value of next_index is read there).
 * THE LIST is env-major: env 0's selected slots by ascending t, then env 1's, and so on.  With off[0 .. N] the exclusive prefix
 * sum of the per-env counts and total = off[N], position m is (n, r) with off[n] <= m < off[n + 1], r = m - off[n]: the r-th
 * selected slot of env n.  For LIVE that is t = L - len'(n) + r; for BOOT it is found by walking the column.
 *
 * THE PERMUTATION of an epoch is a bijection on [0, total) for a total the host never sees: a 6-round Feistel network with
 * cycle walking.  hb = max(1, ceil(bitlen(total - 1) / 2)), mask = (1 << hb) - 1; from x = m repeat
 *     (l, r) = (x >> hb, x & mask)
 *     for i = 0 .. 5:  (l, r) = (r, l ^ (mix(ek + (i + 1) * 0x9E3779B97F4A7C15 + r) & mask))
 *     x = (l << hb) | r
 * until x < total; perm(m) = x.  mix is splitmix64's finaliser and all sums are modulo 2^64.  The walk ends: x runs along the
 * cycle of a permutation of [0, 2^(2 hb)) that holds m.  The key is ek = SM(base[which], calls[which]), base[which] =
 * SM(seed, which), SM(s, i) = mix(s + (i + 1) * 0x9E3779B97F4A7C15) the i-th output of splitmix64 seeded with s (the replay
 * sampler's).  calls[which] counts the selects of that list since create, so the order of an epoch is a pure integer function of
 * (seed, which, the number of selects before it, total).
 */
#ifndef AGX_MINIBATCH_H
#define AGX_MINIBATCH_H

#include "agx_history.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_MB_LIMIT 4096   /* L: the limit of a gathered rollout */
#define AGX_MB_LIVE 0       /* which: the slots that hold a transition */
#define AGX_MB_BOOT 1       /* which: the live slots whose return bootstraps from the learner's V(next_index) */
#define AGX_MB_STREAMS 8    /* f32 streams of one take */

typedef struct agx_minibatch agx_minibatch;

/*
 * A minibatcher on `h` (which supplies N, the device and the error channel).  One small device allocation - off i32 [2][N + 1],
 * cnt i32 [N], state u64 [2][3] (base, calls, the key in flight, per list) - seeded here: calls = 0 and both totals 0.
 * Destroy it before the history.  AGX_E_INVALID: a null h or out.
 */
AGX_API int agx_minibatch_create(agx_history *h, uint64_t seed, agx_minibatch **out);
AGX_API int agx_minibatch_destroy(agx_minibatch *mb);

/*
 * Start an epoch over list `which` of the rollout (d_len i32 [N], d_ends u8 [L][N]): writes off and total, publishes the key
 * ek of this epoch and advances calls[which].  It is the only launch that writes the state, so a replayed graph shuffles anew.
 * d_total (i32 [1], may be NULL) receives total.  d_ends is read only for AGX_MB_BOOT and may be NULL for AGX_MB_LIVE.
 * AGX_E_INVALID: a null handle, a bad which, L outside 1 .. AGX_MB_LIMIT, L * N above INT32_MAX, a null d_len (or d_ends for
 * AGX_MB_BOOT) - in this order.
 */
AGX_API int agx_minibatch_select(agx_minibatch *mb, int which, int32_t L, const int32_t *d_len, const uint8_t *d_ends,
                                 int32_t *d_total, void *stream);

/*
 * What one take reads and writes.  A plain struct in host memory, read at call time.
 *     in     d_obs_index, d_next_index  i64 [L][N]      each may be NULL (its output then holds -1)
 *            d_payload                  u8  [L][N][W]   W = payload_bytes; NULL reads as zeros; W = 0: no payload
 *            src_f32[0 .. n_f32)        f32 [L][N]      0 <= n_f32 <= AGX_MB_STREAMS
 *     out    d_slot                     i32 [S]         required: the slot element e, -1 where none
 *            d_env                      i32 [S]         n
 *            d_obs_index_out, d_next_index_out  i64 [S]
 *            d_payload_out              u8  [S][W]
 *            dst_f32[0 .. n_f32)        f32 [S]         stream k; a NULL src_f32[k] reads as 0, a NULL dst_f32[k] is skipped
 *            d_valid                    u8  [S]
 * Every output but d_slot may be NULL.  (d_env, d_obs_index_out) and (d_env, d_next_index_out) are samples for
 * agx_history_observe.
 */
typedef struct agx_minibatch_io {
    const int64_t *d_obs_index, *d_next_index;
    const void *d_payload;
    int32_t payload_bytes, n_f32;
    const float *src_f32[AGX_MB_STREAMS];
    int32_t *d_slot, *d_env;
    int64_t *d_obs_index_out, *d_next_index_out;
    void *d_payload_out;
    float *dst_f32[AGX_MB_STREAMS];
    uint8_t *d_valid;
} agx_minibatch_io;

/*
 * Rows of list `which` for the positions p = first .. first + S - 1 of the epoch the last select of that list started, one
 * launch.  d_len and d_ends are the arrays that select saw.  Row p - first of every output receives the slot at list position
 *     m = p mod total, and m = perm(m) where `permute` is not 0
 * and valid = 1 iff p < total and the slot was found.  Positions past total wrap on purpose: the row then holds a real, finite
 * sample with valid = 0, so a learner that multiplies by valid never meets an uninitialised row.  With total == 0, or where the
 * slot is not found, the row is slot = -1, env = 0, indices -1, zeros, valid = 0.  A slot is not found when the caller passes
 * other len / ends than select saw, so that the r-th selected slot of the env does not exist: invalid rather than wrong, and
 * nothing outside [L][N] is ever loaded.  Every element of every output that is passed is written.
 * AGX_E_INVALID: a null handle, a bad which, L outside 1 .. AGX_MB_LIMIT or L * N above INT32_MAX, S < 0 or first < 0 or
 * first + S above INT32_MAX, a null io or n_f32 outside 0 .. AGX_MB_STREAMS, a null d_len, d_ends (for AGX_MB_BOOT) or d_slot - in
 * this order.  S == 0 returns AGX_OK with no launch.
 */
AGX_API int agx_minibatch_take(agx_minibatch *mb, int which, int permute, int32_t L, const int32_t *d_len, const uint8_t *d_ends,
                               int32_t first, int32_t S, const agx_minibatch_io *io, void *stream);

/*
 * d_dst[d_slot[i]] = d_src[i] for the rows i < S with d_valid[i] != 0 and 0 <= d_slot[i] < L * N; every other row is skipped and
 * the rest of d_dst (f32 [L][N]) is left as it is.  With the rows of one epoch of the BOOT list this puts the critic's values into a zeroed d_boot_value: the valid slots of an epoch are
 * distinct, so no two rows write the same element.
 * AGX_E_INVALID: a null handle, L outside 1 .. AGX_MB_LIMIT or L * N above INT32_MAX, S < 0, a null d_slot, d_valid, d_src or d_dst - in
 * this order.  S == 0 returns AGX_OK with no launch.
 */
AGX_API int agx_minibatch_scatter(agx_minibatch *mb, int32_t S, const int32_t *d_slot, const uint8_t *d_valid, const float *d_src,
                                  int32_t L, float *d_dst, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_MINIBATCH_H */
