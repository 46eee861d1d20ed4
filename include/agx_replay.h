/*
 * agx_replay.h — a device-side replay sampler on the frame history: draw -> observe -> learn without the host seeing a count.
 *
 * Why: a replay buffer on the frame history (agx_history.h) keeps (env, index) pairs and has agx_history_observe /
 * agx_history_observe_memory re-create the observations.  Which pairs are worth asking for depends on state only the device
 * holds: the per-env append counts and the age byte of every row (what is still retained, where an episode began).  A caller
 * who draws indices blind gets holes, transitions that straddle a reset, and glimpse memories that are not full; a caller who
 * reads the counts back breaks the rule that every call only enqueues.  The sampler draws on the device, by rejection, only
 * pairs that satisfy all of that, as a pure integer function of (seed, call number) any binding can reproduce.
 *
 * Exported by libagx.so next to agx.h, agx_loop.h, agx_hostout.h, agx_history.h and agx_glimpse.h; those headers, their structs
 * and the ABI version are unchanged.  Errors are reported through agx_last_error of the history's context (agx_last_error(NULL)
 * when there is none).  The sampler serves what the history serves.  Every call except create / destroy only enqueues on
 * `stream`: no allocation, no synchronisation, no host copy, stream-capture safe.  AGX_E_STATE while agx_env_range is narrowed.
 *
 * ACCEPTED SAMPLES.  With cnt = count[n], age[k] the age byte of row k of env n, (n, k) is accepted iff all three hold:
 *     1. (n, k) is valid by the history's own rule (agx_history_observe).
 *     2. With b = min(back, age[k]), (n, k - b) is valid by that rule.  Validity of (n, k - i) only gets harder with i, so
 *        glimpses 0 .. b of k are all taken: a glimpse memory (agx_glimpse.h) of back + 1 glimpses at k is full,
 *        taken == min(back + 1, age[k] + 1).
 *     3. k + forward < cnt and age[k + forward] >= forward: no AGX_CMD_CLEAR lies in (k, k + forward], the same episode.
 * What follows:
 *     (n, k + f) is valid for every f <= forward: its oldest needed row is k + f - min(age[k] + f, fs - 1), which is never
 *     older than the one k needs (ages count up by one per append inside an episode; a saturated age of 255 exceeds fs - 1
 *     and back either way).
 *     The memory of back + 1 glimpses at k + forward is full as well: its oldest glimpse is k + forward - min(back,
 *     age[k] + forward), which is k - b or younger.
 *     With forward = 1 the pair (k, k + 1) is a transition of one episode: k + 1 is never a reset observation.  (An autoreset
 *     pushes the terminal observation and then the reset observation; the terminal one may be k + 1, the reset one not.)
 *
 * THE DRAW.  mix is splitmix64's finaliser,
 *     mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 *     SM(s, i) = mix((s + (i + 1) * 0x9E3779B97F4A7C15) mod 2^64)      the i-th output of splitmix64 seeded with s
 *     (s = 1234567 gives 6457827717110365317, 3203168211198807973, 9817491932198370423 for i = 0, 1, 2).
 * Per call: key = SM(seed, calls); then calls += 1, on the device, by the call's first launch - a captured graph draws fresh
 * samples at every replay.  Candidates of env n: lo_n = max(cnt - T, 0), L_n = max(cnt - forward - lo_n, 0); off is the
 * exclusive prefix sum of L in i64, total = off[N].  Sample b, attempt a = 0 .. attempts - 1:
 *     z = SM(key, b * attempts + a)        (the index in 64 bits)
 *     u = (z * total) >> 64                (the high half of the 128-bit product)
 *     n = the env with off[n] <= u < off[n + 1],  k = lo_n + u - off[n]
 * and the first accepted attempt wins.  If none is, or total == 0: d_env[b] = -1, d_index[b] = -1, d_ok[b] = 0, and
 * agx_history_observe leaves that row untouched (env -1 is no env).  Every attempt is uniform over the candidates and
 * independent of the others, so rejection keeps the accepted draws uniform over the accepted set; the multiply-high map's
 * bias is at most total / 2^64.  A sample fails with probability (1 - accepted / total) ^ attempts.
 */
#ifndef AGX_REPLAY_H
#define AGX_REPLAY_H

#include "agx_history.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct agx_replay agx_replay;

#define AGX_REPLAY_SPAN_LIMIT    64   /* back, forward */
#define AGX_REPLAY_ATTEMPT_LIMIT 64

/*
 * A sampler on `h` for samples with `back` earlier glimpses and `forward` later appends of the same episode.  back and
 * forward in 0 .. AGX_REPLAY_SPAN_LIMIT, attempts in 1 .. AGX_REPLAY_ATTEMPT_LIMIT (0 means 16); anything else, or a null
 * argument, is AGX_E_INVALID.  Allocates the sampler's own scratch - offsets i64 [N + 1], state u64 [2] (seed, calls) and the
 * key of the call in flight - outside the history's block: agx_history_bytes is unchanged.  A new sampler has seed 0,
 * calls 0.  Destroy the sampler before its history.
 */
AGX_API int agx_replay_create(agx_history *h, int32_t back, int32_t forward, int32_t attempts, agx_replay **out);
AGX_API int agx_replay_destroy(agx_replay *r);

/* (seed, calls = 0), enqueued on `stream`; the seed travels by value. */
AGX_API int agx_replay_seed(agx_replay *r, uint64_t seed, void *stream);

/*
 * Draw B samples into d_env (i32 [B]) and d_index (i64 [B]); d_ok (u8 [B], may be NULL) says which were accepted and
 * d_total (i64 [1], may be NULL) receives total.  B is not bound by a grid dimension.  B = 0: AGX_OK, no launch, and the call
 * counter does not advance.  B < 0 or a null d_env / d_index with B > 0: AGX_E_INVALID.
 * The counts are read on `stream`: call on the stream that pushes, or order the calls against it.
 */
AGX_API int agx_replay_sample(agx_replay *r, int32_t B, int32_t *d_env, int64_t *d_index, uint8_t *d_ok, int64_t *d_total,
                              void *stream);

/*
 * What the sampler knows, for index lists the caller drew itself (no sampler needed): for sample b = (d_env[b], d_index[b])
 *     d_age[b]   = age[k] of a valid sample, -1 otherwise;
 *     d_ahead[b] = the number of later appends of the same episode already in the history: the largest f <= 255 with
 *                  k + f < cnt and no age == 0 in (k, k + f]; -1 for an invalid sample.  It is what an n-step target needs.
 * Either output may be NULL.  B = 0: AGX_OK, no launch.
 */
AGX_API int agx_replay_inspect(agx_history *h, const int32_t *d_env, const int64_t *d_index, int32_t B, int32_t *d_age,
                               int32_t *d_ahead, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_REPLAY_H */
