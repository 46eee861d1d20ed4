/*
 * agx_priority.h — a prioritized replay sampler on the frame history: draw proportionally to a priority, on the device, only
 * pairs that are retained, lie in one episode and have a full glimpse memory.  The sibling of agx_replay.h (the uniform draw).
 *
 * Why: learners of the Rainbow / Ape-X / R2D2 family draw proportionally to a priority and correct with importance weights.
 * Whether (env, index) may be drawn at all depends on the per-env append counts and the age byte of every row, which only the
 * device holds (agx_replay.h); and a priority table kept by the caller has to follow the row reuse `index mod T`, the two pushes
 * of an autoreset step and every eviction.  This table does that with a stamp per row, as the step log does (agx_steplog.h):
 * an index that reuses a row can never inherit the evicted index's priority.
 *
 * Exported by libagx.so next to agx.h, agx_loop.h, agx_hostout.h, agx_history.h, agx_glimpse.h, agx_replay.h and agx_steplog.h;
 * those headers, their structs, agx_history_bytes and the ABI version are unchanged.  Errors are reported through agx_last_error
 * of the history's context (agx_last_error(NULL) when there is none).  Every call except create / destroy only enqueues on
 * `stream`: no allocation, no synchronisation, no host copy, stream-capture safe.  AGX_E_STATE while agx_env_range is narrowed.
 * With no table created nothing of this runs: agx_history_push has no hook.
 *
 * THE TABLE.  Per history row (env n, row k mod T): stamp i64 (the index the weight was written for, -1: unset) and weight u32,
 * 12 bytes per env-step, and one device scalar wmax (u32), all in one allocation of the table's own.
 *
 * WEIGHTS are fixed point, so that every sum is exact.  quantise(p), p an f32:
 *     !(p > 0)  (zero, negative, NaN)                 -> 1
 *     q = p * 65536.0f  (one f32 multiply)
 *     q >= 4294967296.0f  (+inf included)             -> 0xFFFFFFFF
 *     otherwise                                       -> max((uint32_t)q, 1)      (truncation)
 * Priority 1.0 is weight 65536; no written row has weight 0.  wmax starts at 65536 and becomes the maximum of itself and every
 * weight written.  The effective weight of a retained (n, k) is weight[row] if stamp[row] == k, otherwise wmax - the value the
 * table holds when the reading call runs: a transition nobody has updated yet has the largest priority seen so far.
 *
 * ACCEPTED SAMPLES.  accepted(n, k) is the predicate of agx_replay.h, conditions 1 - 3, with this table's back / forward:
 *     1. (n, k) is valid by the history's own rule (agx_history_observe).
 *     2. With b = min(back, age[k]), (n, k - b) is valid by that rule.
 *     3. k + forward < cnt and age[k + forward] >= forward.
 * What follows from them is spelt out there.
 *
 * THE DRAW.  mix, SM as in agx_replay.h.  With cnt = count[n], lo_n = max(cnt - T, 0):
 *     W(n, k)  = accepted(n, k) ? effective_weight(n, k) : 0          for k = lo_n .. cnt - 1, else 0
 *     P(n, k)  = sum of W(n, j) for lo_n <= j < k                     (i64)
 *     off[n]   = sum of all W(m, .) for m < n,  total = off[N]        (i64; T * N < 2^31, so no sum overflows)
 *     key      = SM(seed, calls); then calls += 1, on the device, by the call's first launch - a captured graph draws fresh
 *                samples at every replay
 *     sample b:  z = SM(key, b);  u = (z * total) >> 64               (the high half of the 128-bit product)
 *                n = the env with off[n] <= u < off[n + 1];  v = u - off[n]
 *                k = the row of env n with P(n, k) <= v < P(n, k) + W(n, k)
 *     outputs:   d_env[b] = n, d_index[b] = k, d_ok[b] = 1, d_weight[b] = W(n, k)
 *     total == 0:  d_env[b] = -1, d_index[b] = -1, d_ok[b] = 0, d_weight[b] = 0 for every b
 *     d_total = total,  d_accepted = the number of (n, k) with W(n, k) > 0
 * One attempt per sample, no rejection: acceptance is folded into the weights, so W / total is the probability of a row up to
 * the multiply-high map's bias of at most total / 2^64, and a sample fails only on an empty accepted set.  The sums are
 * recomputed by every agx_priority_sample, in time proportional to T * N: membership changes with every push (eviction, new
 * rows at wmax, conditions 2 and 3 becoming true), and push has no hook.
 */
#ifndef AGX_PRIORITY_H
#define AGX_PRIORITY_H

#include "agx_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct agx_priority agx_priority;

/*
 * A table on `h` for samples with `back` earlier glimpses and `forward` later appends of the same episode; back and forward
 * in 0 .. AGX_REPLAY_SPAN_LIMIT.  Anything else, a null argument, or a history of T * N >= 2^31 rows is AGX_E_INVALID.
 * Allocates the table and the scratch of the draw outside the history's block.  A new table has every row unset, wmax 65536,
 * seed 0, calls 0.  Destroy the table before its history.
 */
AGX_API int agx_priority_create(agx_history *h, int32_t back, int32_t forward, agx_priority **out);
AGX_API int agx_priority_destroy(agx_priority *p);

/* Device bytes of the table's own allocation (table + scratch); AGX_E_INVALID for a null table. */
AGX_API int64_t agx_priority_bytes(const agx_priority *p);

/* (seed, calls = 0), enqueued on `stream`; the seed travels by value. */
AGX_API int agx_priority_seed(agx_priority *p, uint64_t seed, void *stream);

/* Every row unset, wmax back to 65536.  Call it with agx_history_clear: the history's indices restart there. */
AGX_API int agx_priority_clear(agx_priority *p, void *stream);

/*
 * Sample b = (d_env[b], d_index[b]) = (n, k) is written iff 0 <= n < N and max(count[n] - T, 0) <= k < count[n]: row k mod T
 * of env n gets stamp = k, weight = quantise(d_priority[b]), and wmax becomes the maximum of itself and every weight written.
 * Every other sample is skipped silently (-1 is how a caller skips one).  A sample that occurs more than once in one call
 * gets one of its weights; which one is unspecified.  B = 0: AGX_OK, no launch.
 */
AGX_API int agx_priority_update(agx_priority *p, const int32_t *d_env, const int64_t *d_index, const float *d_priority, int32_t B,
                                void *stream);

/* d_weight[b] (i64) = the effective weight of a retained (n, k), whatever its acceptance; -1 for anything else. */
AGX_API int agx_priority_lookup(agx_priority *p, const int32_t *d_env, const int64_t *d_index, int32_t B, int64_t *d_weight,
                                void *stream);

/*
 * Draw B samples into d_env (i32 [B]) and d_index (i64 [B]).  d_ok (u8 [B]), d_weight (i64 [B]), d_total (i64 [1]) and
 * d_accepted (i64 [1]) may be NULL.  B is not bound by a grid dimension.  B = 0: AGX_OK, no launch, and the call counter does
 * not advance.  B < 0 or a null d_env / d_index with B > 0: AGX_E_INVALID.
 * The counts are read on `stream`: call on the stream that pushes, or order the calls against it.
 */
AGX_API int agx_priority_sample(agx_priority *p, int32_t B, int32_t *d_env, int64_t *d_index, uint8_t *d_ok, int64_t *d_weight,
                                int64_t *d_total, int64_t *d_accepted, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_PRIORITY_H */
