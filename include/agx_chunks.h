/*
 * agx_chunks.h — device-side minibatches of CHUNKS on a gathered on-policy rollout, for a recurrent learner (recurrent PPO):
 * every env's live range cut into runs of C consecutive steps, the list of the runs that hold a live step, a seeded permutation
 * of that list, and one launch per minibatch that writes everything the learner reads for S chunks, time-major [C][S], at fixed
 * shapes and with defined padding.
 *
 * Why: the minibatcher shuffles single slots, which destroys the time order an LSTM or GRU is trained over.  A recurrent learner
 * shuffles whole runs of steps instead, and has to know three things the rollout gather already resolved: where an env's live
 * range starts inside a run, where an episode ended inside a run (the hidden state restarts there), and which observation's stored
 * hidden state opens the run.  Done on the host that is a reshape, a nonzero() - the count is data, so the host waits for it - a
 * host-made permutation and a dozen indexed reads per epoch.
 *
 * Exported by libagx.so next to the other headers; their structs, entry points and the ABI version are unchanged.  Errors are
 * reported through agx_last_error of the history's context (agx_last_error(NULL) when there is none).  Every call except create
 * and destroy only enqueues on `stream`: no allocation, no synchronisation, no host copy, stream-capture safe.  AGX_E_STATE
 * while agx_env_range is narrowed.
 *
 * LAYOUT.  Every per-slot input is the rollout gather's: time-major [L][N], slot element e = t * N + n, N the context's num_envs;
 * t = L - 1 is the newest slot.  1 <= L <= AGX_CHUNK_L_LIMIT and L * N <= INT32_MAX.  d_len is [N].  The chunk length is C,
 * 1 <= C <= AGX_CHUNK_LIMIT and C <= L, and G = ceil(L / C).  Chunk g of env n covers the slots t = g * C + l, l = 0 .. C - 1; a
 * step with t >= L is padding (only in chunk G - 1, when C does not divide L).
 *
 * THE RULE.  With len' = clamp(len[n], 0, L) as in the folds and t0 = L - len':
 *     step (g, l) is LIVE      iff t0 <= t < L;
 *     chunk g     is SELECTED  iff len' > 0 and g >= t0 / C (integer division): it holds a live step.
 * So count(n) = len' > 0 ? G - t0 / C : 0, and the r-th selected chunk of env n is g = t0 / C + r: a closed form, no column walk.
 * Inside a selected chunk first = max(t0 - g * C, 0) is its first live step and steps = min((g + 1) * C, L) - max(g * C, t0) >= 1
 * the number of its live steps, l = first .. first + steps - 1.
 * THE LIST is env-major: env 0's selected chunks by ascending g, then env 1's, and so on.  With off[0 .. N] the exclusive prefix
 * sum of count and total = off[N] <= N * G, position m is (n, r) with off[n] <= m < off[n + 1], r = m - off[n].
 *
 * THE PERMUTATION of an epoch is the minibatcher's, unchanged: a 6-round Feistel network on 2 * hb bits with cycle walking,
 * hb = max(1, ceil(bitlen(total - 1) / 2)), keyed by ek = SM(base, calls), base = SM(seed, AGX_CHUNK_LIST), SM(s, i) the i-th output
 * of splitmix64 seeded with s.  List number 2 continues behind the minibatcher's lists 0 (LIVE) and 1 (BOOT), so a chunker and a
 * minibatcher of the same seed shuffle independently.  calls counts the selects since create: the order of an epoch is a pure
 * integer function of (seed, the number of selects before it, total).
 *
 * THE `ends` BYTE, as the rollout gather writes it; this header reads these bits, by value:
 *     1, 2, 4  the episode ended (terminated, truncated) or was cut behind this step: with (e & 7) != 0 at slot t - 1, step t
 *              starts an episode;
 *     8        the return bootstraps behind this step.  It is copied to d_ends_out with the rest of the byte and not interpreted.
 */
#ifndef AGX_CHUNKS_H
#define AGX_CHUNKS_H

#include "agx_history.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_CHUNK_LIMIT 256         /* C: the longest chunk */
#define AGX_CHUNK_L_LIMIT 4096      /* L: the limit of a gathered rollout */
#define AGX_CHUNK_LIST 2            /* the list number in the key: behind the minibatcher's 0 and 1 */
#define AGX_CHUNK_STREAMS 8         /* f32 streams of one take */
#define AGX_CHUNK_START_CHUNK 1     /* d_start: the first live step of the row's chunk */
#define AGX_CHUNK_START_EPISODE 2   /* d_start: the step behind an episode's end or a cut */

typedef struct agx_chunks agx_chunks;

/*
 * A chunker on `h` (which supplies N, the device and the error channel).  One small device allocation - off i32 [N + 1], state
 * u64 [3] (base, calls, the key in flight) and i32 [3] (total, L, C as the last select saw them) - seeded here: calls = 0,
 * total = L = C = 0, so a take before the first select writes null rows.  Destroy it before the history.
 * AGX_E_INVALID: a null h or out.
 */
AGX_API int agx_chunks_create(agx_history *h, uint64_t seed, agx_chunks **out);
AGX_API int agx_chunks_destroy(agx_chunks *c);

/*
 * Start an epoch over the chunks of the rollout (d_len i32 [N]): writes off and total, records (L, C), publishes the key ek of
 * this epoch and advances calls.  It is the only launch that writes the state, so a replayed graph shuffles anew.  d_total (i32
 * [1], may be NULL) receives total.
 * AGX_E_INVALID: a null handle, L outside 1 .. AGX_CHUNK_L_LIMIT or L * N above INT32_MAX, C outside 1 .. min(L, AGX_CHUNK_LIMIT),
 * a null d_len - in this order.
 */
AGX_API int agx_chunks_select(agx_chunks *c, int32_t L, int32_t C, const int32_t *d_len, int32_t *d_total, void *stream);

/*
 * What one take reads and writes.  A plain struct in host memory, read at call time.
 *     in     d_obs_index, d_next_index  i64 [L][N]      each may be NULL (its output then holds -1)
 *            d_payload                  u8  [L][N][W]   W = payload_bytes; NULL reads as zeros; W = 0: no payload
 *            src_f32[0 .. n_f32)        f32 [L][N]      0 <= n_f32 <= AGX_CHUNK_STREAMS
 *     out, per step, time-major [C][S], element l * S + s:
 *            d_slot                     i32             required: the slot element t * N + n at a live step, -1 otherwise
 *            d_env                      i32             n at EVERY step of the row, padding included
 *            d_obs_index_out, d_next_index_out  i64     -1 at a step that is not live, and where the input is NULL
 *            d_payload_out              u8  [C][S][W]   zeros at a step that is not live
 *            dst_f32[0 .. n_f32)        f32             stream k; 0 at a step that is not live; a NULL src_f32[k] reads as 0, a
 *                                                       NULL dst_f32[k] is skipped
 *            d_ends_out                 u8              the slot's ends byte; 0 at a step that is not live
 *            d_start                    u8              AGX_CHUNK_START_CHUNK iff l == first: the learner loads the hidden state
 *                                                       it stored for (env, state_index) there; AGX_CHUNK_START_EPISODE iff the
 *                                                       step is live, t > t0 and ends[t - 1][n] & 7: the learner restarts from its
 *                                                       initial state.  Both may be set.  0 at a step that is not live
 *            d_mask                     u8              1 iff the step is live AND the row is valid: the loss mask
 *     out, per chunk, [S]:
 *            d_chunk                    i32             g, -1 where none
 *            d_first, d_steps           i32
 *            d_state_index              i64             obs_index[g * C + first][n]; -1 where d_obs_index is NULL
 *            d_valid                    u8
 * Every output but d_slot may be NULL.  (d_env, d_obs_index_out), flattened, are samples for agx_history_observe, which leaves
 * an index of -1 untouched.
 */
typedef struct agx_chunks_io {
    const int64_t *d_obs_index, *d_next_index;
    const void *d_payload;
    int32_t payload_bytes, n_f32;
    const float *src_f32[AGX_CHUNK_STREAMS];
    int32_t *d_slot, *d_env;
    int64_t *d_obs_index_out, *d_next_index_out;
    void *d_payload_out;
    float *dst_f32[AGX_CHUNK_STREAMS];
    uint8_t *d_ends_out, *d_start, *d_mask;
    int32_t *d_chunk, *d_first, *d_steps;
    int64_t *d_state_index;
    uint8_t *d_valid;
} agx_chunks_io;

/*
 * Rows for the positions p = first .. first + S - 1 of the epoch the last select started, one launch.  d_len is the array that
 * select saw, d_ends u8 [L][N] the gather's ends bytes.  Row s = p - first receives the chunk at list position
 *     m = p mod total, and m = perm(m) where `permute` is not 0
 * and valid = 1 iff p < total, the (L, C) passed equal those select recorded, and the chunk is found under the d_len passed:
 * len' > 0 and t0 / C + r < G.  Positions past total wrap on purpose: the row then holds a real chunk with real, finite values,
 * slot >= 0 at its live steps, and valid = 0 and mask = 0 everywhere, so a learner that multiplies by mask never meets an
 * uninitialised row.  With total == 0, another (L, C) than select recorded, or a chunk that is not found, the row is the NULL ROW:
 * per step slot -1, env 0, indices -1 and zeros in every other output; per chunk chunk = -1, first = steps = 0, state_index = -1,
 * valid = 0.  Invalid rather than wrong: nothing outside [L][N] is ever loaded.  Every element of every output that is passed is
 * written, so no output needs a memset.
 * AGX_E_INVALID: a null handle, L outside 1 .. AGX_CHUNK_L_LIMIT or L * N above INT32_MAX, C outside 1 .. min(L, AGX_CHUNK_LIMIT),
 * S < 0 or first < 0 or first + S above INT32_MAX or C * S above INT32_MAX, a null io or n_f32 outside 0 .. AGX_CHUNK_STREAMS, a
 * null d_len, a null d_ends or d_slot - in this order.  S == 0 returns AGX_OK with no launch.
 */
AGX_API int agx_chunks_take(agx_chunks *c, int permute, int32_t L, int32_t C, const int32_t *d_len, const uint8_t *d_ends,
                            int32_t first, int32_t S, const agx_chunks_io *io, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_CHUNKS_H */
