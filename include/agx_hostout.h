/*
 * agx_hostout.h — host (NumPy-side) observations at full duplex: launches over a range of envs, and a step of the
 * native loop that returns its observations in caller-owned pinned host memory, pipelined by env chunk.
 *
 * Why: with host outputs a step is a serial chain - emulators -> H2D of the screens -> kernels -> D2H of the
 * observations - and PCIe carries traffic in one direction at a time.  agx_loop_step_host cuts the batch into env
 * chunks so that chunk c's observations cross the link device-to-host while chunk c + 1's screens cross it
 * host-to-device and its kernels run.  What that needs from the kernels is a launch over a
 * range of envs: agx_env_range.
 *
 * Everything here is exported by libagx.so next to include/agx.h and include/agx_loop.h; those two headers, their
 * structs and the ABI version are unchanged.
 */
#ifndef AGX_HOSTOUT_H
#define AGX_HOSTOUT_H

#include "agx_loop.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Most chunks agx_loop_step_host cuts a step into (more are clamped; so is chunks > num_envs). */
#define AGX_HOSTOUT_MAX_CHUNKS 64

/*
 * Until changed, these entry points act on envs [lo, lo + n) only and leave every other env's ring, head, fov state
 * and output rows untouched:
 *     agx_ingest, agx_ingest_gray_raw, agx_ingest_compact, agx_ingest_gray_raw_compact, agx_ingest_gray,
 *     agx_observe_full, agx_fovea_fixed, agx_fovea_peripheral, agx_fovea_flexible, agx_fovea_reset.
 * Pointer arguments keep their meaning: they are the whole-batch arrays, indexed by absolute env, so a caller passes
 * the same pointers for every range.  (0, num_envs) is the state after agx_create and restores whole-batch launches.
 * No alignment of lo is required: every per-env array is a whole number of its elements per env, and the one byte
 * array (cmd) is read through an aligned-down dword load that stays inside the array.
 *
 * Contract: walking a partition of [0, num_envs) in ascending order, one call of an entry point per range, leaves
 * bit for bit what one whole-batch call leaves (ring, heads, fov state, observations).  The ring head and the fov
 * state are double-buffered and flip on every call: a range call carries the out-of-range envs' entries over to the
 * buffer it flips to, so every env's state is current after every call.
 *
 * While the range is not the whole batch, agx_step_fixed, agx_fovea_flexible_packed, agx_step_flexible_packed and
 * agx_ingest_rgb return AGX_E_STATE (the packed forms scan across all envs).  A colour (AGX_FRAME_RGB) context takes
 * no range other than the whole batch: AGX_E_STATE.  lo < 0, n < 1 or lo + n > num_envs: AGX_E_INVALID.
 * agx_get_stack_u8 / agx_set_stack_u8 / agx_get_fov_state / agx_set_fov_state always act on the whole batch.
 */
AGX_API int agx_env_range(agx_ctx *ctx, int32_t lo, int32_t n);

/*
 * The chunk partition agx_loop_step_host uses: c = min(chunks, num_envs, AGX_HOSTOUT_MAX_CHUNKS) ranges, ascending,
 * covering [0, num_envs) exactly, the first num_envs % c of them one env longer.  lo[] / n[] receive c entries each
 * (room for min(chunks, AGX_HOSTOUT_MAX_CHUNKS)); returns c, or AGX_E_INVALID (null pointer, num_envs < 1, chunks < 1).
 * Pure host arithmetic: no context, no HIP call.
 */
AGX_API int agx_hostout_partition(int32_t num_envs, int32_t chunks, int32_t *lo, int32_t *n);

/*
 * agx_loop_step with host observations.  Arguments as agx_loop_step, plus
 *     h_obs       caller-owned PINNED host memory, [N] observation rows of the context's element type;
 *     h_fov_loc   host i32 [N][2] (fovea kinds; pinned for an asynchronous copy), h_fov_res likewise (flexible kind);
 *     chunks      >= 1.
 * Per chunk: H2D of its screens on the loop's copy stream -> range ingest + range observation on `stream` -> D2H of
 * its observation and fov rows on the loop's one device-to-host stream; then the whole-batch autoreset tail of
 * agx_loop_step; then D2H of the k terminal rows to loop-owned pinned side buffers (agx_loop_host_final) and of the k
 * re-observed rows into their rows of h_obs, behind the chunk copies.  d_obs / d_fov_loc / d_fov_res receive what
 * agx_loop_step would have left in them.
 * The call returns when everything is enqueued; nothing synchronises the device.  h_obs, h_fov_loc, h_fov_res and the
 * side buffers are complete after agx_loop_host_wait.  The side buffers alternate between two sets: they stay valid
 * until the step after next.  Call agx_loop_host_wait before any other loop call that writes d_obs.
 * Null loop / motor / d_obs / res / h_obs, a missing h_fov_loc (fovea) or h_fov_res (flexible) or chunks < 1:
 * AGX_E_INVALID, before any HIP call.
 */
AGX_API int agx_loop_step_host(agx_loop *loop, const int32_t *motor, const void *d_action, int action_dtype,
                               const int32_t *d_action_type, float *d_obs, int32_t *d_fov_loc, int32_t *d_fov_res,
                               agx_loop_result *res, void *stream, void *h_obs, int32_t *h_fov_loc, int32_t *h_fov_res,
                               int chunks);

/* Allocates what agx_loop_step_host needs beyond the loop's own staging, so that no step does: the d2h stream, the events for
 * `chunks` chunks and the two pinned side sets - 2 x [N] observation rows (231 MB at N = 1024 float32 84 x 84 x 4) plus
 * 2 x 2 x [N][2] i32 for the fovea kinds.  Pinned by the calling thread: call it where agx_loop_create is called (bound to the
 * CPUs of the GPU's NUMA node).  A loop that was not prepared allocates the same inside its first agx_loop_step_host. */
AGX_API int agx_loop_host_prepare(agx_loop *loop, int chunks);

/* Blocks until the host copies of the last agx_loop_step_host have landed (no-op if there was none). */
AGX_API int agx_loop_host_wait(agx_loop *loop);

/* Host twins of res->d_final_obs / d_final_loc / d_final_res of the last agx_loop_step_host: [n_done] rows in pinned
 * memory owned by the loop, NULL where the device pointer is NULL.  Complete after agx_loop_host_wait. */
AGX_API int agx_loop_host_final(agx_loop *loop, const void **h_final_obs, const int32_t **h_final_loc,
                                const int32_t **h_final_res);

#ifdef __cplusplus
}
#endif
#endif /* AGX_HOSTOUT_H */
