/*
 * agx_glimpse.h — a glimpse memory on the frame history: the elementwise maximum of an env's last P observations.
 *
 * Why: active-vision agents do not feed one foveal observation to the network; they keep the last few glimpses of the
 * episode and combine them into one image (a persistence-of-vision memory, usually the elementwise maximum, P around 3).
 * The frame history (agx_history.h) already holds what such a memory is made of - the u8 frame and the fov_loc of every
 * retained env-step, and the age that says where the episode began - so one kernel reads the P small windows per
 * stacked frame and writes the combined observation once, instead of P observation batches and P - 1 reduction passes.
 *
 * Exported by libagx.so next to agx.h, agx_loop.h, agx_hostout.h and agx_history.h; those headers, their structs and the
 * ABI version are unchanged.  Errors are reported through agx_last_error of the history's context.
 *
 * Scope: what the history serves, narrowed to AGX_KIND_FIXED contexts in mask-out or resize_to_full mode (a maximum over
 * raw crops taken at different positions means nothing), every AGX_OBS_* type.
 */
#ifndef AGX_GLIMPSE_H
#define AGX_GLIMPSE_H

#include "agx_history.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_GLIMPSE_LIMIT 8

/*
 * The glimpse memory of B samples b = (env d_env[b], index d_index[b]) into d_obs, [B] rows of agx_obs_shape in the
 * context's AGX_OBS_* element type.
 *     Glimpse i (0 = the newest) of a sample (n, k) is the observation of (n, k - i) exactly as
 *     agx_history_observe(AGX_HIST_FOVEA, d_action = NULL) defines it: the stack that was in the ring after that ingest,
 *     seen at the fov_loc recorded for k - i.  It is TAKEN when
 *         i <= age[k]                  no AGX_CMD_CLEAR lies between the two appends: the same episode, and
 *         (n, k - i) is a valid sample by the history's own rule: every row it needs is still retained.
 *     Both conditions only get harder with i: the taken glimpses are 0 .. d_taken[b] - 1.
 *     The output is the elementwise maximum over the taken glimpses, rounded once at the store.  No observation value is
 *     negative and a maximum rounds nothing, so it equals BIT FOR BIT the maximum of the observations the steps
 *     themselves returned for those env-steps, in every element type.  glimpses = 1 is agx_history_observe bit for bit.
 *     The sample is valid iff (n, k) is, i.e. glimpse 0 is taken.  An invalid sample gets d_taken[b] = 0 and its d_obs /
 *     d_fov_loc rows are left untouched.  A glimpse that was evicted is not an error: d_taken[b] says how many were
 *     taken, and a caller who wants a full memory compares it with min(glimpses, age + 1).
 * d_fov_loc (i32 [B][glimpses][2], may be NULL): the position of glimpse i, untouched where not taken.  d_taken (u8 [B],
 * may be NULL).  Samples may repeat and come in any order.  B = 0: AGX_OK, no launch.
 * AGX_E_INVALID: glimpses outside 1 .. AGX_GLIMPSE_LIMIT, B < 0, a null buffer with B > 0.  AGX_E_STATE: a base context,
 * a fixed context in raw-crop mode, while agx_env_range is narrowed, or where glimpses windows plus the resize buffers
 * exceed the 160 KiB of LDS a workgroup can take.
 * Only enqueues on `stream`: no allocation, no synchronisation, no host copy.
 */
AGX_API int agx_history_observe_memory(agx_history *h, int32_t glimpses, const int32_t *d_env, const int64_t *d_index,
                                       int32_t B, float *d_obs, int32_t *d_fov_loc, uint8_t *d_taken, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_GLIMPSE_H */
