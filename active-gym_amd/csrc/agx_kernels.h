// agx_kernels.h — gfx950 device code of the observation pipeline (HBM-bound
// byte/float streaming work: no MFMA anywhere, there is no dense contraction).
//
//   k_ingest            K1  RGB -> ALE luminance -> OpenCV fixed-point bilinear -> 2-frame max -> u8 ring slot
//   k_ingest_gray       K1' same append from already obs-sized gray frames
//   k_ingest_rgb        K1b DMC front end: obs-sized RGB -> cv2 BGR2GRAY fixed point -> ring slot (no max, no resize)
//   k_ingest_rgb_planar K1c colour DMC front end (AGX_FRAME_RGB): obs-sized RGB -> three planar ring planes
//   k_stack_u8 / k_full K0  ring -> stack order (u8 / f32 k/255)
//   k_fovea_fixed       K2  clip/rint sensory action, crop, {raw | mask-out | bilinear upsample}
//   k_fovea_generic     K3/K4 peripheral squeeze-expand + paste, flexible (ragged) fovea
//   k_history_push / k_history_observe  K5  frame history: append the newest ring frame / re-create a retained observation
//   k_history_memory    K6  glimpse memory: the elementwise max of a sample's last P re-created observations
//   k_replay_scan / k_replay_draw / k_replay_inspect  K7  replay sampler: draw accepted (env, index) pairs of the history
//   k_steplog_record / k_steplog_gather  K8  step log: reward / flags / payload rows, n-step returns of drawn samples
//   k_priority_weights / _chunks / _scan / _draw / _update / _lookup  K9  prioritized sampler: draw proportionally to a priority
//   k_history_observe_shifted / k_shift_draw  K10  random-shift augmentation: a retained observation moved by a drawn shift
//   k_sequence_gather / k_sequence_observe  K11  sequence replay: L consecutive steps of one episode per sample, padded with zeros
//   k_rollout_gather / k_slot_fold<GaeFold>  K12  on-policy rollouts: the last L transitions of every env, cut at episode ends, and GAE
//   k_slot_fold<VtraceFold>  K13 V-trace targets and policy-gradient advantages over a gathered rollout, for actor-learner training
//   k_mb_count / k_mb_scan / k_mb_take / k_mb_scatter  K15  minibatches on a gathered rollout: its LIVE / BOOT slot lists, shuffled
//   k_retrace_direct  K16  Retrace-family Q-returns folded backward along the sequences of a sequence-replay batch
//   k_chunk_scan / k_chunk_take  K17  minibatches of chunks of consecutive steps on a gathered rollout, for recurrent learners
//
// The fixed fovea's phases are stated once in agx_fixed_phases.h (K2, K5, K6, K10, K11 run them).  The three kernels that re-create
// observation planes from history rows - k_history_observe, k_history_observe_shifted, k_sequence_observe - are one body,
// agx_hist_plane.h (sample resolution, source row, position, plane write), under their own indexing and shift policy; the
// validity rule of a history sample is agx_hist_rule.h's.  The backward folds over a gathered rollout - GAE and V-trace - are one kernel,
// agx_slot_fold.h's k_slot_fold, under a policy each (streams, step, outputs, set depth).
//
// Persistent per-env state (owned by the context, see agx_api.hip):
//   ring  u8 [N][fs][oh][ow]   numerators k of the reference's float32 k/255 frames
//   head  i32[2][N]            next slot to write == oldest frame; double-buffered so that the
//                              several workgroups of one env all read the pre-launch value
//   loc   i32[2][N][2], res i32[2][N][2]   fov_loc / fov_res, double-buffered for the same reason
#pragma once
#include "agx_common.h"
#include "agx_k0_stack.h"
#include "agx_k1_ingest.h"
#include "agx_fov_common.h"
#include "agx_k2_fixed.h"
#include "agx_k5_history.h"
#include "agx_k6_glimpse.h"
#include "agx_k7_replay.h"
#include "agx_k8_steplog.h"
#include "agx_k9_priority.h"
#include "agx_k10_augment.h"
#include "agx_k11_sequence.h"
#include "agx_k12_rollout.h"
#include "agx_k13_vtrace.h"
#include "agx_k34_resample.h"
#include "agx_k3_per3.h"
#include "agx_k4_flex3.h"
#include "agx_k4_raw3.h"
#include "agx_k14_step_packed.h"
#include "agx_k15_minibatch.h"
#include "agx_k16_retrace.h"
#include "agx_k17_chunks.h"
#ifdef AGX_EXPERIMENTS
#include "experiments/agx_experiments.h"   // measured dead ends: tools/ and the variants test only, never in libagx.so
#include "experiments/agx_packed_wave.h"
#include "experiments/agx_retrace_tiled.h"
#endif
