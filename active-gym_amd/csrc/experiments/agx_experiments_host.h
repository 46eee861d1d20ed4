// agx_experiments_host.h - HOST side of the measured dead ends: the launch branches of the experiments build
// (-DAGX_EXPERIMENTS, libagx_exp.so) that agx_api.hip's shipped entry points hook with one guarded line each.  Included by
// agx_api.hip behind its helpers (agx_ctx, AGX_LAUNCH, ingest_params, fov_params, the with_* dispatchers); every function
// returns whether it took the call.  The knobs are agx_ctx::Tune's experiments members, read in agx_create.
#pragma once

namespace {

// agx_ingest: the opt-in forms of the RGB whole-screen ingest
bool exp_ingest(agx_ctx *ctx, const IngestParams &p, void *stream) {
    const agx_config &c = ctx->cfg;
    const int en = ctx->rng_n, bands = p.nbands;
    const size_t lds = ingest_lds(ctx->band_rows, c.obs_w);
    const int pipe_parts = ctx->tune.pipe_parts;
    // wave-private form: needs the affine row form, band_rows = 4 * RPW with RPW * ow/4 <= 64 lanes and
    // 2 frames * RPW rows * 40 pieces <= 240 (RPW <= 3)
    // (measured equal to the barrier form at N=1024 - 46.5 vs 45.6 us - so it is opt-in: AGX_INGEST_WAVE=1)
    const bool want_wave = ctx->tune.wave != 0;
    const int rpw = ctx->band_rows / 4;
    const bool wave_ok = want_wave && pipe_parts == 0 && ctx->ingest_t == 256 && ctx->k1.y_affine && ctx->band_rows % 4 == 0 &&
                         rpw >= 1 && rpw <= 3 && rpw * (c.obs_w / 4) <= 64;
    if (wave_ok) {
        const size_t slice = ((sizeof(int2) * c.obs_w + (size_t)2 * rpw * kRawW * 2) + 15) & ~(size_t)15;
        hipLaunchKernelGGL(k_ingest_wave, dim3(bands, en), dim3(256), 4 * slice, S(stream), p);
    } else if (pipe_parts > 0 && ctx->ingest_t == 256) {
        const int parts = std::min(pipe_parts, bands);
        const size_t lds2 = sizeof(int4) * c.obs_h + sizeof(int2) * c.obs_w + (size_t)2 * (2 * ctx->band_rows * 2 * kRawW);
        hipLaunchKernelGGL(k_ingest_pipe<256>, dim3(parts, en), dim3(256), lds2, S(stream), p);
    } else if (ctx->ingest_t == 128)
        hipLaunchKernelGGL(k_ingest<128>, dim3(bands, en), dim3(128), lds, S(stream), p);
    // (same box, N=1024: 37.5-37.9 us against 37.9-38.2 for the one-band form - K1 is VALU-issue- and HBM-limited, not
    //  limited by the load-free tail of a workgroup - so it stays opt-in)
    else if (ctx->tune.no_full == 0 && ctx->tune.pair12 != 0 && ctx->tune.band_rows == 0 && ctx->tune.ingest_t == 0 &&
             ctx->k1.y_affine && ctx->band_rows == 12 && c.obs_h % 12 == 0 && (c.obs_w / 4) * 12 <= kThreads)
        AGX_LAUNCH(0, k_ingest_pair12, dim3(bands, (en + 1) / 2), dim3(256), lds + (size_t)2 * 12 * 2 * kRawW, S(stream), p,
                   en);
    else return false;
    return true;
}

// agx_fovea_fixed: two physical slots per workgroup (whole launch resident at once, second frame's load hidden): measured a tie
// with the one-slot form at N=1024 (26.3 vs 25.8 us) - the launch is store-limited
bool exp_fovea_fixed(agx_ctx *ctx, const FovParams &p, void *stream) {
    const agx_config &c = ctx->cfg;
    if (!(c.out_mode == AGX_OUT_RESIZE && c.frame_stack % 2 == 0 && ctx->tune.pair == 1 && ctx->obs_type == AGX_OBS_F32 &&
          ctx->planes == 1))
        return false;
    const dim3 grid2(c.frame_stack / 2, ctx->rng_n), block(kThreads);
    with_geom(ctx->plan.headline, geom_r(c), [&](auto g) {
        hipLaunchKernelGGL((k_fovea_fixed2<decltype(g)>), grid2, block, fixed2_lds(c), S(stream), g, p);
        return 0;
    });
    return true;
}

// packed_crops_raw3: one wave per (slot, env) item: measured slower (docs/HISTORY.md, round 4)
bool exp_packed_crops_raw3(agx_ctx *ctx, const FlexRawParams &fr, const FovParams &p, void *stream) {
    const agx_config &c = ctx->cfg;
    if (ctx->tune.packed_wave == 0) return false;
    const dim3 grid(c.frame_stack, c.num_envs);
    with_geom(ctx->plan.headline, geom_r(c), [&](auto g) {
        AGX_LAUNCH(1, (k_fovea_flexible_raw3_wave<decltype(g)>), grid, dim3(64), ctx->plan.lds, S(stream), g, fr, p);
        return 0;
    });
    return true;
}

// ---- agx_step_fixed: the forms of the fused step that were built and measured slower or equal
// one launch, one workgroup per env (agx_step_env.h): the headline geometry's resize_to_full path
int exp_step_env(agx_ctx *ctx, const uint8_t *d_frames, const uint8_t *d_cmd, const void *d_action, int action_dtype, float *d_obs,
                 int32_t *d_fov_loc, void *stream) {
    const agx_config &c = ctx->cfg;
    DeviceGuard g(c.device);
    const IngestParams pi = ingest_params(ctx, d_frames, d_cmd);
    FovParams pf = fov_params(ctx, d_action, action_dtype, nullptr, nullptr, d_obs, d_fov_loc, nullptr);
    pf.cmd = d_cmd;
    pf.phase = 3;                                        // `head` is the pre-ingest head, every slot is processed
    pf.head = ctx->head[ctx->cur_head];
    const size_t team_lds = (std::max(ingest_lds(ctx->band_rows, c.obs_w), fixed_lds(c)) + 15) & ~(size_t)15;
    using GS = GeomS<84, 84, 30, 30>;
    StepEnvArgs sa;
    sa.pi = pi;
    sa.pf = pf;
    sa.team_lds = (int32_t)team_lds;
    sa.debug = env_int("AGX_STEP_ENV_DEBUG", 0);
    hipLaunchKernelGGL((k_step_env<GS>), dim3(c.num_envs), dim3(2 * kThreads), 2 * team_lds, S(stream), sa);
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_head ^= 1;
    ctx->cur_fov ^= 1;
    return AGX_OK;
}

// split step: the batch as P env ranges, range 0 on the caller's stream, the others on internal streams forked
// from it and joined back before the call returns its work to the caller's stream order.  One range's fovea stores
// and ingest drain then run under another range's ingest loads (reads and writes of the same step overlap), with
// the results of one launch pair bit for bit (same kernels, disjoint env ranges, no shared state).
int exp_step_split(agx_ctx *ctx, int parts, const uint8_t *d_frames, const uint8_t *d_cmd, const void *d_action, int action_dtype,
                   float *d_obs, int32_t *d_fov_loc, void *stream) {
    const agx_config &c = ctx->cfg;
    const agx_ctx::Tune &tn = ctx->tune;
    DeviceGuard g(c.device);
    if (!ctx->ev_fork) {
        int lo_p = 0, hi_p = 0;
        AGX_HIP(ctx, hipDeviceGetStreamPriorityRange(&lo_p, &hi_p));        // lo_p: least urgent (largest number)
        const int prio = tn.aux_prio > 0 ? hi_p : (tn.aux_prio < 0 ? lo_p : 0);
        for (int k = 0; k < 3; ++k) {
            AGX_HIP(ctx, ctx->own.stream(&ctx->aux[k], hipStreamNonBlocking, prio));
            AGX_HIP(ctx, ctx->own.event(&ctx->ev_join[k], hipEventDisableTiming));
        }
        AGX_HIP(ctx, ctx->own.event(&ctx->ev_fork, hipEventDisableTiming));
    }
    hipStream_t st[4] = {S(stream), ctx->aux[0], ctx->aux[1], ctx->aux[2]};
    AGX_HIP(ctx, hipEventRecord(ctx->ev_fork, st[0]));
    for (int k = 1; k < parts; ++k) AGX_HIP(ctx, hipStreamWaitEvent(st[k], ctx->ev_fork, 0));
    const size_t fsz = (size_t)c.obs_h * c.obs_w;
    const size_t obs_env = obs_row_bytes(ctx, c.out_mode == AGX_OUT_RAW) / sizeof(float);      // f32 observations only
    const bool full12 = ctx->k1.y_affine && ctx->band_rows == 12 && c.obs_h % 12 == 0;
    const size_t lds1 = ingest_lds(ctx->band_rows, c.obs_w);
    int n0[5];
    for (int k = 0; k <= parts; ++k) n0[k] = (int)((long long)c.num_envs * k / parts);
    const IngestParams pi0 = ingest_params(ctx, d_frames, d_cmd);
    for (int k = 0; k < parts; ++k) {
        IngestParams q = pi0;
        const size_t b = n0[k];
        q.frames += b * 2 * (size_t)kRawFrameBytes;
        q.cmd += b;
        q.ring += b * c.frame_stack * fsz;
        q.head_in += b;
        q.head_out += b;
        const dim3 grid(q.nbands, n0[k + 1] - n0[k]);
        if (full12) hipLaunchKernelGGL(k_ingest_full12_part, grid, dim3(kThreads), lds1, st[k], q);
        else hipLaunchKernelGGL(k_ingest_part, grid, dim3(kThreads), lds1, st[k], q);
    }
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_head ^= 1;
    const FovParams pf0 = fov_params(ctx, d_action, action_dtype, nullptr, nullptr, d_obs, d_fov_loc, nullptr);
    for (int k = 0; k < parts; ++k) {
        FovParams q = pf0;
        const size_t b = n0[k];
        q.ring += b * c.frame_stack * fsz;
        q.head += b;
        q.loc_in += 2 * b;
        q.loc_out += 2 * b;
        q.res_in += 2 * b;
        q.res_out += 2 * b;
        if (q.action) q.action = static_cast<const char *>(q.action) + b * action_stride(action_dtype);
        q.obs += b * obs_env;
        if (q.user_loc) q.user_loc += 2 * b;
        const dim3 grid(c.frame_stack, n0[k + 1] - n0[k]);
        with_mode(c.out_mode, [&](auto mode) {
            return with_geom(ctx->plan.headline, geom_r(c), [&](auto gm) {
                hipLaunchKernelGGL((k_fovea_fixed_part<decltype(gm), decltype(mode)::value>), grid, dim3(kThreads), ctx->plan.lds, st[k], gm, q);
                return 0;
            });
        });
    }
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_fov ^= 1;
    for (int k = 1; k < parts; ++k) {
        AGX_HIP(ctx, hipEventRecord(ctx->ev_join[k - 1], st[k]));
        AGX_HIP(ctx, hipStreamWaitEvent(st[0], ctx->ev_join[k - 1], 0));
    }
    return AGX_OK;
}

// The heterogeneous launch (ingest bands + fovea of the untouched slots in one grid, written slot after) is
// bit-identical and measured a tie at N=1024 (69.3 vs 67.9 us per step: it fills the ingest's drain but its
// second launch is one latency chain long), so the default is the two stand-alone launches.
int exp_step_fused(agx_ctx *ctx, const uint8_t *d_frames, const uint8_t *d_cmd, const void *d_action, int action_dtype, float *d_obs,
                   int32_t *d_fov_loc, void *mid_event, void *stream) {
    const agx_config &c = ctx->cfg;
    const bool headline = ctx->plan.headline;
    DeviceGuard g(c.device);
    const IngestParams pi = ingest_params(ctx, d_frames, d_cmd);
    FovParams pf = fov_params(ctx, d_action, action_dtype, nullptr, nullptr, d_obs, d_fov_loc, nullptr);
    pf.cmd = d_cmd;
    pf.phase = 1;
    pf.head = ctx->head[ctx->cur_head];                  // the head BEFORE this step's ingest
    const bool b12 = ctx->tune.fused >= 2 && ctx->k1.band12_ok && ctx->band_rows == 12;      // AGX_STEP_FUSED=2 / 3: band12 ingest body
    const size_t lds = std::max(b12 ? band12_lds(c.obs_w) : ingest_lds(ctx->band_rows, c.obs_w), fixed_lds(c));
    const dim3 grid1(pi.nbands + c.frame_stack, c.num_envs), grid2(1, c.num_envs), block(kThreads);
    using GS = GeomS<84, 84, 30, 30>;
    if (b12 && headline && ctx->tune.fused == 3)
        hipLaunchKernelGGL((k_step_fixed12_ff<GS>), grid1, block, lds, S(stream), GS{}, pi, pf);
    else if (b12 && headline)
        hipLaunchKernelGGL((k_step_fixed12<GS>), grid1, block, lds, S(stream), GS{}, pi, pf);
    else
        with_geom(headline, geom_r(c), [&](auto gm) {
            hipLaunchKernelGGL((k_step_fixed<decltype(gm)>), grid1, block, lds, S(stream), gm, pi, pf);
            return 0;
        });
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_head ^= 1;
    if (mid_event) AGX_HIP(ctx, hipEventRecord(static_cast<hipEvent_t>(mid_event), S(stream)));
    pf.phase = 2;
    pf.head = ctx->head[ctx->cur_head];                  // the head AFTER the ingest
    with_geom(headline, geom_r(c), [&](auto gm) {
        hipLaunchKernelGGL((k_step_fixed_tail<decltype(gm)>), grid2, block, fixed_lds(c), S(stream), gm, pf);
        return 0;
    });
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_fov ^= 1;
    return AGX_OK;
}

bool exp_step_fixed(agx_ctx *ctx, const uint8_t *d_frames, const uint8_t *d_cmd, const void *d_action, int action_dtype, float *d_obs,
                    int32_t *d_fov_loc, void *mid_event, void *stream, int *rc) {
    const agx_config &c = ctx->cfg;
    const agx_ctx::Tune &tn = ctx->tune;
    const bool fused = tn.fused != 0 && ctx->obs_type == AGX_OBS_F32;   // tuning / testing knob (f32 outputs only)
    // (the forms below write f32 observations only: a 16-bit context takes the product form)
    const bool default_forms = !fused && !tn.ingest_t && !tn.band_rows && !tn.pipe_parts && !tn.wave && !tn.pair && !tn.no_full &&
                               ctx->obs_type == AGX_OBS_F32;
    // Measured at N=1024 (same box, bench.py --steps 600): one launch pair 60.9 us per step; 2 parts 72.7 (69.3 with
    // low-priority internal streams, 75.1 with high), 3 parts 86.6, 4 parts 105: every cross-stream event edge costs more
    // than the overlap returns (round 1's +6-10 % came from two independent contexts that never join).  So it is opt-in.
    int parts = tn.split > 0 ? tn.split : 1;
    parts = std::min(std::min(parts, 4), c.num_envs);
    if (tn.step_env != 0 && default_forms && !mid_event && c.out_mode == AGX_OUT_RESIZE && ctx->plan.headline && ctx->k1.y_affine &&
        ctx->band_rows == 12 && c.frame_stack >= 1)
        *rc = exp_step_env(ctx, d_frames, d_cmd, d_action, action_dtype, d_obs, d_fov_loc, stream);
    else if (parts > 1 && default_forms && c.obs_h == c.obs_w && !mid_event)
        *rc = exp_step_split(ctx, parts, d_frames, d_cmd, d_action, action_dtype, d_obs, d_fov_loc, stream);
    else if (!(c.out_mode != AGX_OUT_RESIZE || ctx->ingest_t != 256 || !fused || c.obs_h != c.obs_w))
        *rc = exp_step_fused(ctx, d_frames, d_cmd, d_action, action_dtype, d_obs, d_fov_loc, mid_event, stream);
    else
        return false;
    return true;
}

}  // namespace
