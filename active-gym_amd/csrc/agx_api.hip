// agx_api.hip — the C ABI declared in include/agx.h: context, table builders, launches.
// Built for gfx950 only (see ../build.py): hipcc --offload-arch=gfx950 -shared -fPIC.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <new>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include "agx.h"
#include "agx_kernels.h"
#include "agx_host_tables.h"
#include "agx_plan.h"
#include "agx_device_guard.h"
#include "agx_resources.h"
#include "agx_range.h"

using namespace agx;

namespace {

struct HipDeviceApi {
    static int get(int *dev) { return hipGetDevice(dev) == hipSuccess ? 0 : 1; }
    static int set(int dev) { return hipSetDevice(dev) == hipSuccess ? 0 : 1; }
};
using DeviceGuard = agx::DeviceGuardT<HipDeviceApi>;      // agx_device_guard.h (unit-tested with a mocked runtime)

// The runtime behind agx_resources.h: the one place in csrc/ that names these calls.  Everything a handle holds comes from
// the Resources member of its struct and goes back when the struct is deleted.
struct HipResourceApi : HipDeviceApi {
    using Error = hipError_t;
    static Error device_alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void device_free(void *p) { (void)hipFree(p); }
    static Error pinned_alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void pinned_free(void *p) { (void)hipHostFree(p); }
    static Error event_create(void **e, unsigned flags) { return hipEventCreateWithFlags(reinterpret_cast<hipEvent_t *>(e), flags); }
    static void event_destroy(void *e) { (void)hipEventDestroy(static_cast<hipEvent_t>(e)); }
    static Error stream_create(void **s, unsigned flags) { return hipStreamCreateWithFlags(reinterpret_cast<hipStream_t *>(s), flags); }
    static Error stream_create_priority(void **s, unsigned flags, int priority) {
        return hipStreamCreateWithPriority(reinterpret_cast<hipStream_t *>(s), flags, priority);
    }
    static void stream_destroy(void *s) { (void)hipStreamDestroy(static_cast<hipStream_t>(s)); }
};
using Resources = agx::ResourcesT<HipResourceApi>;        // agx_resources.h (unit-tested with a mocked runtime)

}  // namespace

struct agx_ctx {
    explicit agx_ctx(int device) : own(device) {}
    Resources own;             // owns every device allocation below (and the experiments build's streams and events): the typed
                               // pointers the launches read are views into it
    agx_config cfg;            // cfg.out_mode holds the mode only (AGX_OUT_*); its element type bits are obs_type
    int obs_type = AGX_OBS_F32;   // AGX_OBS_F32 | AGX_OBS_BF16 | AGX_OBS_F16
    int planes = 1;               // planes per frame: 1 gray, 3 colour (AGX_FRAME_RGB); the ring holds planes * fs per env
    uint8_t *ring = nullptr;
    int32_t *head[2] = {nullptr, nullptr};
    int32_t *loc[2] = {nullptr, nullptr};
    int32_t *res[2] = {nullptr, nullptr};
    int cur_head = 0;
    int cur_fov = 0;
    int rng_lo = 0, rng_n = 0;    // agx_env_range: the envs the ranged entry points act on ([0, num_envs) after agx_create)
    int2 *in_xtab = nullptr;   // K1 tables
    int4 *in_ytab = nullptr;
    int2 *in_xtab12 = nullptr; // K1 band12 form: {2 * x0, (a0 | a1 << 16) << 4} / {b0 << 8, b1 << 8}
    int2 *in_ytab12 = nullptr;
    K1Plan k1;                 // what build_k1 derives from obs_size: affine row form, band12_ok / compact12_ok, band_rows
    // compact source screens (agx_ingest_compact): the source rows the vertical resize reads, ascending, and the y table with
    // PACKED row indices
    std::vector<int32_t> src_rows;
    int4 *in_ytab_c = nullptr;
    Tap *fx_xtab = nullptr;    // K2 tables
    Tap *fx_ytab = nullptr;
    int2 *per_ln[4] = {nullptr, nullptr, nullptr, nullptr};   // K3 tables
    float *per_w[4] = {nullptr, nullptr, nullptr, nullptr};
    int per_maxt[4] = {0, 0, 0, 0};
    // K4 table families (wd, wb, wf, hd, hb, hf): entries, weights, per-size meta
    int2 *flex_ln[6] = {};
    float *flex_w[6] = {};
    int4 *flex_meta[6] = {};
    // K4 resize_to_full form (k_fovea_flexible3): composed per-axis operators, see agx_k4_flex3.h
    Flex3Params f3{};
    // K4 raw-crop / mask-out / packed forms (k_fovea_flexible_raw3, agx_k4_raw3.h)
    FlexRawParams fr{};
    int64_t *pack_local = nullptr;   // agx_fovea_flexible_packed: [N] block-local exclusive offsets, [ceil(N/256)] block totals
    int64_t *pack_block = nullptr;   // (both made in agx_create for flexible raw-crop contexts: no allocation in a step call)
    // K3 tuned form 3 (k_fovea_peripheral3)
    Per3Params p3{};
    // What runs (agx_plan.h), computed once in agx_create: the fovea launch of the context's kind, and the K1 launch of each
    // screen layout (K1Layout) at the band height in force for it
    FovPlan plan;
    K1Launch k1l[4];
#ifdef AGX_EXPERIMENTS
    // split step (agx_step_fixed): env-range parts 1.. run on these internal streams, forked from / joined to the caller's
    // (made on first use, from own)
    hipStream_t aux[3] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
#endif
    int band_rows = 0;         // rows per band of the RGB whole-screen ingest: k1.band_rows unless an experiments knob is set
    int ingest_t = 256;
    int init_r = 0, init_c = 0;
    hipEvent_t prof[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // agx_profile_next: [ingest | fovea][start | stop]
    // Testing knobs, read from the environment ONCE PER CONTEXT in agx_create (so one process can hold contexts of
    // several forms and compare them).  The shipped library has only the five that select a FALLBACK kernel, i.e. the
    // kernel (or launch sequence) other geometries get anyway (tests/test_gpu_parity.py::test_generic_fallback_kernel_matches_tuned); the rest
    // exist in the experiments build (-DAGX_EXPERIMENTS, experiments/agx_experiments.h) only.
    struct Tune : Knobs {        // the five shipped knobs: agx_plan.h
        // ---- experiments build only (always 0 in libagx.so)
        int ingest_t = 0;        // AGX_INGEST_T          128 | 256 threads per ingest workgroup
        int band_rows = 0;       // AGX_INGEST_BAND_ROWS  output rows per ingest workgroup (<= the default)
        int pipe_parts = 0;      // AGX_INGEST_PIPE       k_ingest_pipe with this many workgroups per env
        int wave = 0;            // AGX_INGEST_WAVE       wave-private (barrier-free) ingest
        int pair = 0;            // AGX_FOVEA_PAIR        two ring slots per K2 workgroup
        int fused = 0;           // AGX_STEP_FUSED        agx_step_fixed as one heterogeneous launch + tail
        int pair12 = 0;          // AGX_INGEST_PAIR12     k_ingest_pair12: two envs' bands per workgroup
        int step_env = 0;        // AGX_STEP_ENV          agx_step_fixed as ONE launch, one workgroup per env (k_step_env)
        int split = 0;           // AGX_STEP_SPLIT        env-range parts of agx_step_fixed on internal streams
        int aux_prio = 0;        // AGX_STEP_AUX_PRIO     -1 | 0 | 1: priority of the internal streams relative to normal
        int packed_wave = 0;     // AGX_PACKED_WAVE       packed ragged crops with one wave (64-thread workgroup) per (slot, env) item
    } tune;
    std::string err;
};

// Launch of a benchmarked kernel.  When agx_profile_next armed a start / stop event pair for this kernel family the
// launch goes through hipExtLaunchKernelGGL, which stamps the two events with the dispatch's own begin / end times (the
// times rocprofv3's kernel trace reports) instead of bracketing it with two more packets on the stream.
#define AGX_LAUNCH(which, kernel, grid, block, lds, stream, ...)                                              \
    do {                                                                                                      \
        hipEvent_t e0_ = ctx->prof[which][0], e1_ = ctx->prof[which][1];                                      \
        if (e0_ && e1_) {                                                                                     \
            ctx->prof[which][0] = ctx->prof[which][1] = nullptr;                                              \
            hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)(lds), stream, e0_, e1_, 0, __VA_ARGS__);    \
        } else {                                                                                              \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                \
        }                                                                                                     \
    } while (0)

namespace {

int env_int(const char *name, int dflt_if_set_empty = 1) {
    const char *e = getenv(name);
    if (!e) return 0;
    return *e ? atoi(e) : dflt_if_set_empty;
}

thread_local std::string g_create_err;

int fail(agx_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->err = buf;
    else
        g_create_err = buf;
    return code;
}

#define AGX_HIP(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail((ctx), AGX_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

inline hipStream_t S(void *s) { return static_cast<hipStream_t>(s); }

// a host table as a device allocation of the context (P: T or const T, as the launch parameters spell the field)
template <class P, class T>
int upload(agx_ctx *ctx, P **dptr, const std::vector<T> &h) {
    static_assert(std::is_same<typename std::remove_const<P>::type, T>::value, "the field's element type is the table's");
    T *d = nullptr;
    AGX_HIP(ctx, ctx->own.device_mem(&d, h.size() * sizeof(T)));
    AGX_HIP(ctx, hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *dptr = d;
    return AGX_OK;
}

bool has_fovea(const agx_config &c) { return c.kind != AGX_KIND_BASE; }

// Calls f(OT{}) with the observation element type of AGX_OBS_* `t` (float, __bf16, _Float16): every launch of a kernel that
// writes observations goes through this, the f32 instantiations are the kernels as they were before the 16-bit outputs.
template <class F>
int with_obs_type(int t, F &&f) {
    switch (t) {
        case AGX_OBS_BF16: return f(__bf16{});
        case AGX_OBS_F16: return f(_Float16{});
        default: return f(float{});
    }
}
// Calls f(std::integral_constant<int, NC>{}) with the context's planes per frame NC (1 gray, 3 AGX_FRAME_RGB): every launch of a
// K0 / K2 / K3 / K4 kernel goes through this; the NC = 1 instantiations are the gray kernels as they were.
template <class F>
int with_planes(int planes, F &&f) {
    return planes == 3 ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 1>{});
}
// Calls f(g) with the geometry argument a plan selects: the compile-time GeomS<84, 84, 30, 30> (K2, K4, K5, K6) /
// PGeomS<84, 84, 30, 30, 20, 20> (K3) where `headline`, the run-time one otherwise.
template <class F>
int with_geom(bool headline, const GeomR &gr, F &&f) {
    return headline ? f(GeomS<84, 84, 30, 30>{}) : f(gr);
}
template <class F>
int with_pgeom(bool headline, const PGeomR &pg, F &&f) {
    return headline ? f(PGeomS<84, 84, 30, 30, 20, 20>{}) : f(pg);
}
// Calls f(std::integral_constant<int, MODE>{}) with the AGX_OUT_* mode of a fixed-fovea kernel (K2, K5)
template <class F>
int with_mode(int mode, F &&f) {
    switch (mode) {
        case AGX_OUT_RAW: return f(std::integral_constant<int, AGX_OUT_RAW>{});
        case AGX_OUT_MASK: return f(std::integral_constant<int, AGX_OUT_MASK>{});
        default: return f(std::integral_constant<int, AGX_OUT_RESIZE>{});
    }
}
GeomR geom_r(const agx_config &c) { return GeomR{c.obs_h, c.obs_w, c.fov_h, c.fov_w}; }
int obs_elem_bytes(int t) { return t == AGX_OBS_F32 ? 4 : 2; }
// bytes of one env's observation in the context's element type: frame_stack * planes images, fov-sized where `crop` (the row of
// agx_obs_shape: crop = a fixed fovea in raw-crop mode)
size_t obs_row_bytes(const agx_ctx *ctx, bool crop) {
    const agx_config &c = ctx->cfg;
    return (size_t)c.frame_stack * ctx->planes * (crop ? (size_t)c.fov_h * c.fov_w : (size_t)c.obs_h * c.obs_w) * obs_elem_bytes(ctx->obs_type);
}
// bytes of one env's sensory action (two values) at action dtype `dt`
size_t action_stride(int dt) { return dt == AGX_DT_F64 || dt == AGX_DT_I64 ? 16 : 8; }

// ---- env range (agx_env_range, include/agx_hostout.h; agx_range.h says how it reaches the kernels)
bool full_range(const agx_ctx *ctx) { return ctx->rng_lo == 0 && ctx->rng_n == ctx->cfg.num_envs; }
int refuse_range(agx_ctx *ctx, const char *who) {
    return fail(ctx, AGX_E_STATE, "%s: acts on the whole batch only; the context's env range is [%d, %d) (agx_env_range)", who,
                ctx->rng_lo, ctx->rng_lo + ctx->rng_n);
}
// the out-of-range envs' entries of a double-buffered state array pair, from the buffer a ranged launch read to the one it wrote
void range_carry(const agx_ctx *ctx, const int32_t *src0, int32_t *dst0, const int32_t *src1, int32_t *dst1, int words, hipStream_t st) {
    if (full_range(ctx)) return;
    RangeCarryParams q;
    q.src[0] = src0; q.dst[0] = dst0; q.src[1] = src1; q.dst[1] = dst1;
    q.words = words;
    q.lo = ctx->rng_lo; q.n = ctx->rng_n; q.total = ctx->cfg.num_envs;
    hipLaunchKernelGGL(k_range_carry, dim3((q.total * words + kThreads - 1) / kThreads), dim3(kThreads), 0, st, q);
}

// the context's env range on an ingest launch: base pointers advanced by rng_lo envs (the grid's env dimension is rng_n);
// env_bytes = the two screens of one env in this entry point's layout
template <class P>
void ingest_range(const agx_ctx *ctx, P &p, const uint8_t *P::*frames, size_t env_bytes) {
    const size_t lo = (size_t)ctx->rng_lo;
    p.*frames += lo * env_bytes;
    p.cmd += lo;
    p.ring += lo * (size_t)ctx->cfg.frame_stack * ctx->planes * ((size_t)ctx->cfg.obs_h * ctx->cfg.obs_w);
    p.head_in += lo;
    p.head_out += lo;
}

// ---- K1: what every ingest entry point shares
// the entry points that do not run on a colour (AGX_FRAME_RGB) context: the raw-screen Atari ingests, the fused Atari step and
// the packed ragged crops
int refuse_rgb(agx_ctx *ctx, const char *who) {
    return fail(ctx, AGX_E_STATE, "%s: not valid on an AGX_FRAME_RGB context (colour frames come in through agx_ingest_rgb with "
                "AGX_GRAY_NONE)", who);
}

// the launch arguments of the K1 band kernels for one screen layout, at the band height its plan holds
IngestParams ingest_params(agx_ctx *ctx, const uint8_t *d_frames, const uint8_t *d_cmd, int layout = kK1Rgb) {
    const agx_config &c = ctx->cfg;
    const bool compact = layout >= kK1RgbCompact;
    IngestParams p;
    p.frames = d_frames;
    p.cmd = d_cmd;
    p.ring = ctx->ring;
    p.head_in = ctx->head[ctx->cur_head];
    p.head_out = ctx->head[ctx->cur_head ^ 1];
    p.xtab = ctx->in_xtab;
    p.ytab = compact ? ctx->in_ytab_c : ctx->in_ytab;     // compact screens: packed row indices
    p.oh = c.obs_h;
    p.ow = c.obs_w;
    p.fs = c.frame_stack;
    p.band_rows = ctx->k1l[layout].band_rows;
    p.y_affine = compact ? 0 : ctx->k1.y_affine;
    p.y_mul = ctx->k1.y_mul;
    p.y_add = ctx->k1.y_add;
    p.y_shift = ctx->k1.y_shift;
    p.nbands = ctx->k1l[layout].nbands;
    p.xtab12 = ctx->in_xtab12;
    p.ytab12 = ctx->in_ytab12;
    p.ow4_inv16 = (65536 + c.obs_w / 4 - 1) / (c.obs_w / 4);
    p.src_rows = compact ? (int32_t)ctx->src_rows.size() : 0;
    p.stamps = nullptr;
#ifdef AGX_STAMPS
    if (const char *e = getenv("AGX_DBG_PTR")) p.stamps = reinterpret_cast<unsigned long long *>(strtoull(e, nullptr, 0));
#endif
    return p;
}
// after a ranged ingest launch, in front of the head flip
void ingest_carry(const agx_ctx *ctx, void *stream) {
    range_carry(ctx, ctx->head[ctx->cur_head], ctx->head[ctx->cur_head ^ 1], nullptr, nullptr, 1, S(stream));
}

// ---- K2 / K3 / K4: what every fovea entry point shares
int check_dt(agx_ctx *ctx, const void *d_action, int dt) {
    if (d_action && (dt < AGX_DT_F32 || dt > AGX_DT_I64)) return fail(ctx, AGX_E_INVALID, "unknown action dtype %d", dt);
    return AGX_OK;
}

FovParams fov_params(agx_ctx *ctx, const void *d_action, int dt, const int32_t *d_type, const uint8_t *d_mask,
                            float *d_obs, int32_t *d_loc, int32_t *d_res) {
    const agx_config &c = ctx->cfg;
    FovParams p;
    p.ring = ctx->ring;
    p.head = ctx->head[ctx->cur_head];
    p.loc_in = ctx->loc[ctx->cur_fov];
    p.loc_out = ctx->loc[ctx->cur_fov ^ 1];
    p.res_in = ctx->res[ctx->cur_fov];
    p.res_out = ctx->res[ctx->cur_fov ^ 1];
    p.action = d_action;
    p.action_type = d_type;
    p.mask = d_mask;
    p.obs = d_obs;
    p.user_loc = d_loc;
    p.user_res = d_res;
    p.xtab = ctx->fx_xtab;
    p.ytab = ctx->fx_ytab;
    p.sas_lo = c.sas_lo;
    p.sas_hi = c.sas_hi;
    p.action_dt = dt;
    p.relative = c.action_mode == AGX_MODE_RELATIVE;
    p.fs = c.frame_stack;
    p.out_mode = c.out_mode;
    p.antialias = c.antialias != 0;
    p.per_h = c.per_h;
    p.per_w = c.per_w;
    p.buf1_floats = (int32_t)generic_buf1(c);
    p.cmd = nullptr;
    p.phase = 0;
    p.packed = nullptr;
    p.packed_off = nullptr;
    p.packed_cap = 0;
    p.stamps = nullptr;
#ifdef AGX_STAMPS
    if (const char *e = getenv("AGX_DBG_PTR2")) p.stamps = reinterpret_cast<unsigned long long *>(strtoull(e, nullptr, 0));
#endif
    return p;
}
// the context's env range on a fovea launch: every per-env base pointer advanced by rng_lo envs (the grid's env dimension is
// rng_n); the observation row is that of agx_obs_shape in the context's element type
void fov_range(const agx_ctx *ctx, FovParams &p) {
    const size_t lo = (size_t)ctx->rng_lo;
    if (lo == 0) return;
    const agx_config &c = ctx->cfg;
    const size_t planes = (size_t)c.frame_stack * ctx->planes, px = (size_t)c.obs_h * c.obs_w;
    p.ring += lo * planes * px;
    p.head += lo;
    p.loc_in += 2 * lo;
    p.loc_out += 2 * lo;
    p.res_in += 2 * lo;
    p.res_out += 2 * lo;
    if (p.action) p.action = static_cast<const char *>(p.action) + lo * action_stride(p.action_dt);
    if (p.action_type) p.action_type += lo;
    if (p.mask) p.mask += lo;
    p.obs = reinterpret_cast<float *>(reinterpret_cast<char *>(p.obs) + lo * obs_row_bytes(ctx, c.kind == AGX_KIND_FIXED && c.out_mode == AGX_OUT_RAW));
    if (p.user_loc) p.user_loc += 2 * lo;
    if (p.user_res) p.user_res += 2 * lo;
}
// after a ranged fovea launch, in front of the fov flip: fov_loc of the out-of-range envs, and fov_res where the kind writes it
void fov_carry(const agx_ctx *ctx, void *stream) {
    const bool flex = ctx->cfg.kind == AGX_KIND_FLEXIBLE;
    range_carry(ctx, ctx->loc[ctx->cur_fov], ctx->loc[ctx->cur_fov ^ 1], flex ? ctx->res[ctx->cur_fov] : nullptr,
                flex ? ctx->res[ctx->cur_fov ^ 1] : nullptr, 2, S(stream));
}

// the state / scan launch of the packed form (fov_env.py:300-324 + level 1 of the exclusive scan of the crop sizes; the scratch
// belongs to the context since agx_create)
FlexParams flex_params(const agx_ctx *ctx) {       // k_fovea_flexible2's table families
    const agx_config &c = ctx->cfg;
    FlexParams g;
    TabFamily *fam[6] = {&g.wd, &g.wb, &g.wf, &g.hd, &g.hb, &g.hf};
    for (int k = 0; k < 6; ++k) {
        fam[k]->ln = ctx->flex_ln[k];
        fam[k]->w = ctx->flex_w[k];
        fam[k]->meta = ctx->flex_meta[k];
    }
    g.oh = c.obs_h; g.ow = c.obs_w; g.fh = c.fov_h; g.fw = c.fov_w;
    return g;
}

FlexScanParams packed_scan_params(agx_ctx *ctx, const void *d_action, int action_dtype, const int32_t *d_action_type,
                                         int32_t *d_fov_loc, int32_t *d_fov_res) {
    FlexScanParams q;
    q.f = fov_params(ctx, d_action, action_dtype, d_action_type, nullptr, nullptr, d_fov_loc, d_fov_res);
    q.local_off = ctx->pack_local;
    q.block_tot = ctx->pack_block;
    q.n = ctx->cfg.num_envs;
    q.oh = ctx->cfg.obs_h;
    q.ow = ctx->cfg.obs_w;
    return q;
}

}  // namespace

#ifdef AGX_EXPERIMENTS
#include "experiments/agx_experiments_host.h"   // the opt-in launch forms the entry points below hook (exp_*)
#endif

extern "C" {

int agx_abi_version(void) { return AGX_ABI_VERSION; }

#ifndef AGX_SRC_HASH
#define AGX_SRC_HASH "unknown"
#endif
#define AGX_STR2(x) #x
#define AGX_STR(x) AGX_STR2(x)
const char *agx_build_info(void) { return "libagx abi " AGX_STR(AGX_ABI_VERSION) " src " AGX_SRC_HASH; }

const char *agx_last_error(const agx_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int agx_device_pci_bus_id(int device, char *buf, int len) {
    if (!buf || len < 13) return fail(nullptr, AGX_E_INVALID, "agx_device_pci_bus_id: buffer of at least 13 bytes needed");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) {
        (void)hipGetLastError();                 // the runtime's last-error slot is sticky: do not leave it to the caller's next HIP call
        return fail(nullptr, AGX_E_HIP, "no HIP device");
    }
    if (device < 0 || device >= ndev) return fail(nullptr, AGX_E_INVALID, "device %d out of range (%d visible)", device, ndev);
    const hipError_t e = hipDeviceGetPCIBusId(buf, len, device);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(nullptr, AGX_E_HIP, "hipDeviceGetPCIBusId(%d): %s", device, hipGetErrorString(e));
    }
    return AGX_OK;
}

int agx_destroy(agx_ctx *ctx) {
    if (!ctx) return AGX_OK;
    DeviceGuard g(ctx->cfg.device);
    delete ctx;
    return AGX_OK;
}

static int ctx_build(agx_ctx *ctx);

int agx_create(const agx_config *cfg, agx_ctx **out) {
    if (!cfg || !out) return fail(nullptr, AGX_E_INVALID, "agx_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(agx_config))
        return fail(nullptr, AGX_E_INVALID, "agx_create: struct_size %d != %zu (ABI mismatch)", cfg->struct_size,
                    sizeof(agx_config));
    // out_mode = AGX_OUT_* | AGX_OBS_*: the context keeps the mode in cfg.out_mode and the element type in obs_type
    const int obs_type = cfg->out_mode & AGX_OBS_TYPE_MASK;
    if (obs_type == AGX_OBS_TYPE_MASK)
        return fail(nullptr, AGX_E_INVALID, "out_mode 0x%x: AGX_OBS_BF16 and AGX_OBS_F16 are exclusive", cfg->out_mode);
    // AGX_FRAME_RGB: three planes per frame, stored in ctx->planes
    const int planes = (cfg->out_mode & AGX_FRAME_RGB) ? 3 : 1;
    agx_config c_split = *cfg;
    c_split.out_mode = cfg->out_mode & ~(AGX_OBS_TYPE_MASK | AGX_FRAME_RGB);
    const agx_config &c = c_split;
    agx_ctx::Tune tune;          // the knobs: read here, once per context
    tune.generic = env_int("AGX_FOVEA_GENERIC");
    tune.no_full = env_int("AGX_INGEST_NO_FULL");
    tune.flex_v2 = env_int("AGX_FLEX_V2");
    tune.per_v2 = env_int("AGX_PER_V2");
    tune.packed_unfused = env_int("AGX_STEP_PACKED_UNFUSED");
    if (c.num_envs < 1 || c.num_envs > 65535)   // env index rides on gridDim.y / gridDim.z
        return fail(nullptr, AGX_E_INVALID, "num_envs must be in [1, 65535] per context (shard larger batches)");
    if (c.raw_h != kRawH || c.raw_w != kRawW)
        return fail(nullptr, AGX_E_INVALID, "raw screen must be %dx%d (ALE), got %dx%d", kRawH, kRawW, c.raw_h, c.raw_w);
    if (c.obs_h < 4 || c.obs_w < 4 || (c.obs_w & 3) || c.obs_w > 1024 || c.obs_h > 1024)
        return fail(nullptr, AGX_E_INVALID, "obs_size (%d,%d): need 4 <= h,w <= 1024 and w %% 4 == 0", c.obs_h, c.obs_w);
    if (c.frame_stack < 1 || c.frame_stack > 16) return fail(nullptr, AGX_E_INVALID, "frame_stack must be in [1,16]");
    if (c.kind < AGX_KIND_BASE || c.kind > AGX_KIND_PERIPHERAL) return fail(nullptr, AGX_E_INVALID, "unknown kind %d", c.kind);
    if (has_fovea(c)) {
        // assert (np.array(self.fov_size) < np.array(self.obs_size)).all()   fov_env.py:112
        if (c.fov_h < 1 || c.fov_w < 1 || c.fov_h >= c.obs_h || c.fov_w >= c.obs_w)
            return fail(nullptr, AGX_E_INVALID, "fov_size (%d,%d) must be >= 1 and < obs_size (%d,%d)", c.fov_h, c.fov_w,
                        c.obs_h, c.obs_w);
        if (c.out_mode < AGX_OUT_RAW || c.out_mode > AGX_OUT_MASK)
            return fail(nullptr, AGX_E_INVALID, "bad out_mode 0x%x (AGX_OUT_* | AGX_OBS_* | AGX_FRAME_RGB)", cfg->out_mode);
        if (c.action_mode != AGX_MODE_ABSOLUTE && c.action_mode != AGX_MODE_RELATIVE)
            return fail(nullptr, AGX_E_INVALID, "bad action_mode");
        if (c.action_mode == AGX_MODE_RELATIVE && !(c.sas_lo <= c.sas_hi))
            return fail(nullptr, AGX_E_INVALID, "relative mode needs sensory_action_space lo <= hi");
        if (!std::isfinite(c.init_loc[0]) || !std::isfinite(c.init_loc[1]))
            return fail(nullptr, AGX_E_INVALID, "fov_init_loc must be finite");
        if (c.kind == AGX_KIND_PERIPHERAL && (c.per_h < 1 || c.per_w < 1 || c.per_h > 1024 || c.per_w > 1024))
            return fail(nullptr, AGX_E_INVALID, "peripheral_res (%d,%d) out of range", c.per_h, c.per_w);
        const size_t lds = create_lds(c, tune);
        if (lds > kMaxLds)
            return fail(nullptr, AGX_E_INVALID, "geometry needs %zu B of LDS per workgroup (limit %zu)", lds, kMaxLds);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, AGX_E_HIP, "no HIP device: libagx has no CPU path");
    if (c.device < 0 || c.device >= ndev) return fail(nullptr, AGX_E_INVALID, "device %d out of range (%d visible)", c.device, ndev);

    agx_ctx *ctx = new (std::nothrow) agx_ctx(c.device);
    if (!ctx) return fail(nullptr, AGX_E_NOMEM, "out of host memory");
    ctx->cfg = c;
    ctx->obs_type = obs_type;
    ctx->planes = planes;
    ctx->rng_n = c.num_envs;
    ctx->tune = tune;
    ctx->plan = plan_base(c);
#ifdef AGX_EXPERIMENTS
    ctx->tune.ingest_t = env_int("AGX_INGEST_T");
    ctx->tune.band_rows = env_int("AGX_INGEST_BAND_ROWS");
    ctx->tune.pipe_parts = env_int("AGX_INGEST_PIPE");
    ctx->tune.wave = env_int("AGX_INGEST_WAVE");
    ctx->tune.pair = env_int("AGX_FOVEA_PAIR");
    ctx->tune.fused = env_int("AGX_STEP_FUSED");
    ctx->tune.pair12 = env_int("AGX_INGEST_PAIR12");
    ctx->tune.step_env = env_int("AGX_STEP_ENV");
    ctx->tune.split = env_int("AGX_STEP_SPLIT");
    ctx->tune.aux_prio = env_int("AGX_STEP_AUX_PRIO", 0);
    ctx->tune.packed_wave = env_int("AGX_PACKED_WAVE");
#endif
    DeviceGuard g(c.device);
    const int rc = ctx_build(ctx);
    if (rc != AGX_OK) {                 // whatever the context holds by now goes back with it
        g_create_err = ctx->err;
        delete ctx;
        return rc;
    }
    *out = ctx;
    return AGX_OK;
}

// What agx_create allocates and uploads for a checked configuration (the plans ride along: they read the host tables).  Any
// failure leaves its message in ctx->err and returns; agx_create deletes the context, which gives back whatever was made.
static int ctx_build(agx_ctx *ctx) {
    const agx_config &c = ctx->cfg;
    const Knobs &tune = ctx->tune;      // the five shipped knobs: what the plans read
    const int planes = ctx->planes;
    int rc = AGX_OK;
    const size_t N = c.num_envs, fsz = (size_t)c.obs_h * c.obs_w;
    AGX_HIP(ctx, ctx->own.device_mem(&ctx->ring, N * c.frame_stack * planes * fsz));
    AGX_HIP(ctx, hipMemset(ctx->ring, 0, N * c.frame_stack * planes * fsz));
    for (int b = 0; b < 2; ++b) {
        AGX_HIP(ctx, ctx->own.device_mem(&ctx->head[b], N * sizeof(int32_t)));
        AGX_HIP(ctx, hipMemset(ctx->head[b], 0, N * sizeof(int32_t)));
    }
    // K1 tables and plan (only meaningful for square obs; built anyway, agx_ingest checks): build_k1, agx_host_tables.h
    {
        const K1Host k1 = build_k1(c.obs_h, c.obs_w);
        ctx->k1 = k1.plan;
        ctx->src_rows = k1.src_rows;
        std::vector<int2> xt(c.obs_w), xt12(c.obs_w), yt12(c.obs_h);
        std::vector<int4> yt(c.obs_h), ytc(c.obs_h);
        for (int i = 0; i < c.obs_w; ++i) {
            xt[i] = make_int2(k1.x0[i] | (k1.x1[i] << 16), (k1.a0[i] & 0xFFFF) | (k1.a1[i] << 16));
            // band12 form: the same coefficients in the shape its phase 2 consumes
            xt12[i] = make_int2(2 * k1.x0[i], (int)((((uint32_t)k1.a0[i] & 0xFFFFu) | ((uint32_t)k1.a1[i] << 16)) << 4));
        }
        for (int i = 0; i < c.obs_h; ++i) {
            yt[i] = make_int4(k1.y0[i], k1.y1[i], k1.b0[i], k1.b1[i]);
            ytc[i] = make_int4(k1.py0[i], k1.py1[i], k1.b0[i], k1.b1[i]);
            yt12[i] = make_int2(k1.b0[i] << 8, k1.b1[i] << 8);
        }
        if ((rc = upload(ctx, &ctx->in_ytab_c, ytc)) != AGX_OK) return rc;
        if ((rc = upload(ctx, &ctx->in_xtab, xt)) != AGX_OK) return rc;
        if ((rc = upload(ctx, &ctx->in_ytab, yt)) != AGX_OK) return rc;
        if ((rc = upload(ctx, &ctx->in_xtab12, xt12)) != AGX_OK) return rc;
        if ((rc = upload(ctx, &ctx->in_ytab12, yt12)) != AGX_OK) return rc;
        // the RGB whole-screen ingest: 128-thread workgroups give 16 independent workgroups per CU whose load / compute
        // phases interleave (AGX_INGEST_T tunes; 8 WGs/CU whatever T: 256 fills the wave slots), fewer rows per band
        // (AGX_INGEST_BAND_ROWS).  Both knobs are 0 in the shipped library: band_rows is then the plan's.
        const int forced_t = ctx->tune.ingest_t;
        ctx->ingest_t = (forced_t == 128 || forced_t == 256) ? forced_t : 256;
        if (c.obs_w / 4 > 128) ctx->ingest_t = 256;
        ctx->band_rows = k1_band_rows(c.obs_w, ctx->ingest_t);
        const int forced_br = ctx->tune.band_rows;
        if (forced_br >= 1 && forced_br <= ctx->band_rows) ctx->band_rows = forced_br;
        // agx_ingest_gray_raw: the plan's 256-thread bands (AGX_INGEST_BAND_ROWS of the experiments build narrows them as it
        // does the RGB ingest's; the other opt-in variants are RGB-only); compact screens: always the default 256-thread band form
        const int gray_rows = ctx->ingest_t == 256 ? std::min(k1.plan.band_rows, ctx->band_rows) : k1.plan.band_rows;
        const int rows[4] = {ctx->band_rows, gray_rows, k1.plan.band_rows, k1.plan.band_rows};
        for (int k = 0; k < 4; ++k) ctx->k1l[k] = plan_k1(k1.plan, k, rows[k], c.obs_h, c.obs_w, tune);
    }
    if (has_fovea(c)) {
        // _init_fov_loc: np.rint(fov_init_loc).astype(np.int32)  (not clipped)   fov_env.py:149-150
        ctx->init_r = (int)std::nearbyint(c.init_loc[0]);
        ctx->init_c = (int)std::nearbyint(c.init_loc[1]);
        if (ctx->init_r < 0 || ctx->init_c < 0 || ctx->init_r > c.obs_h - c.fov_h || ctx->init_c > c.obs_w - c.fov_w)
            return fail(ctx, AGX_E_INVALID, "fov_init_loc (%g,%g) puts the %dx%d window outside the %dx%d frame", c.init_loc[0],
                        c.init_loc[1], c.fov_h, c.fov_w, c.obs_h, c.obs_w);
        std::vector<int32_t> loc(2 * N), res(2 * N);
        for (size_t i = 0; i < N; ++i) {
            loc[2 * i] = ctx->init_r;
            loc[2 * i + 1] = ctx->init_c;
            res[2 * i] = c.fov_h;
            res[2 * i + 1] = c.fov_w;
        }
        for (int b = 0; b < 2; ++b) {
            if ((rc = upload(ctx, &ctx->loc[b], loc)) != AGX_OK) return rc;
            if ((rc = upload(ctx, &ctx->res[b], res)) != AGX_OK) return rc;
        }
        if (c.kind == AGX_KIND_FLEXIBLE) {
            HostFamily fam[6];
            const size_t tab_floats = build_families(c, fam);   // worst-case LDS floats of the staged tables
            for (int k = 0; k < 6; ++k) {
                if ((rc = upload(ctx, &ctx->flex_ln[k], fam[k].ln)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &ctx->flex_w[k], fam[k].w)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &ctx->flex_meta[k], fam[k].meta)) != AGX_OK) return rc;
            }
            // resize_to_full: the composed-operator kernel where its plan applies (thread-per-column, <= 16 taps)
            const Flex3Host f3 = build_flex3(c);
            if (flex3_fits(f3, c)) {
                Flex3Params &q = ctx->f3;
                if ((rc = upload(ctx, &q.wf, f3.wf)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.wc_meta, f3.wc_meta)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.wc_lo, f3.wc_lo)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.wc_w, f3.wc_w)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.hd_meta, f3.hd_meta)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.hd_lo, f3.hd_lo)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.hd_w, f3.hd_w)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.hy, f3.hy)) != AGX_OK) return rc;
                q.r0_bytes = f3.r0_bytes;
                q.r1_bytes = f3.r1_bytes;
                q.dp = f3.dp;
            }
            // raw-crop / mask-out: the composed squeeze-and-back form where its plan applies
            const FlexRawHost fr = build_flexraw(c);
            if (flexraw_fits(fr, c)) {
                FlexRawParams &q = ctx->fr;
                if ((rc = upload(ctx, &q.wb_meta, fr.wb_meta)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.wb_lo, fr.wb_lo)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.wb_w, fr.wb_w)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.hd_meta, fr.hd_meta)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.hd_lo, fr.hd_lo)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.hd_w, fr.hd_w)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.hb, fr.hb)) != AGX_OK) return rc;
                q.r0_bytes = fr.r0_bytes;
                q.r1_bytes = fr.r1_bytes;
                q.dp = fr.dp;
                q.n_envs = c.num_envs;
            }
            ctx->plan = plan_flexible(c, tune, f3, fr, tab_floats);
            if (c.out_mode == AGX_OUT_RAW) {       // the packed form's scan buffers
                const size_t nb = (N + kScanEnvsPerBlock - 1) / kScanEnvsPerBlock;
                AGX_HIP(ctx, ctx->own.device_mem(&ctx->pack_local, N * sizeof(int64_t)));
                AGX_HIP(ctx, ctx->own.device_mem(&ctx->pack_block, nb * sizeof(int64_t)));
            }
        }
        if (c.kind == AGX_KIND_PERIPHERAL) {
            int nin[4], nout[4];
            per_axes(c, nin, nout);
            for (int k = 0; k < 4; ++k) {
                std::vector<int2> ln;
                std::vector<float> w;
                axis_taps(nin[k], nout[k], c.antialias != 0, ln, w, ctx->per_maxt[k]);
                if (k == 0)                          // the first pass reads u8 numerators: fold the /255 into its weights
                    for (float &v : w) v = (float)((double)v / 255.0);
                if ((rc = upload(ctx, &ctx->per_ln[k], ln)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &ctx->per_w[k], w)) != AGX_OK) return rc;
            }
            const Per3Host h3 = build_per3(c);
            if (per3_fits(h3)) {
                Per3Params &q = ctx->p3;
                if ((rc = upload(ctx, &q.lo0, h3.lo0)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.w0, h3.w0)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.lo1, h3.lo1)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.w1, h3.w1)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.x2, h3.x2)) != AGX_OK) return rc;
                if ((rc = upload(ctx, &q.y3, h3.y3)) != AGX_OK) return rc;
            }
            ctx->plan = plan_peripheral(c, tune, h3, ctx->per_maxt);
            ctx->p3.same = ctx->plan.same;
        }
        if (c.kind == AGX_KIND_FIXED) ctx->plan = plan_fixed(c);
        if (c.kind == AGX_KIND_FIXED && c.out_mode == AGX_OUT_RESIZE) {
            std::vector<Tap> xt(c.obs_w), yt(c.obs_h);
            for (int i = 0; i < c.obs_w; ++i) xt[i] = make_tap_lin2(i, c.fov_w, c.obs_w);
            for (int i = 0; i < c.obs_h; ++i) yt[i] = make_tap_lin2(i, c.fov_h, c.obs_h);
            if ((rc = upload(ctx, &ctx->fx_xtab, xt)) != AGX_OK) return rc;
            if ((rc = upload(ctx, &ctx->fx_ytab, yt)) != AGX_OK) return rc;
        }
    }
    return AGX_OK;
}

int agx_obs_shape(const agx_ctx *ctx, int32_t dims[4]) {
    if (!ctx || !dims) return AGX_E_INVALID;
    const agx_config &c = ctx->cfg;
    dims[0] = c.num_envs;
    dims[1] = c.frame_stack * ctx->planes;
    const bool crop = c.kind == AGX_KIND_FIXED && c.out_mode == AGX_OUT_RAW;
    dims[2] = crop ? c.fov_h : c.obs_h;
    dims[3] = crop ? c.fov_w : c.obs_w;
    return AGX_OK;
}

int agx_profile_next(agx_ctx *ctx, int kernel_id, void *start_event, void *stop_event) {
    if (!ctx) return AGX_E_INVALID;
    const int which = kernel_id == AGX_K_INGEST ? 0 : (kernel_id == AGX_K_FOVEA ? 1 : -1);
    if (which < 0) return fail(ctx, AGX_E_INVALID, "agx_profile_next: kernel_id must be AGX_K_INGEST or AGX_K_FOVEA");
    if ((start_event == nullptr) != (stop_event == nullptr))
        return fail(ctx, AGX_E_INVALID, "agx_profile_next: pass both events, or neither to disarm");
    ctx->prof[which][0] = static_cast<hipEvent_t>(start_event);
    ctx->prof[which][1] = static_cast<hipEvent_t>(stop_event);
    return AGX_OK;
}

int64_t agx_algorithmic_bytes(const agx_ctx *ctx, int kernel_id) {
    if (!ctx) return AGX_E_INVALID;
    const agx_config &c = ctx->cfg;
    const int64_t N = c.num_envs, px = (int64_t)c.obs_h * c.obs_w, e = obs_elem_bytes(ctx->obs_type);
    const int64_t fs = (int64_t)c.frame_stack * ctx->planes;   // planes of the stack (AGX_FRAME_RGB: 3 per frame)
    if (ctx->planes != 1 && kernel_id != AGX_K_INGEST_RGB && kernel_id != AGX_K_FULL && kernel_id != AGX_K_FOVEA)
        return AGX_E_STATE;   // the raw-screen ingests do not run on a colour context
    switch (kernel_id) {
        case AGX_K_INGEST:   // two frames, only the source rows the vertical resize touches + one u8 slot
            return N * (2 * (int64_t)ctx->k1.rows_touched * kRawRowBytes + px);
        case AGX_K_INGEST_GRAY_RAW:   // two gray frames, only the touched source rows, + one u8 slot
            return N * (2 * (int64_t)ctx->k1.rows_touched * kRawW + px);
        case AGX_K_INGEST_RGB:   // one obs-sized RGB render in, one u8 slot out (colour: three u8 planes out)
            return N * px * (3 + ctx->planes);
        case AGX_K_FULL:
            return N * fs * px * (1 + e);
        case AGX_K_FOVEA: {
            if (!has_fovea(c)) return AGX_E_STATE;
            const int64_t win = (int64_t)c.fov_h * c.fov_w;
            if (c.kind == AGX_KIND_PERIPHERAL) return N * fs * px * (1 + e);
            if (c.kind == AGX_KIND_FIXED && c.out_mode == AGX_OUT_RAW) return N * fs * win * (1 + e);
            return N * fs * (win + px * e);
        }
        default:
            return AGX_E_INVALID;
    }
}

// ---------------------------------------------------------------- K1

int agx_ingest(agx_ctx *ctx, const uint8_t *d_frames, const uint8_t *d_cmd, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    if (ctx->planes != 1) return refuse_rgb(ctx, "agx_ingest");
    if (!d_frames || !d_cmd) return fail(ctx, AGX_E_INVALID, "agx_ingest: null buffer");
    const agx_config &c = ctx->cfg;
    if (c.obs_h != c.obs_w)
        return fail(ctx, AGX_E_INVALID,
                    "agx_ingest: obs_size (%d,%d) is not square; the reference hands obs_size to cv2.resize as "
                    "(width,height) and fails on non-square sizes (atari_env.py:74,126)", c.obs_h, c.obs_w);
    DeviceGuard g(c.device);
    IngestParams p = ingest_params(ctx, d_frames, d_cmd);
    ingest_range(ctx, p, &IngestParams::frames, (size_t)2 * kRawFrameBytes);
    const K1Launch &l = ctx->k1l[kK1Rgb];
    const dim3 grid(l.nbands, ctx->rng_n);     // rng_n: the envs of the launch (num_envs unless agx_env_range narrowed it)
#ifdef AGX_EXPERIMENTS
    if (!exp_ingest(ctx, p, stream))
#endif
    {
        // the headline form where its plan applies (12-row bands all full, affine source rows, adjacent x taps), the general
        // band kernel otherwise
        if (l.band12) AGX_LAUNCH(0, k_ingest_full12, grid, dim3(256), l.lds, S(stream), p);
        else AGX_LAUNCH(0, k_ingest<256>, grid, dim3(256), l.lds, S(stream), p);
    }
    ingest_carry(ctx, stream);
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_head ^= 1;
    return AGX_OK;
}

int agx_ingest_gray_raw(agx_ctx *ctx, const uint8_t *d_gray, const uint8_t *d_cmd, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    if (ctx->planes != 1) return refuse_rgb(ctx, "agx_ingest_gray_raw");
    if (!d_gray || !d_cmd) return fail(ctx, AGX_E_INVALID, "agx_ingest_gray_raw: null buffer");
    const agx_config &c = ctx->cfg;
    if (c.obs_h != c.obs_w)
        return fail(ctx, AGX_E_STATE, "agx_ingest_gray_raw needs a square obs_size (cv2.resize takes (width, height): atari_env.py:74)");
    DeviceGuard g(c.device);
    IngestParams p = ingest_params(ctx, d_gray, d_cmd, kK1Gray);
    ingest_range(ctx, p, &IngestParams::frames, (size_t)2 * kRawH * kRawW);
    const K1Launch &l = ctx->k1l[kK1Gray];
    const dim3 grid(l.nbands, ctx->rng_n), block(kThreads);
    if (l.band12) AGX_LAUNCH(0, k_ingest_grayraw_full12, grid, block, l.lds, S(stream), p);
    else AGX_LAUNCH(0, k_ingest_grayraw, grid, block, l.lds, S(stream), p);
    ingest_carry(ctx, stream);
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_head ^= 1;
    return AGX_OK;
}

int agx_source_rows(const agx_ctx *ctx, int32_t *rows, int32_t *n) {
    if (!ctx || !n) return AGX_E_INVALID;
    *n = (int32_t)ctx->src_rows.size();
    if (rows) std::copy(ctx->src_rows.begin(), ctx->src_rows.end(), rows);
    return AGX_OK;
}

// agx_ingest / agx_ingest_gray_raw from compact screens: the same band kernels with packed source rows
static int ingest_compact(agx_ctx *ctx, const uint8_t *d_rows, const uint8_t *d_cmd, void *stream, bool gray, const char *who) {
    if (!ctx) return AGX_E_INVALID;
    if (ctx->planes != 1) return refuse_rgb(ctx, who);
    if (!d_rows || !d_cmd) return fail(ctx, AGX_E_INVALID, "%s: null buffer", who);
    const agx_config &c = ctx->cfg;
    if (c.obs_h != c.obs_w)
        return fail(ctx, AGX_E_INVALID, "%s: obs_size (%d,%d) is not square (cv2.resize takes (width, height): atari_env.py:74)", who,
                    c.obs_h, c.obs_w);
    DeviceGuard g(c.device);
    const int layout = gray ? kK1GrayCompact : kK1RgbCompact;
    IngestParams p = ingest_params(ctx, d_rows, d_cmd, layout);
    ingest_range(ctx, p, &IngestParams::frames, (size_t)2 * ctx->src_rows.size() * kRawW * (gray ? 1 : 3));
    const K1Launch &l = ctx->k1l[layout];
    const dim3 grid(l.nbands, ctx->rng_n), block(kThreads);
    if (l.band12) {
        if (gray) AGX_LAUNCH(0, k_ingest_grayraw_full12_compact, grid, block, l.lds, S(stream), p);
        else AGX_LAUNCH(0, k_ingest_full12_compact, grid, block, l.lds, S(stream), p);
    } else {
        if (gray) AGX_LAUNCH(0, k_ingest_grayraw_compact, grid, block, l.lds, S(stream), p);
        else AGX_LAUNCH(0, k_ingest_compact, grid, block, l.lds, S(stream), p);
    }
    ingest_carry(ctx, stream);
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_head ^= 1;
    return AGX_OK;
}

int agx_ingest_compact(agx_ctx *ctx, const uint8_t *d_rows, const uint8_t *d_cmd, void *stream) {
    return ingest_compact(ctx, d_rows, d_cmd, stream, false, "agx_ingest_compact");
}
int agx_ingest_gray_raw_compact(agx_ctx *ctx, const uint8_t *d_rows, const uint8_t *d_cmd, void *stream) {
    return ingest_compact(ctx, d_rows, d_cmd, stream, true, "agx_ingest_gray_raw_compact");
}

int agx_ingest_gray(agx_ctx *ctx, const uint8_t *d_small, const uint8_t *d_cmd, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    if (ctx->planes != 1) return refuse_rgb(ctx, "agx_ingest_gray");
    if (!d_small || !d_cmd) return fail(ctx, AGX_E_INVALID, "agx_ingest_gray: null buffer");
    const agx_config &c = ctx->cfg;
    DeviceGuard g(c.device);
    IngestGrayParams p;
    p.small = d_small;
    p.cmd = d_cmd;
    p.ring = ctx->ring;
    p.head_in = ctx->head[ctx->cur_head];
    p.head_out = ctx->head[ctx->cur_head ^ 1];
    p.oh = c.obs_h;
    p.ow = c.obs_w;
    p.fs = c.frame_stack;
    ingest_range(ctx, p, &IngestGrayParams::small, (size_t)2 * c.obs_h * c.obs_w);
    const int words = c.obs_h * c.obs_w / 4;
    hipLaunchKernelGGL(k_ingest_gray, dim3((words + kThreads - 1) / kThreads, ctx->rng_n), dim3(kThreads), 0,
                       S(stream), p);
    ingest_carry(ctx, stream);
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_head ^= 1;
    return AGX_OK;
}

int agx_ingest_rgb(agx_ctx *ctx, const uint8_t *d_frames, const uint8_t *d_cmd, int gray_mode, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    if (!d_frames || !d_cmd) return fail(ctx, AGX_E_INVALID, "agx_ingest_rgb: null buffer");
    if (!full_range(ctx)) return refuse_range(ctx, "agx_ingest_rgb");
    const agx_config &c = ctx->cfg;
    DeviceGuard g(c.device);
    IngestRgbParams p;
    p.frames = d_frames;
    p.cmd = d_cmd;
    p.ring = ctx->ring;
    p.head_in = ctx->head[ctx->cur_head];
    p.head_out = ctx->head[ctx->cur_head ^ 1];
    p.oh = c.obs_h;
    p.ow = c.obs_w;
    p.fs = c.frame_stack;
    if (gray_mode != AGX_GRAY_CV15 && gray_mode != AGX_GRAY_CV14 && gray_mode != AGX_GRAY_NONE)
        return fail(ctx, AGX_E_INVALID, "agx_ingest_rgb: unknown gray_mode %d", gray_mode);
    if ((gray_mode == AGX_GRAY_NONE) != (ctx->planes == 3))
        return fail(ctx, AGX_E_STATE, "agx_ingest_rgb: gray_mode %d on a %s context (AGX_GRAY_NONE <=> AGX_FRAME_RGB)", gray_mode,
                    ctx->planes == 3 ? "colour" : "gray");
    if (gray_mode == AGX_GRAY_NONE) {
        // colour: the three channels to three planar ring planes (k_ingest_rgb_planar), 16 pixels per thread where every plane
        // is 16-B aligned
        const int px = c.obs_h * c.obs_w, per = px % 16 == 0 ? 16 : 4, groups = px / per;
        const dim3 grid((groups + kThreads - 1) / kThreads, c.num_envs);
        if (per == 16) AGX_LAUNCH(0, k_ingest_rgb_planar<16>, grid, dim3(kThreads), 0, S(stream), p);
        else AGX_LAUNCH(0, k_ingest_rgb_planar<4>, grid, dim3(kThreads), 0, S(stream), p);
        AGX_HIP(ctx, hipGetLastError());
        ctx->cur_head ^= 1;
        return AGX_OK;
    }
    // cv2.cvtColor(rgb, COLOR_BGR2GRAY): channel 0 gets the blue weight (dmc_env.py:181-182 hands it an RGB render)
    switch (gray_mode) {
        case AGX_GRAY_CV15: p.k0 = 3735, p.k1 = 19235, p.k2 = 9798, p.shift = 15; break;   // OpenCV 4.x: BY15 GY15 RY15
        case AGX_GRAY_CV14: p.k0 = 1868, p.k1 = 9617, p.k2 = 4899, p.shift = 14; break;    // OpenCV <= 3.x: B2Y G2Y R2Y
        default: return fail(ctx, AGX_E_INVALID, "agx_ingest_rgb: unknown gray_mode %d", gray_mode);
    }
    const int words = c.obs_h * c.obs_w / 4;
    AGX_LAUNCH(0, k_ingest_rgb, dim3((words + kThreads - 1) / kThreads, c.num_envs), dim3(kThreads), 0, S(stream), p);
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_head ^= 1;
    return AGX_OK;
}

// ---------------------------------------------------------------- K0
static int stack_launch(agx_ctx *ctx, int which, const uint8_t *in_u8, uint8_t *out_u8, float *out_f32, void *stream) {
    const agx_config &c = ctx->cfg;
    DeviceGuard g(c.device);
    StackParams p;
    p.ring = ctx->ring;
    p.head = ctx->head[ctx->cur_head];
    p.in_u8 = in_u8;
    p.out_u8 = out_u8;
    p.out_f32 = out_f32;
    p.words = c.obs_h * c.obs_w / 4;
    p.fs = c.frame_stack;
    int en = c.num_envs;
    if (which == 2) {                          // agx_observe_full acts on the context's env range (get / set: the whole batch)
        const size_t lo = (size_t)ctx->rng_lo, row = (size_t)c.frame_stack * ctx->planes * c.obs_h * c.obs_w;
        p.ring += lo * row;
        p.head += lo;
        p.out_f32 = reinterpret_cast<float *>(reinterpret_cast<char *>(out_f32) + lo * obs_row_bytes(ctx, false));
        en = ctx->rng_n;
    }
    const dim3 grid((p.words + kThreads - 1) / kThreads, c.frame_stack * ctx->planes, en);
    with_planes(ctx->planes, [&](auto pc) {
        constexpr int NC = decltype(pc)::value;
        if (which == 0)
            hipLaunchKernelGGL(k_stack_u8<NC>, grid, dim3(kThreads), 0, S(stream), p);
        else if (which == 1)
            hipLaunchKernelGGL(k_set_stack<NC>, grid, dim3(kThreads), 0, S(stream), p);
        else
            with_obs_type(ctx->obs_type, [&](auto tag) {
                using OT = decltype(tag);
                hipLaunchKernelGGL((k_full<OT, NC>), grid, dim3(kThreads), 0, S(stream), p);
                return 0;
            });
        return 0;
    });
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_observe_full(agx_ctx *ctx, float *d_obs, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    if (!d_obs) return fail(ctx, AGX_E_INVALID, "agx_observe_full: null buffer");
    return stack_launch(ctx, 2, nullptr, nullptr, d_obs, stream);
}
int agx_get_stack_u8(agx_ctx *ctx, uint8_t *d_out, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    if (!d_out) return fail(ctx, AGX_E_INVALID, "agx_get_stack_u8: null buffer");
    return stack_launch(ctx, 0, nullptr, d_out, nullptr, stream);
}
int agx_set_stack_u8(agx_ctx *ctx, const uint8_t *d_in, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    if (!d_in) return fail(ctx, AGX_E_INVALID, "agx_set_stack_u8: null buffer");
    return stack_launch(ctx, 1, d_in, nullptr, nullptr, stream);
}

// ---------------------------------------------------------------- fovea state
int agx_fovea_reset(agx_ctx *ctx, const uint8_t *d_mask, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    const agx_config &c = ctx->cfg;
    if (!has_fovea(c)) return fail(ctx, AGX_E_STATE, "agx_fovea_reset: context has no fovea (AGX_KIND_BASE)");
    DeviceGuard g(c.device);
    FovResetParams p;
    p.mask = d_mask ? d_mask + ctx->rng_lo : nullptr;
    p.loc = ctx->loc[ctx->cur_fov] + 2 * (size_t)ctx->rng_lo;
    p.res = ctx->res[ctx->cur_fov] + 2 * (size_t)ctx->rng_lo;
    p.init_r = ctx->init_r;
    p.init_c = ctx->init_c;
    p.fh = c.fov_h;
    p.fw = c.fov_w;
    p.n = ctx->rng_n;
    hipLaunchKernelGGL(k_fovea_reset, dim3((p.n + kThreads - 1) / kThreads), dim3(kThreads), 0, S(stream), p);
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

int agx_get_fov_state(agx_ctx *ctx, int32_t *d_fov_loc, int32_t *d_fov_res, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    const agx_config &c = ctx->cfg;
    if (!has_fovea(c)) return fail(ctx, AGX_E_STATE, "agx_get_fov_state: context has no fovea");
    DeviceGuard g(c.device);
    const size_t b = (size_t)c.num_envs * 2 * sizeof(int32_t);
    if (d_fov_loc) AGX_HIP(ctx, hipMemcpyAsync(d_fov_loc, ctx->loc[ctx->cur_fov], b, hipMemcpyDeviceToDevice, S(stream)));
    if (d_fov_res) AGX_HIP(ctx, hipMemcpyAsync(d_fov_res, ctx->res[ctx->cur_fov], b, hipMemcpyDeviceToDevice, S(stream)));
    return AGX_OK;
}

int agx_set_fov_state(agx_ctx *ctx, const int32_t *d_fov_loc, const int32_t *d_fov_res, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    const agx_config &c = ctx->cfg;
    if (!has_fovea(c)) return fail(ctx, AGX_E_STATE, "agx_set_fov_state: context has no fovea");
    DeviceGuard g(c.device);
    const size_t b = (size_t)c.num_envs * 2 * sizeof(int32_t);
    if (d_fov_loc) AGX_HIP(ctx, hipMemcpyAsync(ctx->loc[ctx->cur_fov], d_fov_loc, b, hipMemcpyDeviceToDevice, S(stream)));
    if (d_fov_res) AGX_HIP(ctx, hipMemcpyAsync(ctx->res[ctx->cur_fov], d_fov_res, b, hipMemcpyDeviceToDevice, S(stream)));
    return AGX_OK;
}

// ---------------------------------------------------------------- K2/K3/K4

int agx_fovea_fixed(agx_ctx *ctx, const void *d_action, int action_dtype, const uint8_t *d_mask, float *d_obs,
                    int32_t *d_fov_loc, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    const agx_config &c = ctx->cfg;
    if (c.kind != AGX_KIND_FIXED) return fail(ctx, AGX_E_STATE, "agx_fovea_fixed on a context of kind %d", c.kind);
    if (!d_obs) return fail(ctx, AGX_E_INVALID, "agx_fovea_fixed: null obs buffer");
    int rc = check_dt(ctx, d_action, action_dtype);
    if (rc) return rc;
    DeviceGuard g(c.device);
    FovParams p = fov_params(ctx, d_action, action_dtype, nullptr, d_mask, d_obs, d_fov_loc, nullptr);
    fov_range(ctx, p);
    const dim3 grid(c.frame_stack * ctx->planes, ctx->rng_n), block(kThreads);
#ifdef AGX_EXPERIMENTS
    if (!exp_fovea_fixed(ctx, p, stream))
#endif
        with_planes(ctx->planes, [&](auto pc) {
            return with_obs_type(ctx->obs_type, [&](auto tag) {
                return with_mode(c.out_mode, [&](auto mode) {
                    return with_geom(ctx->plan.headline, geom_r(c), [&](auto g) {
                        AGX_LAUNCH(1, (k_fovea_fixed<decltype(g), decltype(mode)::value, decltype(tag), decltype(pc)::value>), grid, block,
                                   ctx->plan.lds, S(stream), g, p);
                        return 0;
                    });
                });
            });
        });
    fov_carry(ctx, stream);
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_fov ^= 1;
    return AGX_OK;
}

// ---------------------------------------------------------------- fused step (K1 + K2)
int agx_step_fixed(agx_ctx *ctx, const uint8_t *d_frames, const uint8_t *d_cmd, const void *d_action, int action_dtype,
                   float *d_obs, int32_t *d_fov_loc, void *mid_event, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    const agx_config &c = ctx->cfg;
    if (ctx->planes != 1) return refuse_rgb(ctx, "agx_step_fixed");
    if (c.kind != AGX_KIND_FIXED) return fail(ctx, AGX_E_STATE, "agx_step_fixed on a context of kind %d", c.kind);
    if (!full_range(ctx)) return refuse_range(ctx, "agx_step_fixed");
    if (!d_frames || !d_cmd || !d_obs) return fail(ctx, AGX_E_INVALID, "agx_step_fixed: null buffer");
    int rc = check_dt(ctx, d_action, action_dtype);
    if (rc) return rc;
    // The step as the library ships it: the two stand-alone launches (ingest, then fovea), the fastest form measured.  The
    // other forms of this call that were built and measured slower or equal (heterogeneous fused launch + tail, env-range
    // parts on internal streams, one workgroup per env) live in the experiments build only.
#ifdef AGX_EXPERIMENTS
    if (exp_step_fixed(ctx, d_frames, d_cmd, d_action, action_dtype, d_obs, d_fov_loc, mid_event, stream, &rc)) return rc;
#endif
    rc = agx_ingest(ctx, d_frames, d_cmd, stream);
    if (rc) return rc;
    if (mid_event) AGX_HIP(ctx, hipEventRecord(static_cast<hipEvent_t>(mid_event), S(stream)));
    return agx_fovea_fixed(ctx, d_action, action_dtype, nullptr, d_obs, d_fov_loc, stream);
}

int agx_fovea_peripheral(agx_ctx *ctx, const void *d_action, int action_dtype, const uint8_t *d_mask, float *d_obs,
                         int32_t *d_fov_loc, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    const agx_config &c = ctx->cfg;
    if (c.kind != AGX_KIND_PERIPHERAL) return fail(ctx, AGX_E_STATE, "agx_fovea_peripheral on a context of kind %d", c.kind);
    if (!d_obs) return fail(ctx, AGX_E_INVALID, "agx_fovea_peripheral: null obs buffer");
    int rc = check_dt(ctx, d_action, action_dtype);
    if (rc) return rc;
    DeviceGuard g(c.device);
    FovParams p = fov_params(ctx, d_action, action_dtype, nullptr, d_mask, d_obs, d_fov_loc, nullptr);
    fov_range(ctx, p);
    const FovPlan &pl = ctx->plan;
    const dim3 grid(c.frame_stack * ctx->planes, ctx->rng_n), block(kThreads);     // rng_n: the envs of the launch
    with_planes(ctx->planes, [&](auto pc) {
    constexpr int NC = decltype(pc)::value;
    return with_obs_type(ctx->obs_type, [&](auto tag) {
    using OT = decltype(tag);
    if (pl.form == kFormPer3) {
        const PGeomR pg{c.obs_h, c.obs_w, c.fov_h, c.fov_w, c.per_h, c.per_w};
        using GS = PGeomS<84, 84, 30, 30, 20, 20>;
        if (pl.headline && pl.mt == 12) AGX_LAUNCH(1, (k_fovea_peripheral3<GS, 12, OT, NC>), grid, block, pl.lds, S(stream), GS{}, ctx->p3, p);
        else if (pl.headline) AGX_LAUNCH(1, (k_fovea_peripheral3<GS, 4, OT, NC>), grid, block, pl.lds, S(stream), GS{}, ctx->p3, p);
        else if (pl.mt == 4) AGX_LAUNCH(1, (k_fovea_peripheral3<PGeomR, 4, OT, NC>), grid, block, pl.lds, S(stream), pg, ctx->p3, p);
        else if (pl.mt == 8) AGX_LAUNCH(1, (k_fovea_peripheral3<PGeomR, 8, OT, NC>), grid, block, pl.lds, S(stream), pg, ctx->p3, p);
        else if (pl.mt == 12) AGX_LAUNCH(1, (k_fovea_peripheral3<PGeomR, 12, OT, NC>), grid, block, pl.lds, S(stream), pg, ctx->p3, p);
        else AGX_LAUNCH(1, (k_fovea_peripheral3<PGeomR, 16, OT, NC>), grid, block, pl.lds, S(stream), pg, ctx->p3, p);
    } else if (pl.form == kFormPeripheral2) {
        PerParams g;
        for (int k = 0; k < 4; ++k) {
            g.t[k].ln = ctx->per_ln[k];
            g.t[k].w = ctx->per_w[k];
            g.t[k].maxt = ctx->per_maxt[k];
        }
        g.t[0].n_out = c.per_w; g.t[1].n_out = c.per_h; g.t[2].n_out = c.obs_w; g.t[3].n_out = c.obs_h;
        g.oh = c.obs_h; g.ow = c.obs_w; g.fh = c.fov_h; g.fw = c.fov_w; g.ph = c.per_h; g.pw = c.per_w;
        g.same = pl.same;
        switch (pl.mt) {
            case 2: AGX_LAUNCH(1, (k_fovea_peripheral2<2, OT, NC>), grid, block, pl.lds, S(stream), g, p); break;
            case 4: AGX_LAUNCH(1, (k_fovea_peripheral2<4, OT, NC>), grid, block, pl.lds, S(stream), g, p); break;
            case 8: AGX_LAUNCH(1, (k_fovea_peripheral2<8, OT, NC>), grid, block, pl.lds, S(stream), g, p); break;
            case 12: AGX_LAUNCH(1, (k_fovea_peripheral2<12, OT, NC>), grid, block, pl.lds, S(stream), g, p); break;
            case 16: AGX_LAUNCH(1, (k_fovea_peripheral2<16, OT, NC>), grid, block, pl.lds, S(stream), g, p); break;
            default: AGX_LAUNCH(1, (k_fovea_peripheral2<0, OT, NC>), grid, block, pl.lds, S(stream), g, p); break;
        }
    } else {
        hipLaunchKernelGGL((k_fovea_generic<AGX_KIND_PERIPHERAL, OT, NC>), grid, block, pl.lds, S(stream), geom_r(c), p);
    }
    return 0;
    });
    });
    fov_carry(ctx, stream);
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_fov ^= 1;
    return AGX_OK;
}

int agx_fovea_flexible(agx_ctx *ctx, const void *d_action, int action_dtype, const int32_t *d_action_type,
                       const uint8_t *d_mask, float *d_obs, int32_t *d_fov_loc, int32_t *d_fov_res, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    const agx_config &c = ctx->cfg;
    if (c.kind != AGX_KIND_FLEXIBLE) return fail(ctx, AGX_E_STATE, "agx_fovea_flexible on a context of kind %d", c.kind);
    if (!d_obs) return fail(ctx, AGX_E_INVALID, "agx_fovea_flexible: null obs buffer");
    int rc = check_dt(ctx, d_action, action_dtype);
    if (rc) return rc;
    DeviceGuard g(c.device);
    FovParams p = fov_params(ctx, d_action, action_dtype, d_action_type, d_mask, d_obs, d_fov_loc, d_fov_res);
    fov_range(ctx, p);
    const FovPlan &pl = ctx->plan;
    const dim3 grid(c.frame_stack * ctx->planes, ctx->rng_n), block(kThreads);     // rng_n: the envs of the launch
    with_planes(ctx->planes, [&](auto pc) {
    constexpr int NC = decltype(pc)::value;
    return with_obs_type(ctx->obs_type, [&](auto tag) {
    using OT = decltype(tag);
    if (pl.form == kFormFlex3) {
        return with_geom(pl.headline, geom_r(c), [&](auto g) {
            AGX_LAUNCH(1, (k_fovea_flexible3<decltype(g), OT, NC>), grid, block, pl.lds, S(stream), g, ctx->f3, p);
            return 0;
        });
    } else if (pl.form == kFormRaw3) {
        return with_geom(pl.headline, geom_r(c), [&](auto g) {
            using G = decltype(g);
            if (c.out_mode == AGX_OUT_MASK) AGX_LAUNCH(1, (k_fovea_flexible_raw3<G, AGX_OUT_MASK, OT, NC>), grid, block, pl.lds, S(stream), g, ctx->fr, p);
            else AGX_LAUNCH(1, (k_fovea_flexible_raw3<G, AGX_OUT_RAW, OT, NC>), grid, block, pl.lds, S(stream), g, ctx->fr, p);
            return 0;
        });
    } else if (pl.form == kFormFlexible2) {
        const FlexParams g = flex_params(ctx);
        if (c.out_mode == AGX_OUT_RESIZE) AGX_LAUNCH(1, (k_fovea_flexible2<true, OT, NC>), grid, block, pl.lds, S(stream), g, p);
        else AGX_LAUNCH(1, (k_fovea_flexible2<false, OT, NC>), grid, block, pl.lds, S(stream), g, p);
    } else {
        hipLaunchKernelGGL((k_fovea_generic<AGX_KIND_FLEXIBLE, OT, NC>), grid, block, pl.lds, S(stream), geom_r(c), p);
    }
    return 0;
    });
    });
    fov_carry(ctx, stream);
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_fov ^= 1;
    return AGX_OK;
}

// the crop launches of the packed form read the final state (cur_fov has been flipped by the caller) and write ragged crops
static FovParams packed_fov_params(agx_ctx *ctx, float *d_packed, int64_t capacity_floats, int64_t *d_offsets) {
    FovParams p = fov_params(ctx, nullptr, 0, nullptr, nullptr, d_packed, nullptr, nullptr);
    p.packed = d_packed;
    p.packed_off = d_offsets;
    p.packed_cap = capacity_floats;
    return p;
}

// the crop launch of the packed form on the raw3 plan
static int packed_crops_raw3(agx_ctx *ctx, float *d_packed, int64_t capacity_floats, int64_t *d_offsets, void *stream) {
    const agx_config &c = ctx->cfg;
    const FovParams p = packed_fov_params(ctx, d_packed, capacity_floats, d_offsets);
    FlexRawParams fr = ctx->fr;
    fr.local_off = ctx->pack_local;
    fr.block_tot = ctx->pack_block;
    fr.offsets = d_offsets;
    const dim3 grid(c.frame_stack, c.num_envs), block(kThreads);
#ifdef AGX_EXPERIMENTS
    if (!exp_packed_crops_raw3(ctx, fr, p, stream))
#endif
        with_geom(ctx->plan.headline, geom_r(c), [&](auto g) {
            AGX_LAUNCH(1, (k_fovea_flexible_raw3<decltype(g), kRawPacked>), grid, block, ctx->plan.lds, S(stream), g, fr, p);
            return 0;
        });
    AGX_HIP(ctx, hipGetLastError());
    return AGX_OK;
}

// what both packed entry points require of the context
static int packed_check(agx_ctx *ctx, const char *who) {
    const agx_config &c = ctx->cfg;
    if (ctx->planes != 1) return refuse_rgb(ctx, who);
    if (!full_range(ctx)) return refuse_range(ctx, who);
    if (c.kind != AGX_KIND_FLEXIBLE || c.out_mode != AGX_OUT_RAW)
        return fail(ctx, AGX_E_STATE, "%s needs a flexible context in raw-crop mode (kind %d, out_mode %d)", who, c.kind, c.out_mode);
    if (ctx->obs_type != AGX_OBS_F32)
        return fail(ctx, AGX_E_STATE, "%s: the packed ragged crops are float32 only (context has AGX_OBS_* 0x%x)", who, ctx->obs_type);
    return AGX_OK;
}

int agx_fovea_flexible_packed(agx_ctx *ctx, const void *d_action, int action_dtype, const int32_t *d_action_type,
                              float *d_packed, int64_t capacity_floats, int64_t *d_offsets, int32_t *d_fov_loc,
                              int32_t *d_fov_res, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    const agx_config &c = ctx->cfg;
    int rc = packed_check(ctx, "agx_fovea_flexible_packed");
    if (rc) return rc;
    if (!d_packed || !d_offsets || capacity_floats < 0) return fail(ctx, AGX_E_INVALID, "agx_fovea_flexible_packed: null buffer");
    if ((rc = check_dt(ctx, d_action, action_dtype))) return rc;
    DeviceGuard g(c.device);
    // launch 1: every env's new fov_loc / fov_res (fov_env.py:300-324), its crop size, and level 1 of the exclusive scan
    // (block-local offsets + block totals)
    const FlexScanParams q = packed_scan_params(ctx, d_action, action_dtype, d_action_type, d_fov_loc, d_fov_res);
    const int nb = (c.num_envs + kScanEnvsPerBlock - 1) / kScanEnvsPerBlock;
    hipLaunchKernelGGL(k_flex_state_scan, dim3(nb), dim3(kThreads), 0, S(stream), q);
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_fov ^= 1;                   // the state is final from here on; the crop launch only reads it
    // launch 2: the crops (squeezed to fov_size and back iff rows > fov rows, fov_env.py:283-287) at their offsets
    if (ctx->plan.packed == kPackedRaw3) return packed_crops_raw3(ctx, d_packed, capacity_floats, d_offsets, stream);
    const FovParams p = packed_fov_params(ctx, d_packed, capacity_floats, d_offsets);
    // geometries outside the raw3 plan: offsets as a launch of their own, then the pass-by-pass crop kernel, which writes
    // the (unchanged) state through into the other half of the double buffer
    hipLaunchKernelGGL(k_flex_finish_offsets, dim3((c.num_envs + 1 + kThreads - 1) / kThreads), dim3(kThreads), 0, S(stream),
                       ctx->pack_local, ctx->pack_block, d_offsets, (int)c.num_envs);
    const dim3 grid(c.frame_stack, c.num_envs), block(kThreads);
    if (ctx->plan.packed == kPackedOffsetsFlexible2)
        AGX_LAUNCH(1, k_fovea_flexible2<false>, grid, block, ctx->plan.lds, S(stream), flex_params(ctx), p);
    else
        hipLaunchKernelGGL((k_fovea_generic<AGX_KIND_FLEXIBLE>), grid, block, ctx->plan.lds, S(stream), geom_r(c), p);
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_fov ^= 1;
    return AGX_OK;
}

int agx_step_flexible_packed(agx_ctx *ctx, const uint8_t *d_screens, int screens, const uint8_t *d_cmd, const void *d_action,
                             int action_dtype, const int32_t *d_action_type, float *d_packed, int64_t capacity_floats,
                             int64_t *d_offsets, int32_t *d_fov_loc, int32_t *d_fov_res, void *stream) {
    if (!ctx) return AGX_E_INVALID;
    const agx_config &c = ctx->cfg;
    int rc = packed_check(ctx, "agx_step_flexible_packed");
    if (rc) return rc;
    if (!d_screens || !d_cmd || !d_packed || !d_offsets || capacity_floats < 0)
        return fail(ctx, AGX_E_INVALID, "agx_step_flexible_packed: null buffer");
    if (screens & ~(AGX_SCREENS_GRAY | AGX_SCREENS_COMPACT))
        return fail(ctx, AGX_E_INVALID, "agx_step_flexible_packed: unknown screen layout bits 0x%x", screens);
    if ((rc = check_dt(ctx, d_action, action_dtype))) return rc;
    const bool gray = (screens & AGX_SCREENS_GRAY) != 0, compact = (screens & AGX_SCREENS_COMPACT) != 0;
    // the two-launch form needs the band12 ingest plan for this layout and the raw3 crop plan; everything else (and
    // AGX_STEP_PACKED_UNFUSED=1, for A/B runs) is the three launches of the stand-alone entry points, same results
    const int layout = (compact ? kK1RgbCompact : kK1Rgb) + (gray ? 1 : 0);
    const K1Launch &l = ctx->k1l[layout];
    const int nb = (c.num_envs + kScanEnvsPerBlock - 1) / kScanEnvsPerBlock;
    const bool fused = c.obs_h == c.obs_w && l.band12 && ctx->plan.packed == kPackedRaw3 && c.num_envs + nb <= 65535 &&
                       ctx->tune.packed_unfused == 0 && ctx->tune.packed_wave == 0 &&
                       ctx->tune.pipe_parts == 0 && ctx->tune.wave == 0 && ctx->tune.pair12 == 0 && ctx->ingest_t == 256;
    if (!fused) {
        if (compact) rc = gray ? agx_ingest_gray_raw_compact(ctx, d_screens, d_cmd, stream) : agx_ingest_compact(ctx, d_screens, d_cmd, stream);
        else rc = gray ? agx_ingest_gray_raw(ctx, d_screens, d_cmd, stream) : agx_ingest(ctx, d_screens, d_cmd, stream);
        if (rc) return rc;
        return agx_fovea_flexible_packed(ctx, d_action, action_dtype, d_action_type, d_packed, capacity_floats, d_offsets, d_fov_loc,
                                         d_fov_res, stream);
    }
    DeviceGuard g(c.device);
    const IngestParams p = ingest_params(ctx, d_screens, d_cmd, layout);
    const FlexScanParams q = packed_scan_params(ctx, d_action, action_dtype, d_action_type, d_fov_loc, d_fov_res);
    // launch 1: the scan blocks (first rows of the grid) + the ingest bands
    const dim3 grid(l.nbands, nb + c.num_envs), block(kThreads);
    const size_t lds = l.lds;
    if (compact) {
        if (gray) AGX_LAUNCH(0, (k_ingest_full12_flexscan<true, true>), grid, block, lds, S(stream), p, q, nb);
        else AGX_LAUNCH(0, (k_ingest_full12_flexscan<false, true>), grid, block, lds, S(stream), p, q, nb);
    } else {
        if (gray) AGX_LAUNCH(0, (k_ingest_full12_flexscan<true, false>), grid, block, lds, S(stream), p, q, nb);
        else AGX_LAUNCH(0, (k_ingest_full12_flexscan<false, false>), grid, block, lds, S(stream), p, q, nb);
    }
    AGX_HIP(ctx, hipGetLastError());
    ctx->cur_head ^= 1;
    ctx->cur_fov ^= 1;
    // launch 2: the crops
    return packed_crops_raw3(ctx, d_packed, capacity_floats, d_offsets, stream);
}

}  // extern "C"

#include "agx_loop_impl.h"
#include "agx_hostout_impl.h"
#include "agx_history_impl.h"
#include "agx_glimpse_impl.h"
#include "agx_replay_impl.h"
#include "agx_steplog_impl.h"
#include "agx_priority_impl.h"
#include "agx_augment_impl.h"
#include "agx_sequence_impl.h"
#include "agx_rollout_impl.h"
#include "agx_vtrace_impl.h"
#include "agx_minibatch_impl.h"
#include "agx_retrace_impl.h"
#include "agx_chunks_host.h"
