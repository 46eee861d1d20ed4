// CPU harness for the host-built operator tables of k_fovea_flexible3 (active-gym_amd/csrc/agx_host_tables.h) and the
// host plan (active-gym_amd/csrc/agx_plan.h).
// Replays the kernel's arithmetic (same tables, same float32 operation order, same index rules) on the host and
// compares it with the reference chain  crop -> [Resize(fov) -> Resize(res) iff rh > fov_h] -> Resize(obs)
// (fov_env.py:276-298) evaluated pass by pass in double with the plain per-axis operators.  Also checks the memory
// rules the kernel relies on (every LDS index inside the regions agx_create sizes).
// Build: hipcc -std=c++17 -I include -I active-gym_amd/csrc tests/host_tables_harness.cpp -o <out>   (host code only)
// Usage: harness oh ow fh fw antialias          (k_fovea_flexible3 tables) -> "max_err <e> cases <n>" | "unsupported"
//        harness per oh ow ph pw antialias      (k_fovea_peripheral3 tables + unit_fast over all 256 values)
//        harness raw oh ow fh fw antialias      (k_fovea_flexible_raw3 tables: raw-crop / mask-out / packed forms)
//        harness plan oh ow fh fw ph pw antialias resize|raw|mask [knob=1 ...]
//                                               which kernel form agx_create + the launch code select for each kind, and why
//        harness k1plan obs [knob=1 ...]        which K1 ingest form each screen layout selects at obs x obs, and what it branches on
//        knob: generic flex_v2 per_v2 no_full - the context's fallback knobs (agx_plan.h: Knobs); none given = none set
//        harness k1tables obs                   the K1 tables of build_k1: x0 x1 a0 a1 y0 y1 b0 b1 and the source-row list
//        harness carve oh ow fh fw resize|mask  k_history_memory's LDS regions (fixed_carve) against memory_lds, P = 1, 3, 8
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "agx_plan.h"

using namespace agx;
using namespace agx::rows;

static std::vector<double> apply_w(const Op &op, const std::vector<double> &x, int rows_, int n_in) {
    std::vector<double> y((size_t)rows_ * op.size());
    for (int r = 0; r < rows_; ++r)
        for (size_t i = 0; i < op.size(); ++i) {
            double a = 0;
            for (size_t k = 0; k < op[i].w.size(); ++k) a += op[i].w[k] * x[(size_t)r * n_in + op[i].lo + k];
            y[(size_t)r * op.size() + i] = a;
        }
    return y;
}
static std::vector<double> apply_h(const Op &op, const std::vector<double> &x, int cols, int n_in) {
    (void)n_in;
    std::vector<double> y(op.size() * (size_t)cols);
    for (size_t i = 0; i < op.size(); ++i)
        for (int c = 0; c < cols; ++c) {
            double a = 0;
            for (size_t k = 0; k < op[i].w.size(); ++k) a += op[i].w[k] * x[(size_t)(op[i].lo + k) * cols + c];
            y[i * cols + c] = a;
        }
    return y;
}
// torchvision Resize(size)(x[h][w]) in double: W pass then H pass (identity when the size matches)
static std::vector<double> resize(const std::vector<double> &x, int h, int w, int nh, int nw, bool aa) {
    if (h == nh && w == nw) return x;
    return apply_h(resize_axis(h, nh, aa), apply_w(resize_axis(w, nw, aa), x, h, w), nw, h);
}

static int per_main(int argc, char **argv) {
    if (argc < 7) return 2;
    for (int k = 0; k < 256; ++k)
        if (unit_fast((float)k) != (float)k / 255.0f) { printf("unit_fast(%d) is not the IEEE quotient\n", k); return 1; }
    agx_config c{};
    c.obs_h = atoi(argv[2]); c.obs_w = atoi(argv[3]); c.per_h = atoi(argv[4]); c.per_w = atoi(argv[5]);
    c.antialias = atoi(argv[6]);
    const Per3Host h = build_per3(c);
    if (!h.ok) { printf("unsupported\n"); return 0; }
    const int oh = c.obs_h, ow = c.obs_w, ph = c.per_h, pw = c.per_w, MT = h.mt;
    const bool aa = c.antialias != 0;
    std::mt19937 rng(11);
    std::vector<unsigned char> raw((size_t)oh * ow + 16, 0);
    for (size_t i = 0; i < (size_t)oh * ow; ++i) raw[i] = (unsigned char)(rng() & 0xFF);
    std::vector<float> A((size_t)oh * pw), B((size_t)ph * pw), C((size_t)ph * ow);
    for (int y = 0; y < oh; ++y)
        for (int x = 0; x < pw; ++x) {
            const int off = y * ow + h.lo0[x];
            if (((off & ~3) + 4 * ((MT + 6) / 4)) > oh * ow + 16) { printf("pass-0 read past the pad\n"); return 1; }
            float acc = 0.f;
            for (int q = 0; q < MT; ++q) acc = fmaf(h.w0[(size_t)x * MT + q], (float)raw[off + q], acc);
            A[(size_t)y * pw + x] = acc;
        }
    for (int y = 0; y < ph; ++y)
        for (int x = 0; x < pw; ++x) {
            if (h.lo1[y] + MT > oh) { printf("pass-1 row past A\n"); return 1; }
            float acc = 0.f;
            for (int q = 0; q < MT; ++q) acc = fmaf(h.w1[(size_t)y * MT + q], A[(size_t)(h.lo1[y] + q) * pw + x], acc);
            B[(size_t)y * pw + x] = acc;
        }
    for (int y = 0; y < ph; ++y)
        for (int x = 0; x < ow; ++x) {
            const Tap t = h.x2[x];
            if (t.lo >= pw || t.aux >= pw) { printf("pass-2 column\n"); return 1; }
            C[(size_t)y * ow + x] = fmaf(t.b, B[(size_t)y * pw + t.aux], t.a * B[(size_t)y * pw + t.lo]);
        }
    std::vector<double> x((size_t)oh * ow);
    for (size_t i = 0; i < x.size(); ++i) x[i] = (double)raw[i] / 255.0;
    const std::vector<double> ref = resize(resize(x, oh, ow, ph, pw, aa), ph, pw, oh, ow, aa);
    double worst = 0;
    for (int y = 0; y < oh; ++y) {
        const int4 e = h.y3[y];
        const int i0 = e.x & 0xFF, i1 = e.x >> 8;
        if (i0 >= ph || i1 >= ph) { printf("pass-3 row\n"); return 1; }
        float w0, w1;
        memcpy(&w0, &e.y, 4); memcpy(&w1, &e.z, 4);
        for (int xx = 0; xx < ow; ++xx) {
            const float o = fmaf(w1, C[(size_t)i1 * ow + xx], w0 * C[(size_t)i0 * ow + xx]);
            const double err = std::fabs((double)o - ref[(size_t)y * ow + xx]);
            if (!(err <= worst)) worst = err;
        }
    }
    printf("max_err %.3e mt %d lds %zu\n", worst, MT, h.lds);
    return 0;
}


// k_fovea_flexible_raw3 (agx_k4_raw3.h): the squeeze-and-expand-back chain of the raw-crop / mask-out / packed forms.
// Replays the kernel on its LDS image of the window (rows [r, r + rh + 8) clipped to the frame, of each row the dword-aligned
// column span holding [c, c + rw), a dword past the frame's end clamped to its last dword) with stale-LDS NaNs everywhere
// else, and compares with  crop -> Resize(fov_size) -> Resize(fov_res)  (fov_env.py:276-287) in double.
static int raw_main(int argc, char **argv) {
    if (argc < 7) return 2;
    agx_config c{};
    c.obs_h = atoi(argv[2]); c.obs_w = atoi(argv[3]); c.fov_h = atoi(argv[4]); c.fov_w = atoi(argv[5]);
    c.antialias = atoi(argv[6]);
    c.out_mode = AGX_OUT_RAW;
    const FlexRawHost h = build_flexraw(c);
    if (!h.ok) { printf("unsupported\n"); return 0; }
    const int oh = c.obs_h, ow = c.obs_w, fh = c.fov_h, fw = c.fov_w;
    const bool aa = c.antialias != 0;
    const int rstep = kThreads / ow, erows = (fh + rstep - 1) / rstep * rstep;
    std::mt19937 rng(11);
    double worst = 0;
    long cases = 0;
    std::vector<unsigned char> R0(h.r0_bytes);
    std::vector<float> D((size_t)h.r1_bytes / 4), E((size_t)h.r0_bytes / 4);
    for (int rh = fh + 1; rh <= oh; ++rh)
        for (int rw = 1 + (rh * 5) % 3; rw <= ow; rw += 3) {
            const int r = (int)(rng() % (unsigned)(oh - rh + 1)), cc = (int)(rng() % (unsigned)(ow - rw + 1));
            std::vector<unsigned char> F((size_t)oh * ow);
            for (auto &b : F) b = (unsigned char)(rng() & 0xFF);
            for (auto &b : R0) b = (unsigned char)(rng() & 0xFF);
            for (auto &v : D) v = NAN;
            for (auto &v : E) v = NAN;
            const int wrows = std::min(rh + 8, oh - r), span = ((cc & 3) + rw + 3) >> 2, wp = span * 4;
            if ((size_t)wrows * wp > (size_t)h.r0_bytes || wp > ow) { printf("image too large rh=%d rw=%d\n", rh, rw); return 1; }
            for (int i = 0; i < wrows * span; ++i) {
                const int y = i / span, q = i - y * span;
                const int src = std::min((r + y) * (ow / 4) + (cc >> 2) + q, oh * ow / 4 - 1);
                memcpy(&R0[(size_t)i * 4], &F[(size_t)src * 4], 4);
            }
            const unsigned char *win = R0.data() + (cc & 3);
            auto in_r0 = [&](const unsigned char *p) { return p >= R0.data() && p < R0.data() + h.r0_bytes; };
            const int Tw = h.wb_meta[rw].x, Th = h.hd_meta[rh].x;
            const int kmax = (std::max(rw, Tw) + 7) >> 3;
            if (8 * kmax > h.dp) { printf("D pitch too small rw=%d\n", rw); return 1; }
            for (int yf = 0; yf < fh; ++yf)
                for (int x = 0; x < 8 * kmax; ++x) {
                    const int lo = h.hd_lo[(size_t)rh * fh + yf];
                    const float *w = &h.hd_w[h.hd_meta[rh].y + (size_t)yf * Th];
                    float acc = 0.f;
                    for (int q = 0; q < Th; ++q) {
                        const unsigned char *p = win + (lo + q) * wp + x;
                        if (!in_r0(p)) { printf("raw read outside R0 rh=%d rw=%d\n", rh, rw); return 1; }
                        acc = fmaf(w[q], (float)*p, acc);
                    }
                    D[(size_t)yf * h.dp + x] = acc;
                }
            if (erows * ow * 4 > h.r0_bytes) { printf("E does not fit R0\n"); return 1; }
            for (int y = 0; y < fh; ++y)
                for (int x = 0; x < ow; ++x) {
                    const int lo = h.wb_lo[(size_t)rw * ow + x];
                    const float *w = &h.wb_w[h.wb_meta[rw].y + (size_t)x * Tw];
                    if (lo < 0 || lo + Tw > 8 * kmax) { printf("D read outside the written columns rw=%d x=%d\n", rw, x); return 1; }
                    float acc = 0.f;
                    for (int q = 0; q < Tw; ++q) acc = fmaf(w[q], D[(size_t)y * h.dp + lo + q], acc);
                    E[(size_t)y * ow + x] = acc;
                }
            std::vector<double> crop((size_t)rh * rw);
            for (int y = 0; y < rh; ++y)
                for (int x = 0; x < rw; ++x) {
                    if (win[y * wp + x] != F[(size_t)(r + y) * ow + cc + x]) { printf("image != frame window rh=%d rw=%d\n", rh, rw); return 1; }
                    crop[(size_t)y * rw + x] = (double)F[(size_t)(r + y) * ow + cc + x] / 255.0;
                }
            const std::vector<double> ref = resize(resize(crop, rh, rw, fh, fw, aa), fh, fw, rh, rw, aa);
            for (int y = 0; y < rh; ++y) {
                const Tap tp = h.hb[(size_t)rh * oh + y];
                if (tp.lo < 0 || tp.aux >= fh) { printf("row tap rh=%d y=%d\n", rh, y); return 1; }
                for (int x = 0; x < rw; ++x) {
                    const float o = fmaf(tp.b, E[(size_t)tp.aux * ow + x], tp.a * E[(size_t)tp.lo * ow + x]);
                    const double err = std::fabs((double)o - ref[(size_t)y * rw + x]);
                    if (!(err <= worst)) worst = err;      // NaN-propagating max
                }
            }
            ++cases;
        }
    printf("max_err %.3e cases %ld lds %zu\n", worst, cases, h.lds(c));
    return 0;
}

// ---- plan report: the kernel form agx_create and the launch code of agx_api.hip select for a geometry, per kind.
// Nothing is restated here: the table builders are the ones agx_create calls (agx_host_tables.h) and the plans come from the
// functions agx_create stores in the context and the launch code switches on (agx_plan.h).  The case table of
// tests/test_geometry_plan_cpu.py is what notices a plan that moved.

// trailing `knob=1` arguments (generic, flex_v2, per_v2, no_full) from argv[from] on; false on anything else
static bool parse_knobs(int argc, char **argv, int from, Knobs &k) {
    for (int i = from; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) return false;
        const std::string name(argv[i], (size_t)(eq - argv[i]));
        int *dst = name == "generic" ? &k.generic : name == "flex_v2" ? &k.flex_v2 : name == "per_v2" ? &k.per_v2
                   : name == "no_full" ? &k.no_full : nullptr;
        if (!dst) return false;
        *dst = atoi(eq + 1);
    }
    return true;
}

static void print_set(const char *key, const std::vector<int2> &meta, int from, int to) {
    bool has[17] = {};
    for (int r = from; r <= to; ++r) has[meta[r].x] = true;
    printf(" %s=", key);
    bool any = false;
    for (int t : {4, 8, 16})
        if (has[t]) { printf("%s%d", any ? "," : "", t); any = true; }
    if (!any) printf("-");
}

// agx_create's LDS check: 0 = accepted, else the bytes in "geometry needs %zu B of LDS per workgroup (limit %zu)"
static size_t create_refusal(const agx_config &c, const Knobs &k) {
    const size_t lds = create_lds(c, k);
    return lds > kMaxLds ? lds : 0;
}

static int plan_main(int argc, char **argv) {
    if (argc < 10) return 2;
    agx_config c{};
    c.obs_h = atoi(argv[2]); c.obs_w = atoi(argv[3]); c.fov_h = atoi(argv[4]); c.fov_w = atoi(argv[5]);
    c.per_h = atoi(argv[6]); c.per_w = atoi(argv[7]); c.antialias = atoi(argv[8]);
    const char *mode = argv[9];
    const int out_mode = !strcmp(mode, "resize") ? AGX_OUT_RESIZE : !strcmp(mode, "mask") ? AGX_OUT_MASK : !strcmp(mode, "raw") ? AGX_OUT_RAW : -1;
    Knobs k;
    if (out_mode < 0 || !parse_knobs(argc, argv, 10, k)) return 2;
    size_t refused;
    // ---- fixed (agx_fovea_fixed)
    c.kind = AGX_KIND_FIXED;
    c.out_mode = out_mode;
    if ((refused = create_refusal(c, k))) printf("fixed form=refused lds=%zu\n", refused);
    else {
        const FovPlan p = plan_fixed(c);
        printf("fixed form=%s lds=%zu\n", p.headline ? "fixed<GeomS>" : "fixed<GeomR>", p.lds);
    }
    // ---- flexible (agx_fovea_flexible, agx_fovea_flexible_packed)
    c.kind = AGX_KIND_FLEXIBLE;
    if ((refused = create_refusal(c, k))) printf("flexible form=refused lds=%zu\n", refused);
    else {
        const Flex3Host f3 = build_flex3(c);
        const FlexRawHost fr = build_flexraw(c);
        HostFamily fam[6];
        const FovPlan p = plan_flexible(c, k, f3, fr, build_families(c, fam));
        const char *form = p.form == kFormFlex3 ? "flex3" : p.form == kFormRaw3 ? "raw3" : p.form == kFormFlexible2 ? "flexible2" : "generic";
        printf("flexible form=%s", form);
        if (!p.why) {
            print_set("W", p.form == kFormFlex3 ? f3.wc_meta : fr.wb_meta, 1, c.obs_w);
            print_set("H", p.form == kFormFlex3 ? f3.hd_meta : fr.hd_meta, c.fov_h + 1, c.obs_h);
            printf(" rstep=%d lds=%zu", kThreads / c.obs_w, p.lds);
        } else
            printf(" why=%s lds=%zu", p.why, p.lds);
        if (p.packed == kPackedRaw3) printf(" packed=raw3");
        else if (p.packed != kPackedNone) printf(" packed=offsets+%s", p.packed == kPackedOffsetsFlexible2 ? "flexible2" : "generic");
        printf("\n");
    }
    // ---- peripheral (agx_fovea_peripheral): always resize_to_full (pipeline.py, fov_env.py:361-364)
    c.kind = AGX_KIND_PERIPHERAL;
    c.out_mode = AGX_OUT_RESIZE;
    if (c.per_h < 1 || c.per_w < 1) printf("peripheral form=none\n");
    else if ((refused = create_refusal(c, k))) printf("peripheral form=refused lds=%zu\n", refused);
    else {
        int nin[4], nout[4], maxt[4];
        per_axes(c, nin, nout);
        for (int a = 0; a < 4; ++a) {
            std::vector<int2> ln;
            std::vector<float> w;
            axis_taps(nin[a], nout[a], c.antialias != 0, ln, w, maxt[a]);
        }
        const FovPlan p = plan_peripheral(c, k, build_per3(c), maxt);
        if (p.form == kFormPer3) printf("peripheral form=per3 mt=%d same=%d lds=%zu\n", p.mt, p.same, p.lds);
        else if (p.form == kFormPeripheral2) printf("peripheral form=peripheral2 mt=%d same=%d why=%s lds=%zu\n", p.mt, p.same, p.why, p.lds);
        else printf("peripheral form=generic same=%d why=%s lds=%zu\n", p.same, p.why, p.lds);
    }
    return 0;
}

// ---- K1 ingest: the plan build_k1 (agx_host_tables.h) hands agx_create, per screen layout, as plan_k1 (agx_plan.h) turns it
// into the launch agx_ingest, agx_ingest_gray_raw and ingest_compact make at plan.band_rows.
//   form=band12 br=12 bands=B
//   form=general br=R bands=B partial=P affine=A xclamp=X yclamp=Y
// partial: the last band has fewer rows than br; affine: source rows from the integer form (whole screens only - compact
// screens always read the packed row table); xclamp / yclamp: some tap pair is one source column / row twice.
static int k1plan_main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int o = atoi(argv[2]);
    if (o < 4 || o > 1024 || (o & 3)) return 2;             // not a size agx_create accepts (k1tables: the same)
    Knobs knobs;
    if (!parse_knobs(argc, argv, 3, knobs)) return 2;
    const K1Host h = build_k1(o, o);
    const K1Plan &q = h.plan;
    bool xclamp = false, yclamp = false;
    for (int i = 0; i < o; ++i) {
        xclamp = xclamp || h.x0[i] == h.x1[i];
        yclamp = yclamp || h.y0[i] == h.y1[i];
    }
    const char *names[4] = {"rgb", "gray", "rgb-compact", "gray-compact"};      // K1Layout
    for (int k = 0; k < 4; ++k) {
        const K1Launch l = plan_k1(q, k, q.band_rows, o, o, knobs);
        if (l.band12) printf("%s form=band12 br=%d bands=%d\n", names[k], l.band_rows, l.nbands);
        else
            printf("%s form=general br=%d bands=%d partial=%d affine=%d xclamp=%d yclamp=%d\n", names[k], l.band_rows, l.nbands,
                   o % l.band_rows != 0, k < kK1RgbCompact && q.y_affine, xclamp, yclamp);
    }
    printf("affine mul=%d add=%d shift=%d ok=%d\n", q.y_mul, q.y_add, q.y_shift, q.y_affine);
    printf("flags adjacent=%d pairs=%d band12_ok=%d compact12_ok=%d rows=%d\n", q.adjacent, q.pairs, q.band12_ok, q.compact12_ok,
           q.rows_touched);
    return 0;
}

static void print_row(const char *key, const std::vector<int> &v) {
    printf("%s", key);
    for (int x : v) printf(" %d", x);
    printf("\n");
}

static int k1tables_main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int o = atoi(argv[2]);
    if (o < 4 || o > 1024 || (o & 3)) return 2;
    const K1Host h = build_k1(o, o);
    print_row("x0", h.x0); print_row("x1", h.x1); print_row("a0", h.a0); print_row("a1", h.a1);
    print_row("y0", h.y0); print_row("y1", h.y1); print_row("b0", h.b0); print_row("b1", h.b1);
    print_row("rows", std::vector<int>(h.src_rows.begin(), h.src_rows.end()));
    print_row("py0", h.py0); print_row("py1", h.py1);
    return 0;
}

// ---- K6 (agx_k6_glimpse.h): the LDS regions k_history_memory touches, from fixed_carve(smem + kMemTableBytes, oh, ow, fh, P) -
// the call the kernel makes - against what memory_lds (agx_plan.h) hands the launch as dynamic LDS:
//   table int2[AGX_GLIMPSE_LIMIT] | raw .. raw + P * fixed_pad | RESIZE: ytab_s .. + oh | H .. + 2 * fh * ow | GeomR: acc .. + oh * ow
// One line per P = 1, 3, 8: "P=p end=<bytes> lds=<memory_lds> aligned=<0|1> headline=<0|1>"; exit status 1 if a region ends behind
// memory_lds or one that the kernel reads as float4 / int4 (window dwords as uint32_t, the table as int2) is misaligned.
static int carve_main(int argc, char **argv) {
    if (argc < 7) return 2;
    agx_config c{};
    c.kind = AGX_KIND_FIXED;
    c.obs_h = atoi(argv[2]); c.obs_w = atoi(argv[3]); c.fov_h = atoi(argv[4]); c.fov_w = atoi(argv[5]);
    c.out_mode = !strcmp(argv[6], "resize") ? AGX_OUT_RESIZE : !strcmp(argv[6], "mask") ? AGX_OUT_MASK : -1;
    if (c.out_mode < 0 || c.obs_h < 1 || c.obs_w < 4 || (c.obs_w & 3) || c.fov_h < 1 || c.fov_h > c.obs_h) return 2;
    const int oh = c.obs_h, ow = c.obs_w, fh = c.fov_h;
    const bool headline = headline_fixed(c);
    // (a real buffer, so that the carve's pointer arithmetic stays inside one object: 8 windows of the largest geometry fit)
    static std::vector<unsigned char> store;
    store.assign((size_t)kMemTableBytes + AGX_GLIMPSE_LIMIT * (size_t)fixed_pad(fh, ow) + (size_t)oh * sizeof(Tap) +
                     (2 * (size_t)fh * ow + (size_t)oh * ow) * sizeof(float) + 64, 0);
    unsigned char *smem = store.data() + ((16 - reinterpret_cast<uintptr_t>(store.data()) % 16) % 16);      // as the kernel's: 16-B aligned
    int bad = 0;
    for (int P : {1, 3, 8}) {
        const FixedCarve lds = fixed_carve(smem + kMemTableBytes, oh, ow, fh, P);
        const auto off = [&](const void *q) { return (size_t)(static_cast<const unsigned char *>(q) - smem); };
        bool aligned = off(lds.raw) % 16 == 0 && fixed_pad(fh, ow) % 16 == 0 && sizeof(int2) * AGX_GLIMPSE_LIMIT <= (size_t)kMemTableBytes;
        // the window image of glimpse i: (fh * ow) / 4 dwords at raw + i * fixed_pad (window_land, window_tail); the mask-out
        // form reads the dword at (row, x), x + 4 <= ow
        size_t end = off(lds.raw + (size_t)(P - 1) * fixed_pad(fh, ow)) + (size_t)((fh * ow) >> 2) * 4;
        end = std::max(end, off(lds.raw + (size_t)P * fixed_pad(fh, ow)));
        if (c.out_mode == AGX_OUT_RESIZE) {
            aligned = aligned && off(lds.ytab_s) % 16 == 0 && sizeof(Tap) == 16;                       // ytab_stage: int4 stores
            end = std::max(end, off(lds.ytab_s + oh));
            float *h1 = lds.H + (size_t)fh * ow;                                                       // the second H of the double buffer
            aligned = aligned && off(lds.H) % 16 == 0 && off(h1) % 16 == 0;                            // phase_d_quad: float4 reads
            end = std::max(end, off(lds.H + 2 * (size_t)fh * ow));
            if (!headline) {
                float *acc = lds.H + 2 * (size_t)fh * ow;
                aligned = aligned && off(acc) % 16 == 0;                                               // accL: float4
                end = std::max(end, off(acc + (size_t)oh * ow));
            }
        }
        const size_t lds_bytes = memory_lds(c, P, headline);
        printf("P=%d end=%zu lds=%zu aligned=%d headline=%d\n", P, end, lds_bytes, (int)aligned, (int)headline);
        if (end > lds_bytes || !aligned) bad = 1;
    }
    return bad;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "carve")) return carve_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "k1plan")) return k1plan_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "k1tables")) return k1tables_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "plan")) return plan_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "per")) return per_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "raw")) return raw_main(argc, argv);
    if (argc < 6) return 2;
    agx_config c{};
    c.obs_h = atoi(argv[1]); c.obs_w = atoi(argv[2]); c.fov_h = atoi(argv[3]); c.fov_w = atoi(argv[4]);
    c.antialias = atoi(argv[5]);
    c.out_mode = AGX_OUT_RESIZE;
    const Flex3Host h = build_flex3(c);
    if (!h.ok) { printf("unsupported\n"); return 0; }
    const int oh = c.obs_h, ow = c.obs_w, fh = c.fov_h, fw = c.fov_w;
    const bool aa = c.antialias != 0;
    const int rstep = kThreads / ow, erows = (fh + rstep - 1) / rstep * rstep;
    std::mt19937 rng(7);
    double worst = 0;
    long cases = 0;
    std::vector<unsigned char> R0(h.r0_bytes);
    std::vector<float> D((size_t)h.r1_bytes / 4), E((size_t)std::max(h.r0_bytes, h.r1_bytes) / 4);
    for (int rh = 1; rh <= oh; ++rh)
        for (int rw = 1 + (rh * 7) % 3; rw <= ow; rw += 3) {
            const int r = (int)(rng() % (unsigned)(oh - rh + 1)), cc = (int)(rng() % (unsigned)(ow - rw + 1));
            for (auto &b : R0) b = (unsigned char)(rng() & 0xFF);          // frame + slack: arbitrary bytes
            for (auto &v : D) v = NAN;                                    // stale LDS may hold anything
            for (auto &v : E) v = NAN;
            const unsigned char *win = R0.data() + r * ow + cc;
            const bool squeeze = rh > fh;
            const int er = squeeze ? fh : rh;
            auto in_r0 = [&](const unsigned char *p) { return p >= R0.data() && p < R0.data() + h.r0_bytes; };
            if (squeeze) {
                const int Tw = h.wc_meta[rw].x, Th = h.hd_meta[rh].x;
                const int kmax = (std::max(rw, Tw) + 7) >> 3;
                if (8 * kmax > h.dp) { printf("D pitch too small rw=%d\n", rw); return 1; }
                for (int yf = 0; yf < fh; ++yf)
                    for (int x = 0; x < 8 * kmax; ++x) {
                        const int lo = h.hd_lo[(size_t)rh * fh + yf];
                        const float *w = &h.hd_w[h.hd_meta[rh].y + (size_t)yf * Th];
                        float acc = 0.f;
                        for (int q = 0; q < Th; ++q) {
                            const unsigned char *p = win + (lo + q) * ow + x;
                            if (!in_r0(p)) { printf("raw read outside R0 rh=%d rw=%d\n", rh, rw); return 1; }
                            acc = fmaf(w[q], (float)*p, acc);
                        }
                        D[(size_t)yf * h.dp + x] = acc;
                    }
                for (int y = 0; y < fh; ++y)
                    for (int x = 0; x < ow; ++x) {
                        const int lo = h.wc_lo[(size_t)rw * ow + x];
                        const float *w = &h.wc_w[h.wc_meta[rw].y + (size_t)x * Tw];
                        if (lo < 0 || lo + Tw > 8 * kmax) { printf("D read outside the written columns rw=%d x=%d\n", rw, x); return 1; }
                        float acc = 0.f;
                        for (int q = 0; q < Tw; ++q) acc = fmaf(w[q], D[(size_t)y * h.dp + lo + q], acc);
                        E[(size_t)y * ow + x] = acc;
                    }
            } else {
                const int kmax = (rh + rstep - 1) / rstep;
                if (kmax * rstep > erows) { printf("E rows\n"); return 1; }
                for (int y = 0; y < kmax * rstep; ++y)
                    for (int x = 0; x < ow; ++x) {
                        const Tap t = h.wf[(size_t)rw * ow + x];
                        const unsigned char *p0 = win + y * ow + t.lo, *p1 = win + y * ow + t.aux;
                        if (!in_r0(p0) || !in_r0(p1) || t.aux >= rw) { printf("window read rh=%d rw=%d\n", rh, rw); return 1; }
                        E[(size_t)y * ow + x] = fmaf(t.b, (float)*p1, t.a * (float)*p0);
                    }
            }
            // reference chain in double
            std::vector<double> crop((size_t)rh * rw);
            for (int y = 0; y < rh; ++y)
                for (int x = 0; x < rw; ++x) crop[(size_t)y * rw + x] = (double)win[y * ow + x] / 255.0;
            std::vector<double> ref = crop;
            if (squeeze) ref = resize(resize(ref, rh, rw, fh, fw, aa), fh, fw, rh, rw, aa);
            ref = resize(ref, rh, rw, oh, ow, aa);
            for (int y = 0; y < oh; ++y) {
                const int4 e = h.hy[(size_t)rh * oh + y];
                const int i0 = e.x & 0xFF, i1 = (e.x >> 8) & 0xFF, i2 = e.x >> 16;
                if (i0 >= er || i1 >= er || i2 >= er) { printf("row index rh=%d\n", rh); return 1; }
                float w0, w1, w2;
                memcpy(&w0, &e.y, 4); memcpy(&w1, &e.z, 4); memcpy(&w2, &e.w, 4);
                for (int x = 0; x < ow; ++x) {
                    float o = fmaf(w1, E[(size_t)i1 * ow + x], w0 * E[(size_t)i0 * ow + x]);
                    if (squeeze) o = fmaf(w2, E[(size_t)i2 * ow + x], o);
                    const double err = std::fabs((double)o - ref[(size_t)y * ow + x]);
                    if (!(err <= worst)) worst = err;      // NaN-propagating max
                }
            }
            ++cases;
        }
    printf("max_err %.3e cases %ld lds %zu\n", worst, cases, flex3_lds(h, c));
    return 0;
}
