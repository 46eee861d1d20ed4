// CPU harness for the host-built operator tables of k_fovea_flexible3 (active-gym_amd/csrc/agx_host_tables.h).
// Replays the kernel's arithmetic (same tables, same float32 operation order, same index rules) on the host and
// compares it with the reference chain  crop -> [Resize(fov) -> Resize(res) iff rh > fov_h] -> Resize(obs)
// (fov_env.py:276-298) evaluated pass by pass in double with the plain per-axis operators.  Also checks the memory
// rules the kernel relies on (every LDS index inside the regions agx_create sizes).
// Build: hipcc -std=c++17 -I include -I active-gym_amd/csrc tests/host_tables_harness.cpp -o <out>   (host code only)
// Usage: harness oh ow fh fw antialias          (k_fovea_flexible3 tables) -> "max_err <e> cases <n>" | "unsupported"
//        harness per oh ow ph pw antialias      (k_fovea_peripheral3 tables + unit_fast over all 256 values)
//        harness raw oh ow fh fw antialias      (k_fovea_flexible_raw3 tables: raw-crop / mask-out / packed forms)
//        harness plan oh ow fh fw ph pw antialias resize|raw|mask
//                                               which kernel form agx_create + the launch code select for each kind, and why
//        harness k1plan obs                     which K1 ingest form each screen layout selects at obs x obs, and what it branches on
//        harness k1tables obs                   the K1 tables of build_k1: x0 x1 a0 a1 y0 y1 b0 b1 and the source-row list
#include <cstdio>
#include <cstdlib>
#include <random>

#include "agx_host_tables.h"

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
// The table builders are the ones agx_create calls (agx_host_tables.h).  The predicates that live only in agx_api.hip are
// restated here, each under the name it has there; a change to one of them there must be made here too, and the case table
// of tests/test_geometry_plan_cpu.py is what notices a plan that moved.
namespace plan {

constexpr size_t kMaxLds = 160 * 1024;                     // agx_api.hip: kMaxLds

int tap_bucket(int n) { return n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : n <= 12 ? 12 : n <= 16 ? 16 : n; }   // agx_api.hip: tap_bucket

// agx_api.hip: axis_taps - the bucketed tap bound `maxt` only (the same index arithmetic, the weights left out)
int axis_maxt(int n_in, int n_out, bool antialias) {
    const double scale = (double)n_in / (double)n_out;
    const bool aa = antialias && n_in > n_out;
    int maxt = 1;
    for (int i = 0; i < n_out; ++i) {
        int n;
        if (aa) {
            const double support = scale, center = scale * (i + 0.5);
            long long xmin = (long long)(center - support + 0.5);
            if (xmin < 0) xmin = 0;
            long long xmax = (long long)(center + support + 0.5);
            if (xmax > n_in) xmax = n_in;
            n = xmax > xmin ? (int)(xmax - xmin) : 0;
        } else {
            double f = scale * (i + 0.5) - 0.5;
            if (f < 0.0) f = 0.0;
            int i0 = (int)f;
            if (i0 > n_in - 1) i0 = n_in - 1;
            n = i0 < n_in - 1 ? 2 : 1;
        }
        maxt = std::max(maxt, n);
    }
    return tap_bucket(maxt);
}

size_t per2_tables(const agx_config &c) {                  // agx_api.hip: per2_tables
    const int m1 = axis_maxt(c.obs_h, c.per_h, c.antialias != 0), m3 = axis_maxt(c.per_h, c.obs_h, c.antialias != 0);
    return (size_t)c.per_h * (sizeof(int2) + m1 * sizeof(float)) + (size_t)c.obs_h * (sizeof(int2) + m3 * sizeof(float));
}

size_t per2_lds(const agx_config &c) {                     // agx_api.hip: per2_lds
    const size_t raw = ((size_t)c.obs_h * c.obs_w + 15) & ~(size_t)15;
    const size_t ac = (std::max((size_t)c.obs_h * c.per_w, (size_t)c.per_h * c.obs_w) + 3) & ~(size_t)3;
    const size_t b = ((size_t)c.per_h * c.per_w + 3) & ~(size_t)3;
    return 1024 + raw + (ac + b) * sizeof(float) + per2_tables(c);
}

// agx_api.hip: build_family(...).floats[r] - LDS floats of the staged table of window size r
size_t family_floats(int which, int r, int fov, int obs, bool antialias) {
    const int n_in = which == 0 ? r : (which == 1 ? fov : r);
    const int n_out = which == 0 ? fov : (which == 1 ? r : obs);
    const int maxt = axis_maxt(n_in, n_out, antialias);
    return (((size_t)2 * n_out + (size_t)n_out * maxt) + 3) & ~(size_t)3;
}

size_t flex_tab_floats(const agx_config &c) {              // agx_api.hip: agx_create, ctx->flex_tab_floats
    const bool aa = c.antialias != 0;
    size_t worst_w = 0, worst_h = 0;
    for (int r = 1; r <= c.obs_w; ++r) {
        size_t s = 0;
        for (int k = 0; k < 3; ++k) s += family_floats(k, r, c.fov_w, c.obs_w, aa);
        worst_w = std::max(worst_w, s);
    }
    for (int r = 1; r <= c.obs_h; ++r) {
        size_t s = 0;
        for (int k = 0; k < 3; ++k) s += family_floats(k, r, c.fov_h, c.obs_h, aa);
        worst_h = std::max(worst_h, s);
    }
    return worst_w + worst_h;
}

size_t flex2_lds(const agx_config &c, size_t tab_floats) { // agx_api.hip: flex2_lds
    const size_t raw = ((size_t)c.obs_h * c.obs_w + 15) & ~(size_t)15;
    const size_t ae = (std::max((size_t)c.obs_h * c.fov_w, (size_t)c.fov_h * c.obs_w) + 3) & ~(size_t)3;
    const size_t b = ((size_t)c.fov_h * c.fov_w + 3) & ~(size_t)3;
    const size_t cc = ((size_t)c.fov_h * c.obs_w + 3) & ~(size_t)3;
    return 1024 + std::max(raw, cc * sizeof(float)) + (ae + b + tab_floats) * sizeof(float);
}

size_t fixed_lds(const agx_config &c) {                    // agx_api.hip: fixed_lds
    const size_t raw = ((size_t)c.fov_h * c.obs_w + 15) & ~(size_t)15;
    size_t b = raw;
    if (c.out_mode == AGX_OUT_RESIZE) b += (size_t)c.obs_h * sizeof(Tap) + (size_t)c.fov_h * c.obs_w * sizeof(float);
    return b;
}

size_t generic_buf1(const agx_config &c) {                 // agx_api.hip: generic_buf1
    const size_t cap = ((size_t)c.obs_h * c.obs_w + 3) & ~(size_t)3;
    if (c.kind != AGX_KIND_PERIPHERAL) return cap;
    const size_t abc = (size_t)c.obs_h * c.per_w + (size_t)c.per_h * c.per_w + (size_t)c.per_h * c.obs_w;
    return (abc + 3) & ~(size_t)3;
}

size_t generic_lds(const agx_config &c) {                  // agx_api.hip: generic_lds
    const size_t cap = ((size_t)c.obs_h * c.obs_w + 3) & ~(size_t)3;
    int tmax = std::max(std::max(c.obs_h, c.obs_w), std::max(c.fov_h, c.fov_w));
    if (c.kind == AGX_KIND_PERIPHERAL) tmax = std::max(tmax, std::max(c.per_h, c.per_w));
    return (cap + generic_buf1(c)) * sizeof(float) + (size_t)tmax * sizeof(Tap);
}

// agx_api.hip: agx_create, "the LDS of the kernel that will actually run" (no knob set).  0 = accepted, else the bytes in
// the message "geometry needs %zu B of LDS per workgroup (limit %zu)"
size_t create_refusal(const agx_config &c) {
    const bool per_tuned = per2_lds(c) <= kMaxLds && c.per_w <= kThreads;
    const size_t lds = c.kind == AGX_KIND_FIXED ? fixed_lds(c)
                       : (c.kind == AGX_KIND_PERIPHERAL && per_tuned ? per2_lds(c) : generic_lds(c));
    return lds > kMaxLds ? lds : 0;
}

void print_set(const char *key, const std::vector<int2> &meta, int from, int to) {
    bool has[17] = {};
    for (int r = from; r <= to; ++r) has[meta[r].x] = true;
    printf(" %s=", key);
    bool any = false;
    for (int t : {4, 8, 16})
        if (has[t]) { printf("%s%d", any ? "," : "", t); any = true; }
    if (!any) printf("-");
}

// why a composed-operator plan (build_flex3 / build_flexraw) does not apply: their entry guards restated, everything
// behind the guards is a tap bound (a bucket overflows, or an up-scale row has more taps than the kernel's 2 or 3)
const char *composed_refusal(const agx_config &c, bool ok, size_t lds) {
    if (c.obs_w > kThreads) return "obs_w>256";
    if (c.fov_h > kThreads / 8) return "fov_h>32";
    if (c.obs_h > 1024) return "obs_h>1024";
    if (!ok) return "taps";
    if (lds > kMaxLds) return "lds";
    return nullptr;
}

// agx_fovea_flexible / agx_fovea_flexible_packed behind a refused composed plan
const char *flex_fallback(const agx_config &c, size_t *lds) {
    const size_t lds2 = flex2_lds(c, flex_tab_floats(c));
    if (lds2 <= kMaxLds) { *lds = lds2; return "flexible2"; }
    *lds = generic_lds(c);
    return "generic";
}

int run(int argc, char **argv) {
    if (argc < 10) return 2;
    agx_config c{};
    c.obs_h = atoi(argv[2]); c.obs_w = atoi(argv[3]); c.fov_h = atoi(argv[4]); c.fov_w = atoi(argv[5]);
    c.per_h = atoi(argv[6]); c.per_w = atoi(argv[7]); c.antialias = atoi(argv[8]);
    const char *mode = argv[9];
    const int out_mode = !strcmp(mode, "resize") ? AGX_OUT_RESIZE : !strcmp(mode, "mask") ? AGX_OUT_MASK : !strcmp(mode, "raw") ? AGX_OUT_RAW : -1;
    if (out_mode < 0) return 2;
    const bool headline = c.obs_h == 84 && c.obs_w == 84 && c.fov_h == 30 && c.fov_w == 30;
    size_t refused;
    // ---- fixed (agx_fovea_fixed)
    c.kind = AGX_KIND_FIXED;
    c.out_mode = out_mode;
    if ((refused = create_refusal(c))) printf("fixed form=refused lds=%zu\n", refused);
    else printf("fixed form=%s lds=%zu\n", headline ? "fixed<GeomS>" : "fixed<GeomR>", fixed_lds(c));
    // ---- flexible (agx_fovea_flexible, agx_fovea_flexible_packed)
    c.kind = AGX_KIND_FLEXIBLE;
    if ((refused = create_refusal(c))) printf("flexible form=refused lds=%zu\n", refused);
    else if (out_mode == AGX_OUT_RESIZE) {
        const Flex3Host h = build_flex3(c);
        const size_t lds3 = h.ok ? flex3_lds(h, c) : 0;
        const char *why = composed_refusal(c, h.ok, lds3);
        if (!why) {
            printf("flexible form=flex3");
            print_set("W", h.wc_meta, 1, c.obs_w);
            print_set("H", h.hd_meta, c.fov_h + 1, c.obs_h);
            printf(" rstep=%d lds=%zu\n", kThreads / c.obs_w, lds3);
        } else {
            size_t lds = 0;
            const char *form = flex_fallback(c, &lds);
            printf("flexible form=%s why=%s lds=%zu\n", form, why, lds);
        }
    } else {
        const FlexRawHost h = build_flexraw(c);
        const size_t ldsr = h.ok ? h.lds(c) : 0;
        const char *why = composed_refusal(c, h.ok, ldsr);
        if (!why) {
            printf("flexible form=raw3");
            print_set("W", h.wb_meta, 1, c.obs_w);
            print_set("H", h.hd_meta, c.fov_h + 1, c.obs_h);
            printf(" rstep=%d lds=%zu packed=raw3\n", kThreads / c.obs_w, ldsr);
        } else {
            size_t lds = 0;
            const char *form = flex_fallback(c, &lds);
            printf("flexible form=%s why=%s lds=%zu packed=offsets+%s\n", form, why, lds, form);
        }
    }
    // ---- peripheral (agx_fovea_peripheral): always resize_to_full (pipeline.py, fov_env.py:361-364)
    c.kind = AGX_KIND_PERIPHERAL;
    c.out_mode = AGX_OUT_RESIZE;
    if (c.per_h < 1 || c.per_w < 1) printf("peripheral form=none\n");
    else if ((refused = create_refusal(c))) printf("peripheral form=refused lds=%zu\n", refused);
    else {
        const Per3Host h = build_per3(c);
        const int same = (c.per_h == c.obs_h && c.per_w == c.obs_w) ? 1 : 0;
        if (h.ok && h.lds <= kMaxLds) printf("peripheral form=per3 mt=%d same=%d lds=%zu\n", h.mt, same, h.lds);
        else {
            const char *why = h.ok ? "lds" : (c.obs_w > kThreads ? "obs_w>256" : c.per_w > kThreads ? "per_w>256" : c.per_h > 256 ? "per_h>256" : "taps");
            if (per2_lds(c) <= kMaxLds && c.per_w <= kThreads) {
                const bool aa = c.antialias != 0;
                const int m0 = axis_maxt(c.obs_w, c.per_w, aa), m1 = axis_maxt(c.obs_h, c.per_h, aa);
                printf("peripheral form=peripheral2 mt=%d same=%d why=%s lds=%zu\n", m0 == m1 && m0 <= 16 ? m0 : 0, same, why, per2_lds(c));
            } else
                printf("peripheral form=generic same=%d why=%s lds=%zu\n", same, why, generic_lds(c));
        }
    }
    return 0;
}

}  // namespace plan

// ---- K1 ingest: the plan build_k1 (agx_host_tables.h) hands agx_create, per screen layout, as the launch code of
// agx_api.hip reads it with no knob set (agx_ingest, agx_ingest_gray_raw, ingest_compact: k1_band12 at plan.band_rows).
//   form=band12 br=12 bands=B
//   form=general br=R bands=B partial=P affine=A xclamp=X yclamp=Y
// partial: the last band has fewer rows than br; affine: source rows from the integer form (whole screens only - compact
// screens always read the packed row table); xclamp / yclamp: some tap pair is one source column / row twice.
static int k1plan_main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int o = atoi(argv[2]);
    if (o < 4 || o > 1024 || (o & 3)) return 2;             // not a size agx_create accepts (k1tables: the same)
    const K1Host h = build_k1(o, o);
    const K1Plan &q = h.plan;
    bool xclamp = false, yclamp = false;
    for (int i = 0; i < o; ++i) {
        xclamp = xclamp || h.x0[i] == h.x1[i];
        yclamp = yclamp || h.y0[i] == h.y1[i];
    }
    const int br = q.band_rows, bands = (o + br - 1) / br;
    const char *names[4] = {"rgb", "gray", "rgb-compact", "gray-compact"};
    for (int k = 0; k < 4; ++k) {
        const bool compact = k >= 2;
        if (k1_band12(q, compact, br)) printf("%s form=band12 br=%d bands=%d\n", names[k], br, bands);
        else
            printf("%s form=general br=%d bands=%d partial=%d affine=%d xclamp=%d yclamp=%d\n", names[k], br, bands, o % br != 0,
                   !compact && q.y_affine, xclamp, yclamp);
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

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "k1plan")) return k1plan_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "k1tables")) return k1tables_main(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "plan")) return plan::run(argc, argv);
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
