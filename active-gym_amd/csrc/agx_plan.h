// agx_plan.h - HOST side: the one place a kernel form is chosen and an LDS byte count computed.  agx_create (agx_api.hip)
// computes the plans once per context and the launch functions switch on them; tests/host_tables_harness.cpp prints them from
// these very functions (`plan`, `k1plan`).  No HIP runtime call in here: the inputs are the config, the testing knobs and the host
// tables of agx_host_tables.h that agx_create builds anyway.
#pragma once
#include <algorithm>
#include <vector>

#include "agx_fixed_phases.h"
#include "agx_host_tables.h"

namespace agx {

constexpr size_t kMaxLds = 160 * 1024;   // gfx950: a workgroup may take the whole 160 KiB of its CU

// the five knobs of the shipped library: each selects a FALLBACK kernel (or launch sequence), read once per context in agx_create
struct Knobs {
    int generic = 0;         // AGX_FOVEA_GENERIC     K3 / K4 through the generic fallback kernel
    int flex_v2 = 0;         // AGX_FLEX_V2           K4 through k_fovea_flexible2 (pass-by-pass form)
    int per_v2 = 0;          // AGX_PER_V2            K3 through k_fovea_peripheral2
    int no_full = 0;         // AGX_INGEST_NO_FULL    general k_ingest<256> even where k_ingest_full12 applies
    int packed_unfused = 0;  // AGX_STEP_PACKED_UNFUSED  agx_step_flexible_packed as the three stand-alone launches
};

// ---- taps of one axis, as K3 / K4's pass-by-pass kernels read them
// compile-time tap bounds the tuned kernels are instantiated for (0 = run-time loops)
inline int tap_bucket(int n) { return n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : n <= 12 ? 12 : n <= 16 ? 16 : n; }

// One axis of torchvision Resize (rows::resize_axis, agx_rows.h) as {lo, n} entries and float weights, zero-padded to the
// kernels' compile-time bound `maxt`
inline void axis_taps(int n_in, int n_out, bool antialias, std::vector<int2> &ln, std::vector<float> &w, int &maxt) {
    const rows::Op op = rows::resize_axis(n_in, n_out, antialias);
    maxt = tap_bucket(rows::max_taps(op));
    ln.resize(n_out);
    w.assign((size_t)n_out * maxt, 0.f);
    for (int i = 0; i < n_out; ++i) {
        ln[i] = make_int2(op[i].lo, (int)op[i].w.size());
        for (size_t k = 0; k < op[i].w.size(); ++k) w[(size_t)i * maxt + k] = (float)op[i].w[k];
    }
}

// the four passes of K3 (squeeze W, squeeze H, expand W, expand H): n_in -> n_out of each
inline void per_axes(const agx_config &c, int nin[4], int nout[4]) {
    const int i[4] = {c.obs_w, c.obs_h, c.per_w, c.per_h}, o[4] = {c.per_w, c.per_h, c.obs_w, c.obs_h};
    std::copy(i, i + 4, nin);
    std::copy(o, o + 4, nout);
}

inline size_t per2_tables(const agx_config &c) {
    std::vector<int2> ln;
    std::vector<float> w;
    int m1 = 0, m3 = 0;
    axis_taps(c.obs_h, c.per_h, c.antialias != 0, ln, w, m1);
    axis_taps(c.per_h, c.obs_h, c.antialias != 0, ln, w, m3);
    return (size_t)c.per_h * (sizeof(int2) + m1 * sizeof(float)) + (size_t)c.obs_h * (sizeof(int2) + m3 * sizeof(float));
}

inline size_t per2_lds(const agx_config &c) {
    const size_t raw = ((size_t)c.obs_h * c.obs_w + 15) & ~(size_t)15;
    // A[oh][pw] and C[ph][ow] share one region (C is written after A's last read), then B[ph][pw]
    const size_t ac = (std::max((size_t)c.obs_h * c.per_w, (size_t)c.per_h * c.obs_w) + 3) & ~(size_t)3;
    const size_t b = ((size_t)c.per_h * c.per_w + 3) & ~(size_t)3;
    // + the pass-1 and pass-3 tap tables ({lo,n} + zero-padded weights; bounded by the bucketed tap counts)
    return 1024 + raw + (ac + b) * sizeof(float) + per2_tables(c);
}

// K4: one family = the taps of every window size r in [1, rmax] along one axis.
//   which = 0: r -> fov (squeeze)   1: fov -> r (expand back)   2: r -> obs (final resize)
struct HostFamily {
    std::vector<int2> ln;
    std::vector<float> w;
    std::vector<int4> meta;                       // [rmax + 1]
    std::vector<size_t> floats;                   // LDS floats of the staged table of size r
};
inline HostFamily build_family(int which, int rmax, int fov, int obs, bool antialias) {
    HostFamily f;
    f.meta.assign(rmax + 1, make_int4(0, 0, 1, 0));
    f.floats.assign(rmax + 1, 0);
    for (int r = 1; r <= rmax; ++r) {
        std::vector<int2> ln;
        std::vector<float> w;
        int maxt = 0;
        const int n_in = which == 0 ? r : (which == 1 ? fov : r);
        const int n_out = which == 0 ? fov : (which == 1 ? r : obs);
        axis_taps(n_in, n_out, antialias, ln, w, maxt);
        f.meta[r] = make_int4((int)f.ln.size(), (int)f.w.size(), maxt, n_out);
        f.floats[r] = (((size_t)2 * n_out + (size_t)n_out * maxt) + 3) & ~(size_t)3;
        f.ln.insert(f.ln.end(), ln.begin(), ln.end());
        f.w.insert(f.w.end(), w.begin(), w.end());
    }
    return f;
}
// the six families of a flexible context (wd, wb, wf, hd, hb, hf) and the worst-case LDS floats of their staged tables
inline size_t build_families(const agx_config &c, HostFamily fam[6]) {
    for (int k = 0; k < 6; ++k) {
        const bool is_w = k < 3;
        fam[k] = build_family(k % 3, is_w ? c.obs_w : c.obs_h, is_w ? c.fov_w : c.fov_h, is_w ? c.obs_w : c.obs_h, c.antialias != 0);
    }
    size_t worst_w = 0, worst_h = 0;
    for (int r = 1; r <= c.obs_w; ++r) worst_w = std::max(worst_w, fam[0].floats[r] + fam[1].floats[r] + fam[2].floats[r]);
    for (int r = 1; r <= c.obs_h; ++r) worst_h = std::max(worst_h, fam[3].floats[r] + fam[4].floats[r] + fam[5].floats[r]);
    return worst_w + worst_h;
}

inline size_t flex2_lds(const agx_config &c, size_t tab_floats) {
    const size_t raw = ((size_t)c.obs_h * c.obs_w + 15) & ~(size_t)15;
    const size_t ae = (std::max((size_t)c.obs_h * c.fov_w, (size_t)c.fov_h * c.obs_w) + 3) & ~(size_t)3;
    const size_t b = ((size_t)c.fov_h * c.fov_w + 3) & ~(size_t)3;
    const size_t cc = ((size_t)c.fov_h * c.obs_w + 3) & ~(size_t)3;      // C aliases the raw frame bytes
    return 1024 + std::max(raw, cc * sizeof(float)) + (ae + b + tab_floats) * sizeof(float);
}

// the compile-time geometries: the fixed fovea's kernels (K2, K5, K6) and K4's GeomS<84, 84, 30, 30>, K3's PGeomS<84, 84, 30, 30, 20, 20>
inline bool headline_fixed(const agx_config &c) { return c.obs_h == 84 && c.obs_w == 84 && c.fov_h == 30 && c.fov_w == 30; }
inline bool headline_peripheral(const agx_config &c) { return headline_fixed(c) && c.per_h == 20 && c.per_w == 20; }

inline size_t fixed_lds(const agx_config &c) {
    // window rows u8 [fh][ow] (16-B padded) | ytab[oh] | H[fh][ow]   (agx_fixed_phases.h: fixed_carve)
    size_t b = (size_t)fixed_pad(c.fov_h, c.obs_w);
    if (c.out_mode == AGX_OUT_RESIZE) b += (size_t)c.obs_h * sizeof(Tap) + (size_t)c.fov_h * c.obs_w * sizeof(float);
    return b;
}
#ifdef AGX_EXPERIMENTS
inline size_t fixed2_lds(const agx_config &c) {     // k_fovea_fixed2: lut[256] f32 | raw frame u8 (16-B padded) | ytab[oh] | H[fh][ow]
    const size_t raw = ((size_t)c.obs_h * c.obs_w + 15) & ~(size_t)15;
    return 1024 + raw + (size_t)c.obs_h * sizeof(Tap) + (size_t)c.fov_h * c.obs_w * sizeof(float);
}
#endif
// the LDS carve of k_history_memory (agx_k6_glimpse.h)
inline size_t memory_lds(const agx_config &c, int glimpses, bool headline) {
    size_t b = kMemTableBytes + (size_t)glimpses * fixed_pad(c.fov_h, c.obs_w);
    if (c.out_mode == AGX_OUT_RESIZE) {
        b += (size_t)c.obs_h * sizeof(Tap) + 2 * (size_t)c.fov_h * c.obs_w * sizeof(float);
        if (!headline) b += (size_t)c.obs_h * c.obs_w * sizeof(float);      // the running maximum of the run-time geometry form
    }
    return b;
}

// second LDS buffer of the generic kernels, in floats: flexible ping-pongs two full frames,
// peripheral keeps A[oh][pw] | B[ph][pw] | C[ph][ow] there
inline size_t generic_buf1(const agx_config &c) {
    const size_t cap = ((size_t)c.obs_h * c.obs_w + 3) & ~(size_t)3;
    if (c.kind != AGX_KIND_PERIPHERAL) return cap;
    const size_t abc = (size_t)c.obs_h * c.per_w + (size_t)c.per_h * c.per_w + (size_t)c.per_h * c.obs_w;
    return (abc + 3) & ~(size_t)3;
}

inline size_t generic_lds(const agx_config &c) {
    const size_t cap = ((size_t)c.obs_h * c.obs_w + 3) & ~(size_t)3;
    int tmax = std::max(std::max(c.obs_h, c.obs_w), std::max(c.fov_h, c.fov_w));
    if (c.kind == AGX_KIND_PERIPHERAL) tmax = std::max(tmax, std::max(c.per_h, c.per_w));
    return (cap + generic_buf1(c)) * sizeof(float) + (size_t)tmax * sizeof(Tap);
}

// The LDS of the kernel agx_create holds against kMaxLds ("geometry needs %zu B of LDS per workgroup").  Not always the kernel
// that runs: flexible is judged by the generic kernel even where flex3 / raw3 / flexible2 will run, peripheral by
// k_fovea_peripheral2 where that fits (and the knob does not force the fallback) and by the generic kernel otherwise, never by per3.
inline size_t create_lds(const agx_config &c, const Knobs &k) {
    if (c.kind == AGX_KIND_FIXED) return fixed_lds(c);
    const bool per_tuned = k.generic == 0 && per2_lds(c) <= kMaxLds && c.per_w <= kThreads;
    return c.kind == AGX_KIND_PERIPHERAL && per_tuned ? per2_lds(c) : generic_lds(c);
}

// whether a composed-operator table set applies: agx_create uploads it then, whatever the knobs say
inline bool flex3_fits(const Flex3Host &h, const agx_config &c) { return h.ok && flex3_lds(h, c) <= kMaxLds; }
inline bool flexraw_fits(const FlexRawHost &h, const agx_config &c) { return h.ok && h.lds(c) <= kMaxLds; }
inline bool per3_fits(const Per3Host &h) { return h.ok && h.lds <= kMaxLds; }

// ---- the plan of a context's fovea launches
enum Form { kFormNone, kFormFixed, kFormFlex3, kFormRaw3, kFormFlexible2, kFormPer3, kFormPeripheral2, kFormGeneric };
enum PackedForm { kPackedNone, kPackedRaw3, kPackedOffsetsFlexible2, kPackedOffsetsGeneric };

struct FovPlan {
    Form form = kFormNone;
    bool headline = false;             // compile-time geometry (GeomS / PGeomS) or run-time (GeomR / PGeomR)
    int mt = 0;                        // per3 / peripheral2: compile-time tap bound, 0 = run-time loops
    int same = 0;                      // peripheral: peripheral_res == obs_size, torchvision returns the input
    size_t lds = 0;                    // bytes of the launch
    PackedForm packed = kPackedNone;   // flexible, not resize_to_full: the crop launch of agx_fovea_flexible_packed
    const char *why = nullptr;         // why the composed plan (flex3 / raw3 / per3) does not run, nullptr where it does
};

// base context: no fovea launch; K5's full-frame form still picks its geometry argument by the same test
inline FovPlan plan_base(const agx_config &c) {
    FovPlan p;
    p.headline = headline_fixed(c);
    return p;
}

inline FovPlan plan_fixed(const agx_config &c) {
    FovPlan p;
    p.form = kFormFixed;
    p.headline = headline_fixed(c);
    p.lds = fixed_lds(c);
    return p;
}

// why a composed-operator plan (build_flex3 / build_flexraw) does not apply: their entry guards, everything behind the guards
// is a tap bound (a bucket overflows, or an up-scale row has more taps than the kernel's 2 or 3)
inline const char *composed_refusal(const agx_config &c, const Knobs &k, bool ok, size_t lds) {
    if (k.generic) return "generic";
    if (k.flex_v2) return "flex_v2";
    if (c.obs_w > kThreads) return "obs_w>256";
    if (c.fov_h > kThreads / 8) return "fov_h>32";
    if (c.obs_h > 1024) return "obs_h>1024";
    if (!ok) return "taps";
    if (lds > kMaxLds) return "lds";
    return nullptr;
}

// agx_fovea_flexible and the packed entry points.  f3 applies to resize_to_full only, fr to raw-crop / mask-out only (their
// builders refuse the other modes); tab_floats: build_families
inline FovPlan plan_flexible(const agx_config &c, const Knobs &k, const Flex3Host &f3, const FlexRawHost &fr, size_t tab_floats) {
    FovPlan p;
    p.headline = headline_fixed(c);
    const bool resize = c.out_mode == AGX_OUT_RESIZE;
    p.why = resize ? composed_refusal(c, k, f3.ok, f3.ok ? flex3_lds(f3, c) : 0) : composed_refusal(c, k, fr.ok, fr.ok ? fr.lds(c) : 0);
    if (!p.why) {
        p.form = resize ? kFormFlex3 : kFormRaw3;
        p.lds = resize ? flex3_lds(f3, c) : fr.lds(c);
        if (!resize) p.packed = kPackedRaw3;
        return p;
    }
    const size_t lds2 = flex2_lds(c, tab_floats);
    const bool v2 = k.generic == 0 && lds2 <= kMaxLds;
    p.form = v2 ? kFormFlexible2 : kFormGeneric;
    p.lds = v2 ? lds2 : generic_lds(c);
    if (!resize) p.packed = v2 ? kPackedOffsetsFlexible2 : kPackedOffsetsGeneric;
    return p;
}

// agx_fovea_peripheral; maxt: the four passes' bucketed tap bounds (axis_taps over per_axes)
inline FovPlan plan_peripheral(const agx_config &c, const Knobs &k, const Per3Host &h3, const int maxt[4]) {
    FovPlan p;
    p.same = (c.per_h == c.obs_h && c.per_w == c.obs_w) ? 1 : 0;
    p.why = k.generic ? "generic" : k.per_v2 ? "per_v2" : h3.ok ? (h3.lds > kMaxLds ? "lds" : nullptr)
            : c.obs_w > kThreads ? "obs_w>256" : c.per_w > kThreads ? "per_w>256" : c.per_h > 256 ? "per_h>256" : "taps";
    if (!p.why) {
        p.form = kFormPer3;
        p.mt = h3.mt;
        p.headline = headline_peripheral(c) && (h3.mt == 4 || h3.mt == 12);     // the two PGeomS instantiations
        p.lds = h3.lds;
    } else if (k.generic == 0 && per2_lds(c) <= kMaxLds && c.per_w <= kThreads) {
        // the tuned kernel keeps A | B | C with C 16-byte aligned and one row sweep per 256 threads.  Both squeeze tables are
        // padded to their own bucket; the kernel bound must not exceed either row pitch
        p.form = kFormPeripheral2;
        p.mt = maxt[0] == maxt[1] && maxt[0] <= 16 ? maxt[0] : 0;
        p.lds = per2_lds(c);
    } else {
        p.form = kFormGeneric;
        p.lds = generic_lds(c);
    }
    return p;
}

// ---- K1: the launch of one screen layout (rgb, gray, rgb-compact, gray-compact)
inline size_t ingest_lds(int band_rows, int ow) { return sizeof(int4) * band_rows + sizeof(int2) * ow + (size_t)2 * band_rows * 2 * kRawW; }
// + 8 bytes of slack: phase 2 reads the two ALIGNED dwords around every tap pair, and for the last pair of a row (x0 = 158 at
// 160 -> 84) the second dword lies past the row's 320 bytes - past the allocation for the very last row (its value is shifted
// out, but the read must stay inside the workgroup's LDS)
inline size_t band12_lds(int ow) { return sizeof(int2) * (kB12Rows + ow) + kB12GrayB + 8; }

enum K1Layout { kK1Rgb, kK1Gray, kK1RgbCompact, kK1GrayCompact };   // "rgb", "gray", "rgb-compact", "gray-compact"
struct K1Launch {
    bool band12 = false;     // the band12 form (k_ingest_full12 and its gray / compact / flexscan forms) or the general band kernel
    int band_rows = 0, nbands = 0;
    size_t lds = 0;
};
// band_rows: the band height in force for the layout (compact screens: always the plan's)
inline K1Launch plan_k1(const K1Plan &q, int layout, int band_rows, int oh, int ow, const Knobs &k) {
    K1Launch l;
    l.band12 = k.no_full == 0 && k1_band12(q, layout >= kK1RgbCompact, band_rows);
    l.band_rows = band_rows;
    l.nbands = (oh + band_rows - 1) / band_rows;
    l.lds = l.band12 ? band12_lds(ow) : ingest_lds(band_rows, ow);
    return l;
}

}  // namespace agx
