// experiments/agx_retrace_tiled.h - the batch-major form of K16 (agx_k16_retrace.h) through LDS: built, measured SLOWER than the
// strided form that ships (48.1 against 42.1 us at B = 1024, L = 128, 25.1 against 22.1 us at B = 64, L = 64, through the Python
// binding: DESIGN.md section 29, profiles/retrace_bench.json), kept in the experiments build only (AGX_RETRACE_TILED=1 there).
//
// Tiles of 64 sequences x kRetraceTile steps.  A tile is loaded along l, so a wave reads contiguous runs of kRetraceTile * 4 B
// per row (at 16 steps half a line: a line is fetched once and completed by the next tile from the cache), into registers, and
// goes to LDS at a row pitch of kRetraceTile + 1 dwords: the column reads of the fold - lane b reads dword b * pitch + j - fall
// on bank (b * pitch + j) mod 32, and an odd pitch makes those distinct in either half of the wave.  The fold writes target, td
// and valid over the tile's reward, q and steps planes, and the tile is stored along l again.  The registers are the second
// buffer: the loads of the tile below are issued before the current tile is folded.  Every device write is an ordinary vector
// store.
#pragma once
#include "../agx_k16_retrace.h"

namespace agx {

#ifndef AGX_RETRACE_TILE
#define AGX_RETRACE_TILE 16          // steps per LDS tile, 16 or 32.  16: 64 B per row and load, 96 staging registers, 168 VGPRs, no
                                     // spill.  32 reads a whole 128-B line per row but stages 192 registers: 304 VGPRs, 60 spilled
                                     // SGPRs (the store masks of its 32 rows per lane) - not taken.  64 would need 97.5 KiB of LDS.
#endif

constexpr int kRetraceTile = AGX_RETRACE_TILE;
constexpr int kRetracePitch = kRetraceTile + 1;                  // dwords per LDS row
constexpr int kRetraceRowsPer = kRetraceThreads / kRetraceTile;  // rows one load instruction of the wave covers
static_assert(kRetraceTile == 16 || kRetraceTile == 32, "a tile row divides the wave, and six planes of it fit static LDS (64 KiB)");

// The part of one tile a lane moves: kRetraceTile elements per plane, element k at row k * kRetraceRowsPer + lane / kRetraceTile,
// column lane % kRetraceTile.  (Every index is a constant once unrolled: the arrays live in registers.)
struct RetraceTileRegs {
    float r[kRetraceTile], d[kRetraceTile], q[kRetraceTile], v[kRetraceTile], c[kRetraceTile];
    int32_t s[kRetraceTile];
};

// The planes of one tile in LDS; target, td and valid are written over reward, q and steps.
struct RetraceTile {
    float r[kRetraceThreads * kRetracePitch], d[kRetraceThreads * kRetracePitch], q[kRetraceThreads * kRetracePitch],
        v[kRetraceThreads * kRetracePitch], c[kRetraceThreads * kRetracePitch];
    int32_t s[kRetraceThreads * kRetracePitch];
};

// the tile of steps l0 .. l0 + kRetraceTile - 1 of sequences b0 .. b0 + 63.  No load is conditional: an element past B or L is
// read from the nearest one inside - the last sequence, the last step - and its steps reads as 0, no row, so that nothing of
// what was loaded for it reaches an output.
__device__ __forceinline__ void retrace_tile_load(RetraceTileRegs &g, const RetraceParams &p, int b0, int l0, int row0, int col) {
    const bool in_l = l0 + col < p.L;
    const uint32_t l = (uint32_t)min(l0 + col, p.L - 1);
#pragma unroll
    for (int k = 0; k < kRetraceTile; ++k) {
        const int bb = b0 + row0 + k * kRetraceRowsPer;
        const uint32_t a = (uint32_t)min(bb, p.B - 1) * (uint32_t)p.L + l;
        const int32_t s = p.steps[a];
        g.s[k] = (in_l && bb < p.B) ? s : 0;
        g.r[k] = p.reward[a];
        g.d[k] = p.discount[a];
        g.q[k] = p.q[a];
        g.v[k] = p.v[a];
        g.c[k] = p.c[a];
    }
}

__global__ __launch_bounds__(kRetraceThreads) void k_retrace_tiled(RetraceParams p) {
    __shared__ RetraceTile t;
    const int lane = threadIdx.x;
    const int b0 = blockIdx.x * kRetraceThreads, b = b0 + lane;
    const int row0 = lane / kRetraceTile, col = lane % kRetraceTile;
    const int len = b < p.B ? retrace_len(p.len[b], p.L) : 0;
    const float boot = (p.boot && b < p.B) ? p.boot[b] : 0.0f;
    float carry = 0.0f, vabove = 0.0f;
    int l0 = ((p.L - 1) / kRetraceTile) * kRetraceTile;              // tiles start at multiples of the tile: the top one may be short
    RetraceTileRegs g;
    retrace_tile_load(g, p, b0, l0, row0, col);
    for (;;) {
#pragma unroll
        for (int k = 0; k < kRetraceTile; ++k) {
            const int at = (row0 + k * kRetraceRowsPer) * kRetracePitch + col;
            t.s[at] = g.s[k];
            t.r[at] = g.r[k];
            t.d[at] = g.d[k];
            t.q[at] = g.q[k];
            t.v[at] = g.v[k];
            t.c[at] = g.c[k];
        }
        __syncthreads();
        if (l0 > 0) retrace_tile_load(g, p, b0, l0 - kRetraceTile, row0, col);     // in flight while this tile folds
        const int top = min(kRetraceTile, p.L - l0);                 // (uniform)
#pragma unroll
        for (int j = kRetraceTile - 1; j >= 0; --j) {
            if (j < top) {
                const int at = lane * kRetracePitch + j, l = l0 + j;
                const float vnext = l + 1 < len ? vabove : boot;
                const RetraceOut o = retrace_step(carry, retrace_has(l, len, t.s[at]), t.r[at], t.d[at], vnext, t.q[at], t.c[at]);
                vabove = t.v[at];
                t.r[at] = o.target;
                t.q[at] = o.td;
                t.s[at] = (int32_t)o.valid;
            }
        }
        __syncthreads();
        const bool in_l = l0 + col < p.L;
#pragma unroll
        for (int k = 0; k < kRetraceTile; ++k) {
            const int row = row0 + k * kRetraceRowsPer, bb = b0 + row;
            if (in_l && bb < p.B) {
                const int at = row * kRetracePitch + col;
                const uint32_t a = (uint32_t)bb * (uint32_t)p.L + (uint32_t)(l0 + col);
                p.target[a] = t.r[at];
                if (p.td) p.td[a] = t.q[at];
                if (p.valid) p.valid[a] = (uint8_t)t.s[at];
            }
        }
        if (l0 == 0) break;
        __syncthreads();                                             // the tile is read out before the next one is written
        l0 -= kRetraceTile;
    }
}

}  // namespace agx
