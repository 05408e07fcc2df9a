// qd_geometry.h — what a chain kernel's geometry is allowed to be, and how its LDS is laid out: plain-integer constexpr rules, stated once.
//
// The kernels (qd_chain.h: FixedGeo<>, Pipe3S<>, Spark2<>, the *_ok templates) take their compile-time constants from these
// functions; the host (quadrs_hip.hip: geometry_recipe, lds_for, the launch path) calls the same functions at run time before it
// asks for a build.  Nothing here is HIP-specific: the header compiles as plain C++17 on the host, under hipcc and under hiprtc.
// Sizes are computed in 64 bits so that the host can reject an oversized shape before anything wraps; the kernel side narrows.
#pragma once

#if !defined(__HIPCC_RTC__)
#include <stdint.h>
#else      // hiprtc has no <stdint.h> (qd_device.h adds uintptr_t and size_t to these)
typedef unsigned char uint8_t; typedef signed char int8_t; typedef unsigned short uint16_t; typedef short int16_t;
typedef unsigned int uint32_t; typedef int int32_t; typedef unsigned long long uint64_t; typedef long long int64_t;
#endif

namespace qd {

// ---------------------------------------------------------------- FixedGeo FLAGS_ bits (qd_plan_info.kernel_flags, tile_hint[6] >> 8)
// Bits 0, 1, 4 and 9-12 selected experiments that lost and were removed; they stay reserved, so every other
// bit keeps its number, and plan creation refuses a tile hint that carries one (kHintGeoBits).
constexpr uint32_t kGeoNoSplit = 4;             // bit 2: no component-split FIR; on a 16-byte-row tile the packed lane-per-output FIR (fir_pair)
constexpr uint32_t kGeoFastP1 = 8;              // bit 3: row-aligned phase 1 (tiles start on row boundaries, a compile-time number of rows)
constexpr uint32_t kGeoUnrolledFir = 32;        // bit 5: the shared FIR of overlapping windows as straight-line code
constexpr uint32_t kGeoDeferFft = 64;           // bit 6: the previous tile's FFT + epilogue on a wave the FIR leaves idle (two FFT slots)
constexpr uint32_t kGeoPackedTile = 128;        // bit 7: two outputs per lane as straight-line packed code (fir_tiled2_pk)
constexpr uint32_t kGeoNtLoads = 256;           // bit 8: phase-1 stream loads non-temporal
constexpr uint32_t kGeoHalfTile = 8192;         // bit 13: the tile buffer holds HALF a window's FIR input, two passes per window
constexpr uint32_t kGeoFastFma = 16384;         // bit 14: QD_MODE_FAST — the packed FIRs fuse multiply and add, one rounding per tap
constexpr uint32_t kGeoPipe3 = 32768;           // bit 15: the three-stage kernel for overlapping windows (k_chain_pipe3)
constexpr uint32_t kGeoNtInner = 65536;         // bit 16 (with bit 8): rows a neighbouring tile reads too keep the default cache policy
constexpr uint32_t kGeoStream = 131072;         // bit 17 (with bit 15): its streaming form (k_chain_pipe3s)
constexpr uint32_t kGeoWriteSink = 262144;      // bit 18: the streaming kernel as the `write` sink: producers + FIR waves only
constexpr uint32_t kGeoSpark = 524288;          // bit 19: the wave-local kernels of chains without a lowpass (k_spark)
constexpr uint32_t kGeoSparkReg = 1048576;      // bit 20: ... with the first FFT pass out of registers (k_spark2)
constexpr uint32_t kGeoSparkDirect = 2097152;   // bit 21: ... a window of 2 ... 8 points per lane, no LDS (k_spark0)
constexpr uint32_t kGeoWindow = 1u << 22;       // bit 22: applies the plan's window (ChainParams::window) where phase 2 stores into the FFT buffer; k_chain only

// the variant bits a tile hint may carry: the ones above below bit 19 (the wave-local kernels are not hinted)
constexpr uint32_t kHintGeoBits = kGeoNoSplit | kGeoFastP1 | kGeoUnrolledFir | kGeoDeferFft | kGeoPackedTile | kGeoNtLoads | kGeoHalfTile | kGeoFastFma |
                                  kGeoPipe3 | kGeoNtInner | kGeoStream | kGeoWriteSink;

// cache policy (buffer-load aux operand) of the phase-1 stream loads: nt
constexpr int ct_load_aux(uint32_t flags) { return (flags & kGeoNtLoads) ? 2 : 0; }

// ---------------------------------------------------------------- which kernel a flags word means
constexpr int kThreads = 256;
constexpr int kPipe3Threads = 1024, kPipe3Prod = 512;
constexpr uint32_t kSparkRow = 512;          // samples per NCO row of the wave-local kernels, every format
constexpr uint32_t kSparkMaxW = 1024;
constexpr uint32_t kLaneEntryBytes = 24;     // one entry of an NCO lane table (qd_nco.h LaneEntry: c, sum, dif)

enum Family { kFamChain, kFamPipe3, kFamPipe3s, kFamSpark, kFamSpark2, kFamSpark0 };

constexpr Family family_of(uint32_t flags) {
    return (flags & kGeoSpark) ? ((flags & kGeoSparkDirect) ? kFamSpark0 : (flags & kGeoSparkReg) ? kFamSpark2 : kFamSpark)
         : (flags & kGeoPipe3) ? ((flags & kGeoStream) ? kFamPipe3s : kFamPipe3) : kFamChain;
}

struct FamilyRow {
    const char *name;
    bool on_rows;       // its tiles always start on row boundaries (k_chain: only with kGeoFastP1)
};
constexpr FamilyRow kFamilies[] = {
    {"qd::k_chain", false}, {"qd::k_chain_pipe3", true}, {"qd::k_chain_pipe3s", true},
    {"qd::k_spark", true},  {"qd::k_spark2", true},      {"qd::k_spark0", true},
};
constexpr const char *family_name(uint32_t flags) { return kFamilies[family_of(flags)].name; }
// row-aligned kernels: a launch whose first window is off the row grid goes to the per-sample kernel
constexpr bool row_aligned(uint32_t flags) { return kFamilies[family_of(flags)].on_rows || (flags & kGeoFastP1) != 0; }
// workgroup size: nt row-loading threads plus the consumer waves of the three-stage kernels; the wave-local kernels
// run four waves per workgroup whatever their row geometry (their nt = 512 / SPL only lays out the NCO tables)
constexpr int family_threads(int nt, uint32_t flags) {
    switch (family_of(flags)) {
    case kFamPipe3: return nt + 512;
    case kFamPipe3s: return nt + ((flags & kGeoWriteSink) ? 256 : 512);
    case kFamChain: return nt;
    default: return kThreads;
    }
}

// ---------------------------------------------------------------- small helpers
constexpr uint32_t ct_log2(uint64_t v) { uint32_t l = 0; while ((1ull << l) < v) ++l; return l; }
constexpr bool ct_pow2(uint64_t v) { return v && !(v & (v - 1)); }
constexpr uint64_t ct_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
constexpr uint64_t ct_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
constexpr uint64_t ct_gcd(uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; }
constexpr uint64_t ct_rows(uint64_t samples, uint64_t row) { return (samples + row - 1) / row; }
constexpr uint64_t ct_taps_bytes(uint64_t T) { return ((T + 3) & ~3ull) * 4; }          // taps in LDS: T floats, padded to a multiple of 4

// LDS float2 elements of an interleaved raw tile of tile_raw samples: one pad group per row of D samples (even D), never less than
// the G*W f32 norms the bucket epilogue parks there, even (the FFT buffers behind it stay 16-byte aligned)
constexpr uint64_t ct_tile_elems(uint64_t tile_raw, uint64_t D, uint64_t GW, uint64_t pad_per_row) {
    const uint64_t pad = (D % 2 == 0) ? pad_per_row * (tile_raw / D + 1) : 0;
    return (ct_max(tile_raw + pad + 1, GW / 2 + 1) + 1) & ~1ull;
}
constexpr uint64_t ct_tile_raw(uint64_t W, uint64_t S, uint64_t D, uint64_t T, uint64_t G) { return (G - 1) * S * D + W * D + T; }
constexpr uint64_t ct_raw_elems(uint64_t W, uint64_t S, uint64_t D, uint64_t T, uint64_t G, uint64_t pad_per_row = 1) {
    return ct_tile_elems(ct_tile_raw(W, S, D, T, G), D, G * W, pad_per_row);
}

// ---------------------------------------------------------------- FixedGeo<W, S, D, T, G, FIRB, FIRR, PAD, BATCH, FLAGS>
// (what each constant means is said where the kernels use it: FixedGeo in qd_chain.h)
struct FixedRules {
    uint64_t W, S, D, T, G;
    uint32_t flags, kBatch, kFirBlock;
    bool kFirTile4;
    uint32_t kFirTile, pshift, logW, kPad, dshift, dmagic, log_base, base_len, layers;
    uint64_t PD, Dp, c, a0, b0, T_fast, a1, b1;
    bool kHalfTile;
    uint64_t kHalfOut, kHalfRaw, tile_raw, pass_raw, kNtrunc, Q;
    bool kShared, kPairFir, kUnrolledShared, kPackedTile;
    uint64_t lds_raw_elems;        // float2 elements of the raw tile as the kernel lays it out
    uint64_t lds_raw_alloc;        // ... as the host sizes it: rows padded as ASKED (PAD)
    // component-split FIR (fir_comp): mid-length filters whose tile leaves at least half the lanes without an output
    constexpr bool split_ok(uint64_t nt) const {
        return !(flags & kGeoNoSplit) && !kShared && kFirTile == 1 && kPad != 2 && D % 8 == 0 && T >= 64 && 2 * G * W <= nt;
    }
    // register-tiled kernels: spare waves take the truncated tails (fir_prefix) when main lanes fill whole waves
    constexpr bool helper_ok(uint64_t nt) const {
        return kFirTile > 1 && !kShared && (G * W / kFirTile) % 64 == 0 && G * W / kFirTile + G * kNtrunc <= nt &&
               (T / 2) % 8 == 0 && kNtrunc > 0 && kNtrunc < W;
    }
    constexpr bool split_ok_shared(uint64_t nt) const {      // same, shared-FIR mode: (G-1)*S + W outputs per tile
        return kShared && kFirTile == 1 && kPad != 2 && D % 8 == 0 && T >= 64 && 2 * Q <= nt;
    }
    // lanes the FIR occupies (two outputs per lane: half as many)
    constexpr uint64_t fir_lanes() const { return (kHalfTile ? kHalfOut : G * W) / (kPackedTile ? 2 : 1); }
    // deferred FFT: the packed FIRs leave at least one wave idle
    constexpr bool defer_fft_ok(bool has_fir, uint64_t nt) const {
        return has_fir && (kPairFir || kPackedTile) && (flags & kGeoDeferFft) != 0 && kBatch == 2 && fir_lanes() % 64 == 0 && fir_lanes() + 64 <= nt;
    }
    // ... of one long window on four waves
    constexpr bool quad_fft_ok(bool has_fir, uint64_t nt) const {
        return defer_fft_ok(has_fir, nt) && G == 1 && W >= 256 && layers >= 1 && base_len >= 8 && fir_lanes() + 4 * 64 <= nt;
    }
    // rows of nt * spl samples one pass of the tile covers
    constexpr uint64_t rows(uint64_t nt, uint64_t spl) const { return ct_rows(pass_raw, nt * spl); }
    // fast phase 1 (kGeoFastP1): tiles start at (first_window + t G) S D — on a row boundary for every t when G S D is a multiple of
    // the row AND the launch's first window is (checked per launch) — and are exactly rch rows long
    constexpr bool fast_p1_ok(uint64_t nt, uint64_t spl, uint64_t rch, bool whole, bool aligned) const {
        return whole && aligned && ((kHalfTile ? kHalfOut : S) * D) % (nt * spl) == 0 && (G * S * D) % (nt * spl) == 0 && rch == rows(nt, spl) &&
               D % spl == 0 && (flags & kGeoFastP1);
    }
    // k_chain_pipe3: overlapping windows, straight-line shared FIR, <= 256 outputs per tile, row-aligned tiles (512 producer threads)
    constexpr bool pipe3_geometry_ok(uint64_t spl, uint64_t rch) const {
        return kShared && kUnrolledShared && Q <= 256 && (G * S * D) % (kPipe3Prod * spl) == 0 && rch == ct_rows(tile_raw, kPipe3Prod * spl) &&
               D % spl == 0 && W <= 64 * 16 && G >= 1;
    }
    constexpr uint64_t pipe3_q_pad() const { return (Q + 1) & ~1ull; }
    // k_spark2: W = base * 16 or base * 64
    constexpr bool spark2_ok() const {
        return (base_len == 8 || base_len == 16) && layers >= 1 && (W / base_len == 16 || W / base_len == 64) && S <= W && S >= 1 && D == 1 && T == 0;
    }
    // k_spark0: one base butterfly per window, dword-aligned windows (bps bytes per sample)
    constexpr bool spark0_ok(uint64_t bps) const {
        return W >= 2 && W <= 16 && S >= 1 && S <= W && D == 1 && T == 0 && (W * bps) % 4 == 0 && (S * bps) % 4 == 0;
    }
};

constexpr FixedRules fixed_rules(uint64_t W, uint64_t S, uint64_t D, uint64_t T, uint64_t G, uint32_t firb = 8, uint32_t firr = 1, uint32_t pad = 1,
                                 uint32_t batch = 1, uint32_t flags = 0) {
    FixedRules r{};
    r.W = W; r.S = S; r.D = D; r.T = T; r.G = G; r.flags = flags;
    r.kBatch = batch ? batch : 1;
    r.kFirBlock = firb;
    r.c = T - T / 2;
    r.tile_raw = ct_tile_raw(W, S, D, T, G);
    r.Q = (G - 1) * S + W;
    // outputs per lane in the FIR (register tiling).  The straight-line packed two-output form walks 4-sample blocks and needs
    // 4-aligned geometry only; the register-tiled form needs 8-aligned geometry and at least three interior 4-sample blocks
    r.kFirTile4 = firr == 2 && (flags & kGeoPackedTile) && pad == 2 && D % 4 == 0 && r.c % 4 == 0 && T % 4 == 0 && (T / 2) % 4 == 0 && W % 2 == 0 && S % 2 == 0 &&
                  ct_pow2(D) && D / 4 <= 8 && T > D + 16 && !(T > 0 && S < W);
    r.kFirTile = r.kFirTile4 ? 2u
               : (firr > 1 && D % 8 == 0 && (r.c % D) % 8 == 0 && T % 8 == 0 && (T / 2) % 8 == 0 && W % firr == 0 && S % firr == 0 && ct_pow2(D) && ct_pow2(firr) &&
                  T > (uint64_t)(firr - 1) * D + 8) ? firr : 1u;
    r.PD = D * r.kFirTile;      // LDS pad period: one pad group per PD samples
    r.pshift = ct_pow2(r.PD) ? ct_log2(r.PD) : 0xffffffffu;
    r.logW = ct_log2(W);
    r.kPad = (D % 2 == 0) ? ((pad == 2 && r.c % 2 == 0) ? 2u : 1u) : 0u;
    r.Dp = D + r.kPad;
    r.dshift = ct_pow2(D) ? ct_log2(D) : 0xffffffffu;
    r.dmagic = D > 1 ? (uint32_t)((1ull << 32) / D + 1) : 0u;
    r.a0 = r.c / D; r.b0 = r.c % D;
    r.T_fast = ct_min(T, D + T / 2);
    r.a1 = (r.c + r.T_fast) / D; r.b1 = (r.c + r.T_fast) % D;
    r.log_base = r.logW <= 3 ? r.logW : ((r.logW & 1) ? 3u : 4u);      // rustfft Radix4 plan: W = base_len * 4^layers
    r.base_len = 1u << r.log_base;
    r.layers = (r.logW - r.log_base) / 2;
    r.kHalfTile = (flags & kGeoHalfTile) && G == 1 && !(T > 0 && S < W) && W % 4 == 0 && T > 0;
    r.kHalfOut = W / 2;
    r.kHalfRaw = r.c + (r.kHalfOut - 1) * D + T;
    r.pass_raw = r.kHalfTile ? r.kHalfRaw : r.tile_raw;      // raw samples of one pass
    r.lds_raw_elems = ct_tile_elems(r.pass_raw, D, G * W, r.kPad ? r.kPad : 1);
    r.kNtrunc = r.c ? (r.c + D - 1) / D - 1 : 0;
    r.kShared = T > 0 && S < W && r.kNtrunc <= S;     // shared-FIR mode
    const bool pair_geo = r.kFirTile == 1 && r.kPad == 2 && T % 4 == 0 && r.b0 % 2 == 0 && D % 4 == 0 && T >= 32;
    r.kPairFir = (flags & kGeoNoSplit) && !r.kShared && pair_geo;             // packed lane-per-output FIR (fir_pair) on a 16-byte-row tile
    r.kUnrolledShared = (flags & kGeoUnrolledFir) && r.kShared && pair_geo;
    r.kPackedTile = (flags & kGeoPackedTile) && !r.kShared && r.kFirTile == 2 && r.kPad == 2 && (T / 2) % 4 == 0 && D / 4 <= 8;
    r.lds_raw_alloc = ct_tile_elems(r.pass_raw, D, G * W, pad);
    return r;
}

// ---------------------------------------------------------------- Pipe3S<FMT, GeoT, PT>: the streaming three-stage kernel
struct Pipe3sRules {
    uint64_t SPL, ROW, N, RN, GS, f0, RR, RINGD, MIRD, ROWP, RAW_ELEMS, DR, FBX_OFF, FBX_ALIGN, kLdsBytes, GH;
    bool kOverlap, fir_ok, ok, kWrite, kSwzFft;
    uint32_t kConsumerThreads;
};
constexpr Pipe3sRules pipe3s_rules(uint64_t spl, uint64_t pt, const FixedRules &g) {
    Pipe3sRules k{};
    const uint64_t W = g.W, S = g.S, D = g.D, T = g.T, G = g.G;
    k.SPL = spl; k.ROW = pt * spl;                                      // pt producer threads (pt / 64 waves), then four FIR and four FFT waves
    k.N = G * S * D; k.RN = k.N / k.ROW; k.GS = G * S;
    k.f0 = k.N >= g.c + T ? (k.N - g.c - T) / D + 1 : 0;                // full outputs the cold start's rows complete
    k.RR = (2 * k.N + T + 2 * D + k.ROW - 1) / k.ROW;                   // ring rows: two steps + a chain's look-back
    k.RINGD = k.RR * (k.ROW / D);                                       // ... in LDS rows of D samples
    k.MIRD = (g.b0 + T + D - 1) / D + 1;                                // mirror, in LDS rows
    k.ROWP = (k.ROW / D) * g.Dp;                                        // padded elements per row of ROW samples
    k.RAW_ELEMS = ((k.RINGD + k.MIRD) * g.Dp + 1) & ~1ull;
    k.DR = 3 * k.GS;
    // overlapping windows: the shared FIR keeps a full value AND a truncated snapshot per output (dec + trc); windows side by side
    // (S == W): every output belongs to one window and keeps the one value that window reads (dec only)
    k.kOverlap = S < W;
    k.fir_ok = k.kOverlap ? (g.kShared && g.kUnrolledShared)
                          : (S == W && g.kPad == 2 && T % 4 == 0 && g.b0 % 2 == 0 && D % 4 == 0 && T / 4 > 3 && (T / 2) % 4 == 0);
    k.ok = k.fir_ok && k.GS <= 256 && k.GS >= 1 && k.N % k.ROW == 0 && k.ROW % D == 0 && D % spl == 0 && W <= 64 * 16 && k.f0 >= 1 && k.f0 <= k.GS &&
           k.f0 > W - S && g.kNtrunc <= S && k.MIRD * D <= k.ROW && g.Q <= 2 * k.GS;
    k.kWrite = (g.flags & kGeoWriteSink) != 0;          // no FFT stage, no output ring
    // the two transform buffers (base pass of step s beside the layers of step s - 1) start on a 256-byte boundary: their swizzled layout
    // XORs into LDS byte addresses
    const uint64_t rings = k.RAW_ELEMS + (k.kOverlap ? 2u : 1u) * k.DR;
    k.FBX_OFF = (rings + 31u) & ~31ull;
    k.FBX_ALIGN = k.FBX_OFF - rings;
    // sample ring + mirror | dec (+ trc) rings of 3 G S | two G*W transform buffers | twiddles | taps; the write sink: sample ring | taps
    k.kLdsBytes = k.kWrite ? k.RAW_ELEMS * 8 + ct_taps_bytes(T) : (k.FBX_OFF + 2 * G * W + W) * 8 + ct_taps_bytes(T);
    // swizzled transform buffers need every wave's half of a buffer on a 256-byte boundary
    k.GH = (G + 1) / 2;
    k.kSwzFft = !k.kWrite && W >= 8 && (k.GH * W) % 32 == 0 && (G * W) % 32 == 0;
    k.kConsumerThreads = k.kWrite ? 256u : 512u;
    return k;
}

// ---------------------------------------------------------------- dynamic LDS of every family's layout, in bytes
// k_chain: raw tile | batch x G*W FFT buffers | twiddles | taps | 8-bit LUT | shared-FIR dec + trc | batch bookkeeping |
// tile-queue hand-over
constexpr uint64_t chain_lds_bytes(const FixedRules &g, bool lut8) {
    return g.lds_raw_alloc * 8 + g.kBatch * g.G * g.W * 8 + g.W * 8 + ct_taps_bytes(g.T) + (lut8 ? 256 * 4 : 0) +
           ((g.T && g.S < g.W) ? 2 * g.Q * 8 : 0) + g.kBatch * 16 + 16;
}
// the runtime-geometry kernels (interleaved tile, pad 1, batch 1, taps in LDS, always the full tile) run inside the same allocation
// for an unaligned slab tail
constexpr uint64_t generic_raw_elems(const FixedRules &g) { return ct_tile_elems(g.tile_raw, g.D, g.G * g.W, 1); }
constexpr uint64_t generic_lds_bytes(const FixedRules &g, bool lut8) {
    return generic_raw_elems(g) * 8 + g.G * g.W * 8 + g.W * 8 + ct_taps_bytes(g.T) + (lut8 ? 256 * 4 : 0) + ((g.T && g.S < g.W) ? 2 * g.Q * 8 : 0) + 16 + 16;
}
constexpr uint64_t kPipe3QueueBytes = 8;      // the claimed tile's index, low and high word
// k_chain_pipe3: two raw tiles | dec + trc of two sets | G*W FFT buffers | twiddles | taps | queue hand-over
constexpr uint64_t pipe3_lds_bytes(const FixedRules &g) {
    return 2 * g.lds_raw_alloc * 8 + 4 * g.pipe3_q_pad() * 8 + g.G * g.W * 8 + g.W * 8 + ct_taps_bytes(g.T) + kPipe3QueueBytes;
}
// k_spark / k_spark2: twiddles | four waves' transform buffers of ts samples (| the NCO lane table)
constexpr uint64_t spark_lds_bytes(uint64_t W, uint64_t ts, bool lane_table) { return (ct_max(W, 32) + 4 * ts) * 8 + (lane_table ? kSparkRow * kLaneEntryBytes : 0); }
// Historical slack the host adds on top of the layouts above ("where a kernel's geometry lives"): it keeps every plan's
// LDS size, and with it the workgroups per CU, where they were measured.
// The streaming layout was sized WITHOUT the transform buffers' alignment padding (Pipe3sRules::FBX_ALIGN, at most 31 elements) plus
// 320 bytes, so the host's size is kLdsBytes + kStreamLdsSlack - FBX_ALIGN * 8: never less than kLdsBytes.
constexpr uint64_t kPipe3LdsSlack = 64 - kPipe3QueueBytes, kStreamLdsSlack = 320, kStreamWriteLdsSlack = 64;
static_assert(31 * 8 < kStreamLdsSlack, "the streaming layout's slack covers FBX_OFF's rounding");

}  // namespace qd
