// qd_cuts_plan.h — the cut list's planning, all of it that needs no HIP: the kernel's geometry, cut validation, the emission -> cut
// arithmetic, the tile table and the batch planner.  Plain C++17: quadrs_hip.hip includes it through qd_cuts.h, and a host program can
// include it alone (scripts/cuts_host_check.cpp walks it under the sanitizers against brute force).
//
// GEOMETRY of k_cuts (qd_cuts.h), stated once.  One workgroup of kCutsThreads lanes runs one TILE: outputs [first, first + count) of one
// cut, count <= cuts_tile_outputs(D, T) = min(kCutsThreads, (kCutsTileSamples - T) / D), so that the source samples the tile reads,
// at most (count - 1) D + T of them, fit the LDS tile of kCutsTileSamples samples and every output has a lane of its own.  At D = 1024,
// T = 4096 that is 5 outputs on 5 lanes: correct, not tuned.
// LDS layout: sample k of the tile (k = 0 is the tile's first source sample, first D + c of the cut's span) is the float2 at element
// cuts_lds_index(k) = k + k / 32: rows of 32 samples with one pad sample behind each.  Phase 2 reads 8 bytes per lane (ds_read_b64:
// the two 32-lane halves are served separately, 64 banks of 4 bytes, so 32 lanes are conflict-free when their sample elements differ
// mod 32); lane l reads element index(l D + j), and without the pad lanes D apart would share a bank pair gcd(D, 32)-fold - all 32 of
// them for D = 32.  With the pad, l D + (l D) / 32 runs through all residues for every D that divides 32 and stays at most 2-fold
// for D = 64; larger D are out of tuning scope (a tile holds few outputs there anyway).  Behind the samples lie kCutsTileRows RowBase
// entries, the NCO row bases of the rows of kCutsNcoRow absolute samples the tile touches (at most 9216 / 512 + 1 = 19).
#pragma once

#include "../../include/quadrs_hip.h"

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

namespace qd {

constexpr uint32_t kCutsThreads = 256;
constexpr uint32_t kCutsTileSamples = 9216;
constexpr uint32_t kCutsNcoRow = 512;                                          // qd_shift's row grid
constexpr uint32_t kCutsTileRows = kCutsTileSamples / kCutsNcoRow + 2;
constexpr uint32_t kCutsLdsRow = 32;
constexpr uint32_t cuts_lds_index(uint32_t k) { return k + k / kCutsLdsRow; }
constexpr uint32_t kCutsLdsSamples = cuts_lds_index(kCutsTileSamples) + 1;
constexpr uint32_t kCutsLdsBytes = kCutsLdsSamples * 8 + kCutsTileRows * 32;      // 76680: two workgroups per CU
constexpr uint32_t kCutsBatchTiles = 16384;                                    // tiles per launch: bounds the tile and row tables (10.5 MiB)
constexpr uint64_t kCutsMaxCount = 1ull << 31;
constexpr uint64_t kCutsDefaultChunk = 64ull << 20;

constexpr uint32_t cuts_tile_outputs(uint64_t D, uint64_t T) {
    const uint64_t fit = (kCutsTileSamples - T) / D;
    return (uint32_t)(fit < kCutsThreads ? fit : kCutsThreads);
}
static_assert(QD_CUT_MAX_DECIMATE + QD_CUT_MAX_TAPS <= kCutsTileSamples, "every admissible cut has a tile of at least one output");
static_assert(2 * kCutsLdsBytes <= 160 * 1024, "two workgroups per CU");

// One workgroup's work.  src_off: absolute source sample n lies at element n + src_off of the launch's source buffer.
struct CutTile { uint32_t job, first, count, _pad; uint64_t out_at; int64_t src_off; };

// the source samples outputs [o0, o0 + no) of a cut read: [lo, hi), absolute
inline void cut_reads(const qd_cut &c, uint64_t o0, uint64_t no, uint64_t *lo, uint64_t *hi) {
    const uint64_t D = c.decimate, T = c.taps, ctr = T - T / 2, valid = c.count * D + T, base = c.first * D;
    *lo = base + o0 * D + ctr;
    *hi = base + std::min(valid, (o0 + no - 1) * D + ctr + T);
}

inline int cuts_fail(std::string *err, int code, const char *fmt, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    if (err) *err = buf;
    return code;
}

// The validation of include/quadrs_hip.h, in its order.  offsets: n_cuts + 1 entries or NULL.  slab: check the spans against
// [src_first, +src_count).  *hull_first / *hull_count (may be NULL): the hull of the spans, 0 / 0 without one.
inline int cuts_check(uint64_t sample_rate, uint64_t n_samples, const qd_cut *cuts, size_t n_cuts, bool slab, uint64_t src_first, uint64_t src_count,
                      uint64_t *offsets, uint64_t *hull_first, uint64_t *hull_count, std::string *err) {
    if (n_cuts && !cuts) return cuts_fail(err, QD_ERR_INVALID, "cuts is NULL");
    uint64_t total = 0, lo = ~0ull, hi = 0;
    for (size_t k = 0; k < n_cuts; ++k) {
        const qd_cut &c = cuts[k];
        const unsigned long long kk = k;
        if (c.decimate == 0) return cuts_fail(err, QD_ERR_PANIC, "cut %llu: decimate 0 (src/filter.rs:47)", kk);
        if (c.taps < 2) return cuts_fail(err, QD_ERR_PANIC, "cut %llu: size < 2 (src/filter.rs:74)", kk);
        const uint64_t mag = c.shift_hz < 0 ? 0 - (uint64_t)c.shift_hz : (uint64_t)c.shift_hz;
        if (c.shift_hz != 0 && mag >= sample_rate / 2)
            return cuts_fail(err, QD_ERR_PANIC, "cut %llu: frequency must be under half the sample rate %llu (src/shift.rs:20-24)", kk, sample_rate);
        if (c.decimate > QD_CUT_MAX_DECIMATE) return cuts_fail(err, QD_ERR_UNSUPPORTED, "cut %llu: decimate %llu above QD_CUT_MAX_DECIMATE", kk, c.decimate);
        if (c.taps > QD_CUT_MAX_TAPS) return cuts_fail(err, QD_ERR_UNSUPPORTED, "cut %llu: %llu taps, above QD_CUT_MAX_TAPS", kk, c.taps);
        if (c.count > kCutsMaxCount) return cuts_fail(err, QD_ERR_UNSUPPORTED, "cut %llu: count %llu above 2^31", kk, c.count);
        if (offsets) offsets[k] = total;
        total += c.count;
        if (c.count == 0) continue;
        const uint64_t valid = c.count * c.decimate + c.taps;                  // < 2^42
        if (n_samples < valid || c.first > (n_samples - valid) / c.decimate)
            return cuts_fail(err, QD_ERR_SHORT, "cut %llu: its block of %llu source samples ends past the stream's %llu (a cut is one full read_at block)", kk, valid, n_samples);
        const uint64_t a = c.first * c.decimate, b = a + valid;
        if (slab && (a < src_first || b - src_first > src_count))
            return cuts_fail(err, QD_ERR_INVALID, "cut %llu: its source span is not inside the slab [%llu, +%llu)", kk, src_first, src_count);
        lo = std::min(lo, a);
        hi = std::max(hi, b);
    }
    if (offsets) offsets[n_cuts] = total;
    if (hull_first) *hull_first = hi ? lo : 0;
    if (hull_count) *hull_count = hi ? hi - lo : 0;
    return QD_OK;
}

// ---------------------------------------------------------------- emission -> cut (the arithmetic of include/quadrs_hip.h)

typedef __int128 cuts_i128;
inline cuts_i128 cuts_fdiv(cuts_i128 a, cuts_i128 b) { const cuts_i128 q = a / b, r = a % b; return (r != 0 && ((r < 0) != (b < 0))) ? q - 1 : q; }
inline cuts_i128 cuts_cdiv(cuts_i128 a, cuts_i128 b) { return -cuts_fdiv(-a, b); }

inline int cut_of_emission(const qd_chain_desc *desc, uint64_t first_window, const qd_emission *e, const qd_cut_rule *rule, qd_cut *cut, std::string *err) {
    typedef cuts_i128 I;
    if (!desc || !e || !rule || !cut) return cuts_fail(err, QD_ERR_INVALID, "NULL argument");
    if (desc->struct_size != sizeof(qd_chain_desc)) return cuts_fail(err, QD_ERR_INVALID, "desc.struct_size is not sizeof(qd_chain_desc)");
    if (rule->struct_size != sizeof(qd_cut_rule)) return cuts_fail(err, QD_ERR_INVALID, "rule.struct_size is not sizeof(qd_cut_rule)");
    if (rule->oversample == 0) return cuts_fail(err, QD_ERR_INVALID, "oversample is 0");
    if (rule->taps != 0 && rule->taps < 2) return cuts_fail(err, QD_ERR_INVALID, "rule.taps %llu: 0 (chosen from the decimation) or at least 2", rule->taps);
    const uint64_t sr = desc->sample_rate, W = desc->width, S = desc->stride;
    if (e->first > e->last) return cuts_fail(err, QD_ERR_INVALID, "the emission's first window %llu lies behind its last %llu", e->first, e->last);
    if (e->lo > e->hi || e->hi >= W) return cuts_fail(err, QD_ERR_INVALID, "bins %llu ... %llu are not bins of a %llu-point window", e->lo, e->hi, W);
    if (sr == 0 || S == 0 || (desc->has_lowpass && desc->decimate == 0)) return cuts_fail(err, QD_ERR_INVALID, "desc: sample_rate, stride or decimate is 0");
    if (sr >> 48) return cuts_fail(err, QD_ERR_UNSUPPORTED, "sample rate %llu is 2^48 or more", sr);
    const uint64_t D0 = desc->has_lowpass ? desc->decimate : 1, T0 = desc->has_lowpass ? desc->taps : 0;
    const I R = (I)(sr / D0), f0 = desc->has_shift ? (I)desc->shift_hz : 0;
    // the far end of the emission's source span, refused where it leaves 62 bits (each factor first, so that nothing wraps on the way)
    const I limit = (I)1 << 62;
    const I w_last = (I)first_window + (I)e->last;
    if (w_last >= limit || (I)S >= limit || (I)D0 >= limit || (I)W >= limit || (I)T0 >= limit || w_last * (I)S >= limit || w_last * (I)S * (I)D0 >= limit ||
        (I)W * (I)D0 >= limit || w_last * (I)S * (I)D0 + (I)W * (I)D0 + (I)T0 >= limit)
        return cuts_fail(err, QD_ERR_UNSUPPORTED, "the emission's source span ends at or past sample 2^62");
    const I nu = cuts_fdiv(((I)e->lo + (I)e->hi - (I)W) * R + (I)W, 2 * (I)W);
    I s = (f0 - nu) % (I)sr;
    if (s < 0) s += (I)sr;
    const I hs = (I)(sr / 2);
    if (s >= hs) s -= (I)sr;
    if (s <= -hs) s = 1 - hs;
    const I lp = std::max<I>(1, cuts_cdiv(((I)e->hi - (I)e->lo + 1 + 2 * (I)rule->guard_bins) * R, 2 * (I)W));
    const I dmax = rule->max_decimate ? (I)rule->max_decimate : (I)QD_CUT_MAX_DECIMATE;
    const I D = std::min<I>(std::max<I>((I)sr / (2 * (I)rule->oversample * lp), 1), dmax);
    const I T = rule->taps ? (I)rule->taps : std::min<I>((I)QD_CUT_MAX_TAPS, std::max<I>(40, 8 * D));
    const I n = (I)desc->n_samples, pad = (I)rule->pad;
    const I a = ((I)first_window + (I)e->first) * (I)S * (I)D0;
    const I b = std::min<I>(n, w_last * (I)S * (I)D0 + (I)W * (I)D0 + (I)T0);
    const I first = std::max<I>(0, cuts_fdiv(a - T, D) - pad);
    const I end = cuts_cdiv(std::max<I>(b - T, 0), D) + pad + cuts_cdiv(T - T / 2, D);
    const I count = std::max<I>(0, std::min<I>(end, cuts_fdiv(n - T, D)) - first);
    cut->shift_hz = (int64_t)s;
    cut->lowpass_hz = (uint64_t)lp;
    cut->decimate = (uint64_t)D;
    cut->taps = (uint64_t)T;
    cut->first = (uint64_t)first;
    cut->count = (uint64_t)count;
    return QD_OK;
}

// ---------------------------------------------------------------- pieces, batches, tiles

// A piece: outputs [first, first + count) of cut `cut`, whole tiles of it except for the cut's last; reads source samples [lo, hi).
// out_at: where its outputs start in the batch's own output buffer.  span: the batch's merged span that holds [lo, hi).
struct CutPiece { uint32_t cut, first, count, span; uint64_t lo, hi, out_at; };
// A merged span of a batch: absolute samples [first, first + count), uploaded to element `at` of the batch's source buffer.
struct CutSpan { uint64_t first, count, at; };
struct CutBatch {
    std::vector<CutPiece> pieces;
    std::vector<CutSpan> spans;
    uint64_t src_samples = 0, out_samples = 0, tiles = 0;
};

inline uint64_t cut_piece_tiles(const qd_cut &c, const CutPiece &p) { const uint64_t to = cuts_tile_outputs(c.decimate, c.taps); return (p.count + to - 1) / to; }

// Validated cuts -> batches.  Every output of every cut lies in exactly one piece of exactly one batch; a batch's merged spans are the
// union of its pieces' reads, sorted, disjoint and non-adjacent; a batch reads at most max(budget, one tile's span) source samples and
// holds at most kCutsBatchTiles tiles.  budget: source samples per batch.
inline void cuts_batches(const qd_cut *cuts, size_t n_cuts, uint64_t budget, std::vector<CutBatch> *out) {
    out->clear();
    std::vector<CutPiece> all;
    for (size_t k = 0; k < n_cuts; ++k) {
        const qd_cut &c = cuts[k];
        if (c.count == 0) continue;
        const uint64_t to = cuts_tile_outputs(c.decimate, c.taps), step = to * c.decimate;
        uint64_t tiles_fit = budget > c.taps + step ? (budget - c.taps) / step : 1;
        tiles_fit = std::min<uint64_t>(tiles_fit, kCutsBatchTiles);
        const uint64_t per = tiles_fit * to;
        for (uint64_t o = 0; o < c.count; o += per) {
            CutPiece p{};
            p.cut = (uint32_t)k; p.first = (uint32_t)o; p.count = (uint32_t)std::min<uint64_t>(per, c.count - o);
            cut_reads(c, o, p.count, &p.lo, &p.hi);
            all.push_back(p);
        }
    }
    std::stable_sort(all.begin(), all.end(), [](const CutPiece &x, const CutPiece &y) { return x.lo < y.lo; });
    CutBatch cur;
    uint64_t cur_end = 0;
    auto close = [&]() { if (!cur.pieces.empty()) out->push_back(std::move(cur)); cur = CutBatch(); cur_end = 0; };
    for (CutPiece p : all) {
        const uint64_t tiles = cut_piece_tiles(cuts[p.cut], p);
        for (int attempt = 0; attempt < 2; ++attempt) {
            const bool joins = !cur.spans.empty() && p.lo <= cur_end;
            const uint64_t added = joins ? (p.hi > cur_end ? p.hi - cur_end : 0) : p.hi - p.lo;
            if (!cur.pieces.empty() && (cur.src_samples + added > budget || cur.tiles + tiles > kCutsBatchTiles)) { close(); continue; }
            if (joins) cur.spans.back().count += added;
            else cur.spans.push_back(CutSpan{p.lo, p.hi - p.lo, cur.src_samples});
            cur_end = cur.spans.back().first + cur.spans.back().count;
            p.span = (uint32_t)(cur.spans.size() - 1);
            p.out_at = cur.out_samples;
            cur.src_samples += added; cur.out_samples += p.count; cur.tiles += tiles;
            cur.pieces.push_back(p);
            break;
        }
    }
    close();
}

// The tile table of a batch.  direct_out: the kernel stores into the caller's `out` (element offsets[cut] + output), else into the batch's
// own buffer (piece.out_at + ...).  direct_src: the kernel reads the caller's slab, whose element 0 is absolute sample src_first, else
// the batch's upload of its merged spans.
inline void cuts_tiles(const qd_cut *cuts, const CutBatch &b, bool direct_out, const uint64_t *offsets, bool direct_src, uint64_t src_first,
                       std::vector<CutTile> *tiles) {
    tiles->clear();
    tiles->reserve((size_t)b.tiles);
    for (const CutPiece &p : b.pieces) {
        const qd_cut &c = cuts[p.cut];
        const uint32_t to = cuts_tile_outputs(c.decimate, c.taps);
        const CutSpan &sp = b.spans[p.span];
        for (uint32_t o = 0; o < p.count; o += to) {
            CutTile t{};
            t.job = p.cut; t.first = p.first + o; t.count = std::min<uint32_t>(to, p.count - o);
            t.out_at = direct_out ? offsets[p.cut] + p.first + o : p.out_at + o;
            t.src_off = direct_src ? -(int64_t)src_first : (int64_t)sp.at - (int64_t)sp.first;
            tiles->push_back(t);
        }
    }
}

}  // namespace qd
