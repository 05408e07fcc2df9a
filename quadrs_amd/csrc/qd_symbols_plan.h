// qd_symbols_plan.h — the symbol list's planning, all of it that needs no HIP: the window-count rules, the offsets, the validation, the
// tile table and the grouping of qd_cuts_symbols.  Plain C++17: quadrs_hip.hip includes it through qd_symbols.h, and a host program can
// include it alone (scripts/symbols_host_check.cpp walks it under the sanitizers against brute force).
//
// GEOMETRY of k_symbols (qd_symbols.h), stated once.  A workgroup of kSymThreads = 256 lanes is four independent waves; a TILE is a run of
// consecutive windows [first, first + count) of ONE segment and is handed to ONE wave, because both epilogues want the whole window on
// one wave (one_wave_sink, qd_chain.h).  Tile t of a launch runs on wave t % waves of workgroup t / waves, waves = symbols_waves(W).
// count <= symbols_tile_windows(W) = slice / W, slice = symbols_slice(W) samples: the tile's windows lie side by side in the wave's LDS
// slice, window g at elements [g W, (g + 1) W).  Window r of the tile reads elements [src_at + r S, src_at + r S + W) of the launch's
// cf32 buffer and writes byte out_at + r.
// LDS layout: kSymLdsBytes = 64 KiB of float2 per workgroup, so that two workgroups share a CU's 160 KiB.  Up to W = 2048 that is four
// slices of 2048 samples (16 KiB), one per wave; at W = 4096 a window needs 32 KiB, so the workgroup is cut into two slices of 4096
// samples and only waves 0 and 1 take tiles (waves 2 and 3 leave at once).  Inside a slice sample k of window g is parked at
// g W + yy + (rev4(xx, layers) << log_base), xx = k mod 4^layers, yy = k / 4^layers: rustfft's transposed input order, which
// wave_fft_epilogue_fn expects.  The bucket epilogue overwrites the front of the slice with the f32 norms.  No other LDS.
#pragma once

#include "../../include/quadrs_hip.h"

#include <algorithm>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace qd {

constexpr uint32_t kSymThreads = 256;
constexpr uint32_t kSymSliceSamples = 2048;
constexpr uint32_t kSymLdsBytes = 4 * kSymSliceSamples * 8;                   // 65536
constexpr uint32_t kSymBatchTiles = 65536;                                     // tiles per launch: bounds the tile table (1.5 MiB)
constexpr uint64_t kSymMaxCount = 1ull << 31;
constexpr uint64_t kSymDefaultIqBytes = 1ull << 30;
static_assert(2 * kSymLdsBytes <= 160 * 1024, "two workgroups per CU");
static_assert(2 * QD_SYMBOLS_MAX_WIDTH * 8 <= kSymLdsBytes, "two waves hold a window of the largest width each");

constexpr uint32_t symbols_slice(uint64_t W) { return W > kSymSliceSamples ? 2 * kSymSliceSamples : kSymSliceSamples; }
constexpr uint32_t symbols_waves(uint64_t W) { return kSymLdsBytes / 8 / symbols_slice(W); }
constexpr uint32_t symbols_tile_windows(uint64_t W) { return (uint32_t)(symbols_slice(W) / W); }

// One wave's work: windows of one segment.  src_at: element of the launch's cf32 buffer that holds sample 0 of the tile's first window.
struct SymTile { uint64_t src_at, out_at; uint32_t count, _pad; };

inline int symbols_fail(std::string *err, int code, const char *fmt, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    if (err) *err = buf;
    return code;
}

// the windows of a segment of `count` samples: the bucket sink's (src/fft.rs:86) and the mark sink's (src/fft.rs:28,65); count <= W: none
inline uint64_t symbols_windows(int epilogue, uint64_t count, uint64_t W, uint64_t S) {
    if (count <= W) return 0;
    const uint64_t lim = count - W;
    return epilogue == QD_EPI_BUCKET2_U8 ? lim / S : (lim - 1) / S + 1;
}

// the desc's own checks, in the header's order
inline int symbols_check_desc(const qd_symbols_desc *d, std::string *err) {
    if (!d) return symbols_fail(err, QD_ERR_INVALID, "desc is NULL");
    if (d->struct_size != sizeof(qd_symbols_desc)) return symbols_fail(err, QD_ERR_INVALID, "desc.struct_size is not sizeof(qd_symbols_desc)");
    if (d->epilogue != QD_EPI_BUCKET2_U8 && d->epilogue != QD_EPI_MARK_U8)
        return symbols_fail(err, QD_ERR_INVALID, "epilogue %llu: a symbol list is QD_EPI_BUCKET2_U8 or QD_EPI_MARK_U8", (unsigned long long)(uint32_t)d->epilogue);
    if (d->stride == 0) return symbols_fail(err, QD_ERR_INVALID, "stride 0 never terminates in the reference (src/fft.rs:65)");
    if (d->windowing != 0 && d->windowing != 1) return symbols_fail(err, QD_ERR_INVALID, "windowing %llu: 0 (none) or 1 (Blackman-Harris)", (unsigned long long)(uint32_t)d->windowing);
    if (d->width == 0 || (d->width & (d->width - 1)))
        return symbols_fail(err, QD_ERR_PANIC, "Radix4 requires a power-of-two width (rustfft API contract), got %llu", d->width);
    if (d->width > QD_SYMBOLS_MAX_WIDTH) return symbols_fail(err, QD_ERR_UNSUPPORTED, "width %llu above QD_SYMBOLS_MAX_WIDTH", d->width);
    return QD_OK;
}

// The validation of include/quadrs_hip.h behind the desc's.  offsets: n + 1 entries or NULL.  bounded: check the segments against n_in.
// *hull_first / *hull_count (may be NULL): the hull of the segments that have a window, 0 / 0 without one.
inline int symbols_check(const qd_symbols_desc *d, const qd_segment *segs, size_t n, bool bounded, uint64_t n_in, uint64_t *offsets,
                         uint64_t *hull_first, uint64_t *hull_count, std::string *err) {
    if (const int rc = symbols_check_desc(d, err)) return rc;
    if (n && !segs) return symbols_fail(err, QD_ERR_INVALID, "segments is NULL");
    uint64_t total = 0, lo = ~0ull, hi = 0;
    for (size_t k = 0; k < n; ++k) {
        const qd_segment &s = segs[k];
        if (s.count > kSymMaxCount) return symbols_fail(err, QD_ERR_UNSUPPORTED, "segment %llu: count %llu above 2^31", k, s.count);
        if (bounded && (s.count > n_in || s.first > n_in - s.count))
            return symbols_fail(err, QD_ERR_SHORT, "segment %llu: it ends past the buffer's %llu samples", k, n_in);
        if (offsets) offsets[k] = total;
        const uint64_t nw = symbols_windows(d->epilogue, s.count, d->width, d->stride);
        total += nw;
        if (nw == 0) continue;
        lo = std::min(lo, s.first);
        hi = std::max(hi, s.first + s.count);
    }
    if (offsets) offsets[n] = total;
    if (hull_first) *hull_first = hi ? lo : 0;
    if (hull_count) *hull_count = hi ? hi - lo : 0;
    return QD_OK;
}

// ---------------------------------------------------------------- tiles

// Where the tile table stands: the next tile starts at window `win` of segment `seg`.
struct SymCursor { size_t seg = 0; uint64_t win = 0; };

// The next at most `cap` tiles of validated segments, in list order; true while tiles remain behind them.  Every window of every
// segment lies in exactly one tile.  base: element 0 of the launch's buffer is element `base` of the caller's.
inline bool symbols_tiles(const qd_symbols_desc *d, const qd_segment *segs, size_t n, const uint64_t *offsets, uint64_t base, SymCursor *cur, size_t cap,
                          std::vector<SymTile> *tiles) {
    tiles->clear();
    const uint64_t W = d->width, S = d->stride, per = symbols_tile_windows(W);
    while (cur->seg < n) {
        const qd_segment &s = segs[cur->seg];
        const uint64_t nw = symbols_windows(d->epilogue, s.count, W, S);
        if (cur->win >= nw) { ++cur->seg; cur->win = 0; continue; }
        if (tiles->size() >= cap) return true;
        SymTile t{};
        t.count = (uint32_t)std::min<uint64_t>(per, nw - cur->win);
        t.src_at = s.first + cur->win * S - base;
        t.out_at = offsets[cur->seg] + cur->win;
        tiles->push_back(t);
        cur->win += t.count;
    }
    return false;
}

// ---------------------------------------------------------------- the groups of qd_cuts_symbols

// Cuts in list order, in groups [k0, k1) of whole cuts whose IQ (8 bytes an output) fits iq_bytes (0: kSymDefaultIqBytes); every cut lies
// in exactly one group, the empty ones included.  A single cut above the cap: QD_ERR_UNSUPPORTED.
inline int symbols_groups(const qd_cut *cuts, size_t n_cuts, uint64_t iq_bytes, std::vector<std::pair<size_t, size_t>> *groups, std::string *err) {
    groups->clear();
    const uint64_t cap = (iq_bytes ? iq_bytes : kSymDefaultIqBytes) / 8;
    size_t k0 = 0;
    uint64_t held = 0;
    for (size_t k = 0; k < n_cuts; ++k) {
        const uint64_t c = cuts[k].count;
        if (c > cap)
            return symbols_fail(err, QD_ERR_UNSUPPORTED, "cut %llu: its %llu outputs do not fit the IQ workspace of %llu bytes: lower the count or raise iq_bytes", k, c, cap * 8);
        if (held + c > cap) { groups->push_back({k0, k}); k0 = k; held = 0; }
        held += c;
    }
    if (k0 < n_cuts) groups->push_back({k0, n_cuts});
    return QD_OK;
}

}  // namespace qd
