// qd_paint.h — waterfall pictures of norms rows (qd_plan_picture): k_paint turns a batch of the norms sink's windows
// into the pixels of the reference's `render` (src/ui/mod.rs:294-412): every fftshifted |X| through an HSV colour map, the columns laid into
// wrapped strips of an RGB image.  qd_picture_color and qd_picture_fold (quadrs_hip.hip) are the CPU twins and use the same functions.
//
// THE DEFINITION.  palette 0.5.0 (Cargo.lock:2650) is not at hand, so HSV -> RGB is PARITY UNPINNED, like rustfft: the project pins its own
// statement, the textbook conversion as palette 0.5 is recalled to write it.  "The reference's colours" means this statement.
//
// Colour of one norm.  Every operation is one IEEE f32 operation, separately rounded; nothing is contracted into an FMA; subnormals are kept.
//   scaled = x / scale                     (scale = 2.29 in the reference, :353)
//   s1     = 1.0 - scaled
//   hue    = (s1 * 0.8) * 360.0
//   val    = 1.0 - s1                      (not `scaled`: the reference subtracts twice, :361-366)
//   pos    = hue - floor(hue / 360.0) * 360.0
//   h      = pos / 60.0
//   c      = val * 1.0 ;  m = val - c
//   t      = h - 2.0 * floor(h * 0.5)      (h % 2 for finite h >= 0)
//   xx     = c * (1.0 - |t - 1.0|)
//   (r,g,b) = 0<=h<1:(c,xx,0)  1<=h<2:(xx,c,0)  2<=h<3:(0,c,xx)  3<=h<4:(0,xx,c)  4<=h<5:(xx,0,c)  else:(c,0,xx)
//   byte   = Rust's `as u8` of ((chan + m) * 256.0): truncate, saturate to 0..255, NaN -> 0
// The `else` branch also takes NaN, because every comparison is false there.  NaN and +inf give (0,0,0); 0 and -0 give (0,0,0); x >= scale
// saturates the red channel; 1e-40 gives (0,0,0).
//
// Page.  A picture is w x h pixels of 3 bytes R,G,B; pixel (x, y) lives at byte ((h - 1 - y) w + x) 3, so y = 0 is the bottom row
// (MemImage::set, :286-291).  With row_height = stretch W + 16, window p of the range (counted from the range's first window) is column
// x = p % w of strip r = p / w, whose origin is oy = r row_height.  The strip exists iff oy <= h (the reference tests `>`, :330): a strip at
// oy == h consumes its windows and shows nothing, so strips = h / row_height + 1 and at most strips w windows are ever looked at.  Bin o of
// the window, in the fftshifted order the norms sink writes, paints pixel rows y = oy + o stretch + off for off < stretch; rows with y >= h
// are skipped.  A column with scan >= 1 && p % scan == 0 is painted (0,0,0) in place of its colours (:374-376); scan == 0 means no marker
// columns (our one extension: the reference never has 0, and its default of 1 blackens every column).  The gap rows, and every pixel that
// no window reaches, are (0,0,0).  The reference's ensure!(w > fft_width) is a GUI to-do, not arithmetic: the library does not carry it.
//
// The first half of the header is plain C++17: it compiles on the host, where the CPU twins use it, and under hipcc for the kernel.
#ifndef QD_PAINT_H
#define QD_PAINT_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QD_PAINT_HD __host__ __device__
#else
#define QD_PAINT_HD
#endif

namespace qd {

constexpr uint32_t kPaintThreads = 256;
constexpr uint32_t kPaintCols = 64;              // columns (windows) of a tile
constexpr uint32_t kPaintBins = 16;              // bins of a tile
constexpr uint32_t kPaintPitch = kPaintCols + 1; // words of a bin's row of parked pixels: one word of padding (see k_paint)
constexpr uint32_t kPaintGap = 16;               // blank pixel rows between two strips (:311)
constexpr uint64_t kPaintMaxWorkspace = 1ull << 30;

// Rust's `as u8` of an f32: truncate, saturate to 0 ... 255, NaN -> 0
QD_PAINT_HD inline uint32_t paint_byte(float v) { return !(v > 0.0f) ? 0u : (v >= 255.0f ? 255u : (uint32_t)(int)v); }

// The colour of one norm, packed r | g << 8 | b << 16: the definition above, line for line.  The build never contracts (-ffp-contract=off)
// and `/` is the correctly rounded division on both sides.
QD_PAINT_HD inline uint32_t paint_color(float x, float scale) {
    const float scaled = x / scale;
    const float s1 = 1.0f - scaled;
    const float hue = (s1 * 0.8f) * 360.0f;
    const float val = 1.0f - s1;
    const float pos = hue - floorf(hue / 360.0f) * 360.0f;
    const float h = pos / 60.0f;
    const float c = val * 1.0f, m = val - c;
    const float t = h - 2.0f * floorf(h * 0.5f);
    const float xx = c * (1.0f - fabsf(t - 1.0f));
    float r, g, b;
    if (0.0f <= h && h < 1.0f) { r = c; g = xx; b = 0.0f; }
    else if (1.0f <= h && h < 2.0f) { r = xx; g = c; b = 0.0f; }
    else if (2.0f <= h && h < 3.0f) { r = 0.0f; g = c; b = xx; }
    else if (3.0f <= h && h < 4.0f) { r = 0.0f; g = xx; b = c; }
    else if (4.0f <= h && h < 5.0f) { r = xx; g = 0.0f; b = c; }
    else { r = c; g = 0.0f; b = xx; }
    return paint_byte((r + m) * 256.0f) | paint_byte((g + m) * 256.0f) << 8 | paint_byte((b + m) * 256.0f) << 16;
}

// A page for windows of width W: the checked qd_picture_desc and what follows from it.
struct PaintPage {
    uint32_t W, w, h, stretch, scan;
    float scale;
    uint64_t row_height, strips, max_windows, bytes;
};
inline void paint_page(uint32_t W, uint32_t w, uint32_t h, uint32_t stretch, uint32_t scan, float scale, PaintPage *G) {
    G->W = W; G->w = w; G->h = h; G->stretch = stretch; G->scan = scan; G->scale = scale;
    G->row_height = (uint64_t)stretch * W + kPaintGap;
    G->strips = h / G->row_height + 1;
    G->max_windows = G->strips * w;
    G->bytes = (uint64_t)w * h * 3;
}
QD_PAINT_HD inline bool paint_marker(uint64_t p, uint32_t scan) { return scan >= 1 && p % scan == 0; }

// Tiles.  A strip's columns are cut at the multiples of kPaintCols, so a tile never straddles a strip's wrap; tile t of the page is tile
// t % tiles_per_strip of strip t / tiles_per_strip.  A launch over windows [g0, g0 + nw) takes the tiles from the one that holds g0 to the
// one that holds g0 + nw - 1, each clipped to the batch, times ceil(W / kPaintBins) tiles of bins.
inline uint32_t paint_tiles_per_strip(uint32_t w) { return (w + kPaintCols - 1) / kPaintCols; }
inline uint64_t paint_tile_of(uint64_t p, uint32_t w) { return p / w * paint_tiles_per_strip(w) + (p % w) / kPaintCols; }

}  // namespace qd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace qd {

struct PaintParams {
    const float *norms;                          // the batch's windows, nw x W
    uint8_t *pixels;                             // the whole picture, any alignment
    uint64_t g0, nw;                             // windows [g0, g0 + nw) of the range, all below max_windows
    uint64_t tile0;                              // the page's tile that holds g0
    uint64_t row_height;
    uint32_t W, w, h, stretch, scan, tiles_per_strip, bin_tiles;
    float scale;
};

// One tile of at most kPaintCols columns x kPaintBins bins a workgroup.
//   read    lane t takes bin t % 16 of columns t / 16 + 16 k (k = 0 ... 3): the 16 lanes of a column read 64 consecutive bytes of its
//           window, colour them (a marker column stores zeros without evaluating the map) and park the packed pixel as one word at
//           [bin][column] of LDS.  The pitch of 65 words puts the 16 bins of a column on 16 banks; the two columns a half-wave holds
//           make the store 2-way, which a 4-byte LDS store hides.  16 x 65 words = 4160 bytes a workgroup.
//   store   a pixel row (bin, off) of the tile is one run of 3 tx consecutive bytes of the picture.  A wave takes a run at a time: lanes
//           0 ... 47 each build one of the run's 4-byte-aligned interior words from two neighbouring parked pixels (consecutive lanes read
//           consecutive or equal LDS words: no conflict) and store it whole; lanes 48 ... 50 store the at most three single bytes before
//           the first aligned word, lanes 51 ... 53 those behind the last.  Every byte of a run belongs to this tile alone and is
//           stored by exactly one lane once, so no word shared with a neighbouring tile is ever read or rewritten: no atomics, and no
//           dependence on batch or launch order.  Rows with y >= h are skipped row by row.
__global__ __launch_bounds__(kPaintThreads) void k_paint(const PaintParams Q) {
    __shared__ uint32_t s_px[kPaintBins * kPaintPitch];
    const uint32_t tid = threadIdx.x;
    const uint32_t bt = blockIdx.x % Q.bin_tiles;
    const uint64_t tile = Q.tile0 + blockIdx.x / Q.bin_tiles;
    const uint64_t r = tile / Q.tiles_per_strip;
    const uint64_t p_strip = r * Q.w;                                   // the strip's first window
    uint32_t xa = (uint32_t)(tile % Q.tiles_per_strip) * kPaintCols;
    uint32_t xb = xa + kPaintCols < Q.w ? xa + kPaintCols : Q.w;
    if (p_strip + xa < Q.g0) xa = (uint32_t)(Q.g0 - p_strip);           // the batch's seams may fall inside the tile
    if (p_strip + xb > Q.g0 + Q.nw) xb = (uint32_t)(Q.g0 + Q.nw - p_strip);
    if (xa >= xb) return;
    const uint32_t o0 = bt * kPaintBins;
    const uint32_t nb = Q.W - o0 < kPaintBins ? Q.W - o0 : kPaintBins;
    const uint64_t y0 = r * Q.row_height + (uint64_t)o0 * Q.stretch;    // the tile's lowest pixel row
    if (y0 >= Q.h) return;                                              // clipped whole (and the strip at oy == h)

    const uint32_t bl = tid % kPaintBins, xl = tid / kPaintBins;
    const uint32_t m0 = Q.scan ? (uint32_t)((p_strip + xa) % Q.scan) : 0u;
#pragma unroll
    for (uint32_t k = 0; k < kPaintCols / (kPaintThreads / kPaintBins); ++k) {
        const uint32_t xi = xl + k * (kPaintThreads / kPaintBins);
        if (xa + xi < xb && bl < nb) {
            const uint64_t m = (uint64_t)m0 + xi;                       // (p % scan) from the tile's first column: xi < 64
            const uint32_t mm = Q.scan > kPaintCols ? (uint32_t)(m >= Q.scan ? m - Q.scan : m) : (Q.scan ? (uint32_t)m % Q.scan : 1u);
            uint32_t px = 0;
            if (mm != 0) px = paint_color(Q.norms[(p_strip + xa + xi - Q.g0) * Q.W + o0 + bl], Q.scale);
            s_px[bl * kPaintPitch + xi] = px;
        }
    }
    __syncthreads();

    const uint32_t len = (xb - xa) * 3;                                 // bytes of a run
    // pixel rows of the tile: row q is y = y0 + q, bin q / stretch; those with y >= h are cut off
    const uint64_t all = (uint64_t)nb * Q.stretch, rows = all < Q.h - y0 ? all : Q.h - y0;
    const uint32_t lane = tid & 63u;
    for (uint64_t q = tid >> 6; q < rows; q += kPaintThreads / 64) {
        const uint64_t y = y0 + q;
        const uint32_t *row = s_px + ((uint32_t)q / Q.stretch) * kPaintPitch;
        uint8_t *dst = Q.pixels + ((uint64_t)(Q.h - 1 - y) * Q.w + xa) * 3;
        uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
        head = head < len ? head : len;
        const uint32_t nd = (len - head) / 4, tail = len - head - nd * 4;
        if (lane < nd) {
            const uint32_t at = head + lane * 4, px = at / 3, ch = at - px * 3;
            const uint64_t two = (uint64_t)row[px] | (uint64_t)row[px + 1] << 24;   // px + 1 <= 64: the padding word, whose bytes are then not used
            *reinterpret_cast<uint32_t *>(dst + at) = (uint32_t)(two >> (8 * ch));
        } else if (lane >= 48 && lane < 54) {
            const uint32_t i = lane < 51 ? lane - 48 : lane - 51;
            if (i < (lane < 51 ? head : tail)) {
                const uint32_t at = lane < 51 ? i : head + nd * 4 + i, px = at / 3, ch = at - px * 3;
                dst[at] = (uint8_t)(row[px] >> (8 * ch));
            }
        }
    }
}

}  // namespace qd
#endif  // __HIPCC__
#endif
