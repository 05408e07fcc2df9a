// qd_symbols.h — the symbol list (include/quadrs_hip.h, "symbol list"): one byte per FFT window of many short cf32 segments in one launch.
//
// The geometry and the LDS layout are stated in qd_symbols_plan.h, which also holds everything of the call that needs no HIP.  One kernel:
//   k_symbols<EPI>  workgroups of 256 lanes as four independent waves, one tile (a run of windows of one segment) per wave, no workgroup
//                   barrier anywhere: a wave's LDS slice is its own, and LDS operations of one wave execute in order.  The wave loads its
//                   tile's windows from the cf32 buffer - windows side by side (stride == width) are one span, read with 16-byte loads
//                   over its 16-byte aligned middle and 8-byte loads at the ragged ends, as k_cuts reads, since a segment starts at any
//                   element; any other stride loads each window's samples again with 8-byte loads (correct, not tuned: the cuts are small
//                   and L2-resident) -, multiplies by the window table where the desc asks for one, parks the samples in rustfft's
//                   transposed input order, transforms them with wave_fft_epilogue_fn<DynGeo, 0, 3> on the runtime geometry and runs
//                   wave_bucket_epilogue_fn or wave_mark_epilogue_fn of qd_chain.h: the arithmetic of a plan's sink, single-sourced.
// The tile table, the layer twiddles and the window table are plain device memory written with ordinary copies; the bytes are ordinary
// vector stores.
#pragma once

#include "qd_symbols_plan.h"

#if defined(__HIPCC__)
#include "qd_chain.h"

namespace qd {

// P: W, logW, S (clamped to 2^31: a larger stride leaves a segment one window at most), base_len, log_base, layers, tw, window (or NULL),
// rmin, the butterfly constants, out = byte 0 of the output, out_window0 = 0.
template <int EPI>
__global__ __launch_bounds__(kSymThreads) void k_symbols(const ChainParams P, const float2 *__restrict__ in, const SymTile *__restrict__ tiles, uint32_t n_tiles) {
    extern __shared__ __attribute__((aligned(16))) float2 sym_lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const DynGeo geo(P);
    const uint32_t W = geo.W, logW = geo.logW, S = P.S;
    const uint32_t waves = symbols_waves(W);
    if (wave >= waves) return;
    const uint64_t t = (uint64_t)blockIdx.x * waves + wave;
    if (t >= n_tiles) return;
    const SymTile tl = tiles[t];
    float2 *fb = sym_lds + wave * symbols_slice(W);
    const uint32_t n = tl.count << logW;                                       // <= symbols_slice(W): symbols_tiles keeps a tile inside its slice

    // source -> [window] -> the slice, transposed (src/ffts.rs:64-68; rustfft's bitreversed_transpose)
    const uint32_t lw = 2 * geo.layers, xmask = (1u << lw) - 1u;
    auto put = [&](uint32_t e, float2 v) {
        const uint32_t k = e & (W - 1u);
        if (P.window) { const float wv = P.window[k]; v.x = v.x * wv; v.y = v.y * wv; }
        fb[(e & ~(W - 1u)) + (k >> lw) + (rev4(k & xmask, geo.layers) << geo.log_base)] = v;
    };
    const float2 *p0 = in + tl.src_at;
    if (S == W) {
        uint32_t head = (uint32_t)(((16u - (uint32_t)((uintptr_t)p0 & 15u)) & 15u) / 8u);      // samples ahead of the first 16-byte boundary
        if (head > n || ((uintptr_t)p0 & 7u)) head = n;                                      // (a buffer that is not even sample-aligned: no wide loads)
        const uint32_t n_vec = (n - head) / 2u, tail = head + n_vec * 2u;
        for (uint32_t k = lane; k < head; k += 64) put(k, p0[k]);
        for (uint32_t v = lane; v < n_vec; v += 64) {
            const float4 q = *reinterpret_cast<const float4 *>(p0 + head + 2u * v);
            put(head + 2u * v, make_float2(q.x, q.y));
            put(head + 2u * v + 1u, make_float2(q.z, q.w));
        }
        for (uint32_t k = tail + lane; k < n; k += 64) put(k, p0[k]);
    } else {
        for (uint32_t e = lane; e < n; e += 64) put(e, p0[(uint64_t)(e >> logW) * S + (e & (W - 1u))]);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    wave_fft_epilogue_fn<DynGeo, 0, 3>(P, geo, P.tw, fb, 0, tl.count, tid);
    if constexpr (EPI == QD_EPI_BUCKET2_U8)
        wave_bucket_epilogue_fn<DynGeo, 2 * kSymSliceSamples / 64>(P, geo, fb, tl.out_at, tl.count, lane);
    else
        wave_mark_epilogue_fn<DynGeo>(P, geo, [&](uint32_t o) { return fb[o]; }, reinterpret_cast<uint8_t *>(P.out) + tl.out_at, tl.count, lane);
}

}  // namespace qd
#endif  // __HIPCC__
