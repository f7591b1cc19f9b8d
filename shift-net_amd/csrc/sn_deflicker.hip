// Brightness flicker taken out on the device (gfx950), for `restore_video --deflicker`: planar Y'CbCr payloads in, payloads of the same format out.
// No float frame is made and no colour conversion runs; the rule that turns histograms into tables is the host's (shiftnet_amd/deflicker.py).
//
//   sn_yuv_code_hist : T payloads -> [T][2^bits] uint32, the exact counts of the luma codes of every payload, whole frames or a picture rectangle.
//   sn_yuv_apply_lut : T payloads + [T][2][2^bits] uint16 tables (Y; Cb and Cr) -> T payloads, dst[sample] = lut[plane][src[sample]], in place if asked.
//
// Both index with min(code, 2^bits - 1): a 10-bit payload is 16-bit words and may hold anything.
//
// The histogram.  A lane owns a unit of 16 bytes of a luma row (16 samples at 8 bit, 8 at 10: one wide load where the address allows it, element-wise
// otherwise and on the ragged right edge); a workgroup walks units gridDim.x * 256 apart of one frame.  The counts live in LDS in COPIES copies, copy
// (lane & (COPIES - 1)) of bin c at word c * COPIES + copy, as the noise histograms of csrc/sn_yuv_stats.hip keep their low bins: with 32 copies (8 bit)
// the 32 lanes of an LDS lane group hit 32 different banks whatever their bins, so no add ever meets a bank conflict or a second lane on its own word.
// At 10 bit 32 KB hold 8 copies: lanes 8 apart share a word.  A FLAT frame -- bars, a fade to black: an ordinary frame here -- sends every sample to one
// bin, so on top of the copies a lane adds RUNS: equal neighbours among its own samples become one LDS atomic with the run's length.  A flat 8-bit unit
// is one atomic instead of 16, on a word no other lane of its group touches; a noisy one pays a few compares.  At the end the copies are summed, each
// lane starting at another copy, and the non-zero bins go to dst with one global atomic each.  Integer sums commute: the counts do not depend on the
// geometry or the schedule.
//
// The tables.  A workgroup owns 256 x 64 luma samples of one frame (32 x 8 threads of 8 x 2 samples, four steps down) and their chroma; the frame's two
// tables go into LDS once per workgroup (1 KB at 8 bit, 4 KB at 10), as 32-bit words.  A thread reads its samples with the wide ldn, looks every one up
// and stores them with the wide stn, each with its element-wise fallback; it stores only what it alone has read, so dst == src is legal.  Nothing
// assumes a monotone table.
#include "sn_yuv_color.h"

namespace {

template <int ESZ> struct CodeHistK {
    static constexpr int CODES = ESZ == 1 ? 256 : 1024;
    static constexpr int COPIES = ESZ == 1 ? 32 : 8;                      // 32 KB of LDS either way
    static constexpr int N = 16 / ESZ;                                    // samples of a unit
};

constexpr int CH_UNITS = 2048;                                            // units per workgroup (8 per lane) while the grid has room: 32 KB of samples

template <int ESZ>
__global__ __launch_bounds__(256) void yuv_code_hist_kernel(const uint8_t* __restrict__ src, uint32_t* __restrict__ dst, int w, int py, int ux, int units,
                                                          size_t origin, size_t frame_bytes) {
    using K = CodeHistK<ESZ>;
    constexpr int CODES = K::CODES, COPIES = K::COPIES, N = K::N;
    __shared__ __attribute__((aligned(16))) uint32_t hist[CODES * COPIES];
    const int tid = threadIdx.x, t = blockIdx.y, cp = tid & (COPIES - 1);
    for (int i = tid; i < CODES * COPIES / 4; i += 256) ((uint4*)hist)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const uint8_t* y = src + (size_t)t * frame_bytes + origin;            // py: the luma row pitch; origin: the byte offset of the picture's first sample
    for (int u = blockIdx.x * 256 + tid; u < units; u += gridDim.x * 256) {
        const int row = u / ux, x0 = (u - row * ux) * N;
        const int n = imin(N, w - x0);                                    // 1 .. N samples of this row exist from x0 on
        const size_t o = (size_t)row * py + x0;
        int v[N];
        if (n == N) ldn<ESZ, N>(y, o, v);
        else {
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = k < n ? ld1<ESZ>(y, o + k) : 0;
        }
        int code = imin(v[0], CODES - 1);                                 // the index is min(code, L - 1) before any use
        uint32_t run = 1;
#pragma unroll
        for (int k = 1; k < N; ++k) {
            if (k < n) {
                const int c = imin(v[k], CODES - 1);
                if (c == code) ++run;
                else {
                    atomicAdd(&hist[code * COPIES + cp], run);
                    code = c;
                    run = 1;
                }
            }
        }
        atomicAdd(&hist[code * COPIES + cp], run);
    }
    __syncthreads();
    uint32_t* out = dst + (size_t)t * CODES;
    for (int i = tid; i < CODES; i += 256) {
        const uint32_t* c = hist + i * COPIES;
        const int rot = (i * COPIES) >> 5;                                // consecutive bins start on different copies: the lanes of a group read different banks
        uint32_t s = 0;
#pragma unroll 8
        for (int k = 0; k < COPIES; ++k) s += c[(k + rot) & (COPIES - 1)];
        if (s) atomicAdd(&out[i], s);
    }
}

constexpr int LUT_TW = 256, LUT_TH = 64, LUT_STEPS = LUT_TH / 16;          // a workgroup's tile in luma samples; 16 rows a step

template <int ESZ, int CH>
__global__ __launch_bounds__(256) void yuv_apply_lut_kernel(const uint8_t* src, uint8_t* dstp, const uint16_t* __restrict__ lut, const YuvGeo G) {
    constexpr int CODES = ESZ == 1 ? 256 : 1024;
    constexpr int CNX = CH == SN_YUV_444 ? 8 : 4, CNY = CH == SN_YUV_444 ? 2 : 1;      // a thread's chroma samples
    __shared__ __attribute__((aligned(4))) uint16_t tab[2 * CODES];       // Y, then Cb and Cr
    const int tid = threadIdx.y * 32 + threadIdx.x, t = blockIdx.z;
    const uint32_t* lt = (const uint32_t*)(lut + (size_t)t * 2 * CODES);   // 4-byte aligned: the entry point has checked lut, and 2 * CODES is even
    for (int i = tid; i < CODES; i += 256) ((uint32_t*)tab)[i] = lt[i];
    __syncthreads();
    const uint16_t* ty = tab;
    const uint16_t* tc = tab + CODES;
    const int H = G.h, W = G.w, py = G.py, pc = G.pc;
    const int cw = CH == SN_YUV_444 ? W : (W + 1) >> 1, ch = CH == SN_YUV_444 ? H : (H + 1) >> 1;
    const uint8_t* ibase = src + (size_t)t * G.frame_bytes;
    uint8_t* obase = dstp + (size_t)t * G.frame_bytes;
    const int x0 = blockIdx.x * LUT_TW + threadIdx.x * 8;
    if (x0 >= W) return;                                                  // behind the only barrier
    const int cx0 = CH == SN_YUV_444 ? x0 : x0 >> 1;
    const int n = imin(8, W - x0), ncx = imin(CNX, cw - cx0);
    const bool inner = n == 8, cinner = ncx == CNX;
#pragma unroll 1
    for (int step = 0; step < LUT_STEPS; ++step) {
        const int y0 = blockIdx.y * LUT_TH + step * 16 + threadIdx.y * 2;
        if (y0 >= H) return;
        const int cy0 = CH == SN_YUV_444 ? y0 : y0 >> 1;
        // ---- everything the thread reads from memory, before anything is stored
        int Y[2][8], Cq[2][CNY][CNX];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int k = 0; k < 8; ++k) Y[r][k] = 0;
            if (y0 + r >= H) break;
            const size_t o = (size_t)(y0 + r) * py + x0;
            if (inner) ldn<ESZ, 8>(ibase + G.oy, o, Y[r]); else for (int k = 0; k < n; ++k) Y[r][k] = ld1<ESZ>(ibase + G.oy, o + k);
        }
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const uint8_t* cp = ibase + (pl ? G.ov : G.ou);
#pragma unroll
            for (int r = 0; r < CNY; ++r) {
#pragma unroll
                for (int k = 0; k < CNX; ++k) Cq[pl][r][k] = 0;
                if (cy0 + r >= ch) break;
                const size_t o = (size_t)(cy0 + r) * pc + cx0;
                if (cinner) ldn<ESZ, CNX>(cp, o, Cq[pl][r]); else for (int k = 0; k < ncx; ++k) Cq[pl][r][k] = ld1<ESZ>(cp, o + k);
            }
        }
        // ---- the lookups: the index is min(code, L - 1) before any use
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 8; ++k) Y[r][k] = ty[imin(Y[r][k], CODES - 1)];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int r = 0; r < CNY; ++r)
#pragma unroll
                for (int k = 0; k < CNX; ++k) Cq[pl][r][k] = tc[imin(Cq[pl][r][k], CODES - 1)];
        // ---- the stores: wide where the address allows
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (y0 + r >= H) break;
            const size_t o = (size_t)(y0 + r) * py + x0;
            if (inner) stn<ESZ, 8>(obase + G.oy, o, Y[r]); else for (int k = 0; k < n; ++k) st1<ESZ>(obase + G.oy, o + k, Y[r][k]);
        }
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            uint8_t* cp = obase + (pl ? G.ov : G.ou);
#pragma unroll
            for (int r = 0; r < CNY; ++r) {
                if (cy0 + r >= ch) break;
                const size_t o = (size_t)(cy0 + r) * pc + cx0;
                if (cinner) stn<ESZ, CNX>(cp, o, Cq[pl][r]); else for (int k = 0; k < ncx; ++k) st1<ESZ>(cp, o + k, Cq[pl][r][k]);
            }
        }
    }
}

}  // namespace

extern "C" {

int sn_yuv_code_hist(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, uint32_t* dst, int T, int H, int W, void* stream) {
    sn_clear_error();
    YuvK K;
    YuvGeo G;
    if (!valid_payloads(src, fmt, T, H, W) || !make_consts(fmt, &K)) return SN_EINVAL;
    if (!dst || ((uintptr_t)dst & 3) || !make_geo(fmt, H, W, rect, &G)) return SN_EINVAL;
    if ((long long)G.h * G.w > 0xFFFFFFFFLL) return SN_EINVAL;             // a count is 32 bits, and a flat frame puts every sample into one
    const int codes = 1 << fmt->bits, n = fmt->bits == 8 ? 16 : 8;
    const int ux = (G.w + n - 1) / n;
    const long long units = (long long)ux * G.h;
    if (units > 0x7fffffffLL - 1024 * 256) return SN_EINVAL;               // a unit's index, and the walk's last step, are ints
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(dst, 0, (size_t)T * codes * sizeof(uint32_t), s) != hipSuccess) return sn_check_launch();      // dst is overwritten, not added to
    const long long wgs = (units + CH_UNITS - 1) / CH_UNITS;
    const dim3 block(256), grid(wgs < 1024 ? (int)wgs : 1024, T);
    with_esz(fmt, [&](auto esz) {
        hipLaunchKernelGGL((yuv_code_hist_kernel<esz()>), grid, block, 0, s, src, dst, G.w, G.py, ux, (int)units, G.oy, G.frame_bytes);
    });
    return sn_check_launch();
}

int sn_yuv_apply_lut(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const uint16_t* lut, uint8_t* dst, int T, int H, int W,
                     void* stream) {
    sn_clear_error();
    YuvK K;
    YuvGeo G;
    if (!valid_payloads(dst, fmt, T, H, W) || !src || !aligned_payload(fmt, src) || !make_consts(fmt, &K)) return SN_EINVAL;
    if (!lut || ((uintptr_t)lut & 3) || !make_geo(fmt, H, W, rect, &G)) return SN_EINVAL;
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    const size_t bytes = (size_t)T * G.frame_bytes;
    if (a != b && a < b + bytes && b < a + bytes) return SN_EINVAL;       // in place, or apart: a thread stores only what it alone has read
    const dim3 block(32, 8), grid((G.w + LUT_TW - 1) / LUT_TW, (G.h + LUT_TH - 1) / LUT_TH, T);
    if (grid.y > 65535) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    with_esz_chroma(fmt, [&](auto esz, auto ch) { hipLaunchKernelGGL((yuv_apply_lut_kernel<esz(), ch()>), grid, block, 0, s, src, dst, lut, G); });
    return sn_check_launch();
}

}  // extern "C"
