// Motion blur of a sharp stream on the device (gfx950), for the experiment `restore_video --add_blur` makes: planar Y'CbCr payloads in, planar
// Y'CbCr payloads of the same format out, whole frames.
//
//   sn_yuv_blur : S source payloads -> T payloads: output t is the mean of n consecutive source frames around frame c0 + t, indices clamped to
//                 [lo, hi] (the frame's scene), taken on sn_ingest_yuv's float32 R', G', B' -- through a gamma table into linear light and back
//                 when tables are given -- then the egress of sn_egress_yuv.  How the deblur datasets (GOPRO, DVD) are made.
//
// The steps are composed in registers: no float frame reaches memory.  The arithmetic (order of operations, constants) is stated in
// include/shiftnet_hip.h and restated in float32 by tests/blur_ref.py, which the kernel equals bit for bit; every float product and sum is rounded
// separately (contraction is off for this file: no FMA), and there is no division, powf or exp2f.  The two ends are the arithmetic of csrc/sn_yuv.hip
// through csrc/sn_yuv_color.h.
//
// A bandwidth kernel with a table: n frames read per frame written (consecutive outputs share n - 1 of them, which the caches may or may not
// serve), and with tables one interpolated read per channel and tap on the way in and a 12-step search per channel on the way out.  Both tables
// (4096 + 4095 float32, 32 KB) are copied into LDS by every workgroup.  The thread geometry is that of the two edge kernels: a thread owns four
// horizontally adjacent 2x2 luma blocks (8 x 2 pixels), the 8 pixels of a row are one 8 / 16 B load and one store where the address is aligned; a
// thread whose span is not aligned or touches the frame edge takes the element-wise path with the same arithmetic.  blockIdx.z is the output frame.
#include "sn_yuv_color.h"
#pragma clang fp contract(off)

namespace {

constexpr int LIN = 4096;                                   // lin[0 .. 4095], then rinv[0 .. 4094]

struct BlurK {
    int n, c0, lo, hi;
    float inv_n, k;                                         // 1 / n and 1 / 4095, float64 quotients rounded once
};

// R', G' or B' in [0, 1] -> linear light
template <bool TAB> __device__ __forceinline__ float decode(const float* lin, float v) {
    if (!TAB) return v;
    const float u = mulr(v, 4095.0f);
    const int i = imin((int)u, LIN - 2);                    // u >= 0: the conversion is the floor
    const float e = subr(u, (float)i);
    return addr(lin[i], mulr(e, subr(lin[i + 1], lin[i])));
}

// the mean in linear light -> R', G' or B'
template <bool TAB> __device__ __forceinline__ float encode(const float* lin, float k, float m) {
    if (!TAB) return m;
    int i = 0;                                              // the largest index in 0 .. 4094 with lin[i] <= m; lin[0] = 0 <= m
#pragma unroll
    for (int s = LIN / 2; s >= 1; s >>= 1) {
        const int c = i + s;
        if (c <= LIN - 2 && lin[c] <= m) i = c;
    }
    const float e = fminf(mulr(subr(m, lin[i]), lin[LIN + i]), 1.0f);
    return mulr(addr((float)i, e), k);
}

// R', G', B' (sn_ingest_yuv's, clamped to [0, 1]) of pixels x0 - 1 .. x0 + 7 (index 0 .. 8) of rows y0, y0 + 1 of one frame, coordinates clamped to the
// H x W frame: put(row, index, R, G, B) for index 1 .. 8, and for index 0 where the left-sited 4:2:0 filter reads it.  The loads of sn_yuv_degrade.
template <int ESZ, int CH, typename F>
__device__ __forceinline__ void span_rgb(const YuvK& K, const YuvGeo& G, const uint8_t* frame, int x0, int y0, bool interior, F&& put) {
    const int H = G.h, W = G.w, py = G.py, pc = G.pc;
    const int cw = CH == SN_YUV_444 ? W : (W + 1) >> 1, ch = CH == SN_YUV_444 ? H : (H + 1) >> 1;
    const uint8_t* iyp = frame + G.oy;
    const uint8_t* iup = frame + G.ou;
    const uint8_t* ivp = frame + G.ov;
    if (interior) {                                        // whole blocks, wide loads (sn_ingest_yuv's interior path)
        int Y[2][8];
#pragma unroll
        for (int r = 0; r < 2; ++r) ldn<ESZ, 8>(iyp, (size_t)(y0 + r) * py + x0, Y[r]);
        if (CH == SN_YUV_444) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                int U[8], V[8];
                ldn<ESZ, 8>(iup, (size_t)(y0 + r) * pc + x0, U);
                ldn<ESZ, 8>(ivp, (size_t)(y0 + r) * pc + x0, V);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float R, Gn, B;
                    yuv_to_rgb<CH>(K, Y[r][k], U[k], V[k], &R, &Gn, &B);
                    put(r, 1 + k, R, Gn, B);
                }
            }
        } else {
            const int j = y0 >> 1, c0 = x0 >> 1;
            const int jr[3] = {imax(j - 1, 0), j, imin(j + 1, ch - 1)};
            int num[2][2][8];                               // [plane][row][pixel]
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const uint8_t* cp = pl ? ivp : iup;
                int win[3][6];                              // chroma columns c0 - 1 .. c0 + 4 (clamped) of rows j - 1, j, j + 1 (clamped)
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const size_t row = (size_t)jr[q] * pc;
                    ldn<ESZ, 4>(cp, row + c0, &win[q][1]);
                    win[q][0] = CH == SN_YUV_420_CENTER ? ld1<ESZ>(cp, row + imax(c0 - 1, 0)) : 0;
                    win[q][5] = ld1<ESZ>(cp, row + imin(c0 + 4, cw - 1));
                }
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    int vr[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) vr[k] = 3 * win[1][k] + win[r ? 2 : 0][k];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int i = k >> 1;
                        if (CH == SN_YUV_420_CENTER) num[pl][r][k] = 3 * vr[i + 1] + vr[(k & 1) ? i + 2 : i];
                        else num[pl][r][k] = (k & 1) ? vr[i + 1] + vr[i + 2] : 2 * vr[i + 1];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float R, Gn, B;
                    yuv_to_rgb<CH>(K, Y[r][k], num[0][r][k], num[1][r][k], &R, &Gn, &B);
                    put(r, 1 + k, R, Gn, B);
                }
        }
    }
    // element-wise: index k of row r, pixel (min(y0 + r, H - 1), clamp(x0 + k - 1, 0, W - 1))
    const auto element = [&](int r, int k) {
        const int ye = imin(y0 + r, H - 1), xe = imin(imax(x0 + k - 1, 0), W - 1);
        const int y = ld1<ESZ>(iyp, (size_t)ye * py + xe);
        int un, vn;
        if (CH == SN_YUV_444) { un = ld1<ESZ>(iup, (size_t)ye * pc + xe); vn = ld1<ESZ>(ivp, (size_t)ye * pc + xe); }
        else { un = chroma_num<ESZ, CH>(iup, pc, cw, ch, ye, xe); vn = chroma_num<ESZ, CH>(ivp, pc, cw, ch, ye, xe); }
        float R, Gn, B;
        yuv_to_rgb<CH>(K, y, un, vn, &R, &Gn, &B);
        put(r, k, R, Gn, B);
    };
    if (!interior) {                                       // the frame edge: the span pixel by pixel
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 1; k < 9; ++k) element(r, k);
    }
    if (CH == SN_YUV_420_LEFT) {                           // the pixel left of the span, which the left-sited filter reads and the neighbouring thread owns
#pragma unroll
        for (int r = 0; r < 2; ++r) element(r, 0);
    }
}

template <int ESZ, int CH, bool TAB>
__global__ __launch_bounds__(256) void blur_yuv_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dstp, const float* __restrict__ lin_g,
                                                     const float* __restrict__ rinv_g, const YuvK K, const BlurK B, const YuvGeo G) {
    __shared__ float lin[TAB ? 2 * LIN - 1 : 1];
    if (TAB) {
        const int tid = threadIdx.y * 32 + threadIdx.x;
        for (int i = tid; i < LIN; i += 256) lin[i] = lin_g[i];
        for (int i = tid; i < LIN - 1; i += 256) lin[LIN + i] = rinv_g[i];
        __syncthreads();
    }
    const int t = blockIdx.z;
    const int x0 = (blockIdx.x * 32 + threadIdx.x) * 8, y0 = (blockIdx.y * 8 + threadIdx.y) * 2;
    const int H = G.h, W = G.w, py = G.py, pc = G.pc;
    if (x0 >= W || y0 >= H) return;
    const int cw = CH == SN_YUV_444 ? W : (W + 1) >> 1;
    const bool inner = x0 + 8 <= W;
    const bool interior = inner && y0 + 2 <= H;
    // the sums over the taps, in linear light: acc = v(-r), then acc = acc + v(j) in ascending j
    float acc[3][2][9];
#pragma unroll
    for (int i = 0; i < 54; ++i) (&acc[0][0][0])[i] = 0.f;
    const int r = B.n >> 1;
    for (int j = -r; j <= r; ++j) {
        const long long want = (long long)B.c0 + t + j;    // clamped to [lo, hi], which the host has checked against the S source payloads
        const int f = want < B.lo ? B.lo : (want > B.hi ? B.hi : (int)want);
        const bool first = j == -r;
        span_rgb<ESZ, CH>(K, G, src + (size_t)f * G.frame_bytes, x0, y0, interior, [&](int row, int k, float R, float Gn, float Bl) {
            const float v0 = decode<TAB>(lin, R), v1 = decode<TAB>(lin, Gn), v2 = decode<TAB>(lin, Bl);
            acc[0][row][k] = first ? v0 : addr(acc[0][row][k], v0);
            acc[1][row][k] = first ? v1 : addr(acc[1][row][k], v1);
            acc[2][row][k] = first ? v2 : addr(acc[2][row][k], v2);
        });
    }
    // ---- the egress of sn_egress_yuv on the encoded means --------------------------------------------------------------------------------------
    uint8_t* base = dstp + (size_t)t * G.frame_bytes;
    uint8_t* yp = base + G.oy;
    uint8_t* up = base + G.ou;
    uint8_t* vp = base + G.ov;
    float yv[2][9], cb[2][9], cr[2][9];
#pragma unroll
    for (int row = 0; row < 2; ++row)
#pragma unroll
        for (int k = CH == SN_YUV_420_LEFT ? 0 : 1; k < 9; ++k) {
            const float R = clamp01(encode<TAB>(lin, B.k, mulr(acc[0][row][k], B.inv_n)));
            const float Gn = clamp01(encode<TAB>(lin, B.k, mulr(acc[1][row][k], B.inv_n)));
            const float Bl = clamp01(encode<TAB>(lin, B.k, mulr(acc[2][row][k], B.inv_n)));
            const float y = addr(addr(mulr(K.kr, R), mulr(K.kg, Gn)), mulr(K.kb, Bl));
            yv[row][k] = y;
            cb[row][k] = mulr(subr(Bl, y), K.cu);
            cr[row][k] = mulr(subr(R, y), K.cv);
        }
    const int n = imin(8, W - x0);
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        if (y0 + row >= H) break;
        int q[8];
        const size_t o = (size_t)(y0 + row) * py + x0, oc = (size_t)(y0 + row) * pc + x0;
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = quant(K.yo, K.ys, yv[row][1 + k], K.ylo, K.yhi);
        if (inner) stn<ESZ, 8>(yp, o, q); else for (int k = 0; k < n; ++k) st1<ESZ>(yp, o + k, q[k]);
        if (CH == SN_YUV_444) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
                for (int k = 0; k < 8; ++k) q[k] = quant(K.co, K.cs, pl ? cr[row][1 + k] : cb[row][1 + k], K.clo, K.chi);
                if (inner) stn<ESZ, 8>(pl ? vp : up, oc, q); else for (int k = 0; k < n; ++k) st1<ESZ>(pl ? vp : up, oc + k, q[k]);
            }
        }
    }
    if (CH != SN_YUV_444) {
        const int c0 = x0 >> 1, nc = imin(4, cw - c0);
        const size_t o = (size_t)(y0 >> 1) * pc + c0;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            int q[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* a = pl ? cr[0] : cb[0];
                const float* b = pl ? cr[1] : cb[1];
                float m;
                if (CH == SN_YUV_420_CENTER)       // mean of the 2x2 block: ((a0 + a1) + (b0 + b1)) / 4
                    m = mulr(0.25f, addr(addr(a[1 + 2 * i], a[2 + 2 * i]), addr(b[1 + 2 * i], b[2 + 2 * i])));
                else                               // (1,2,1)/4 along x centred on the even pixel, (1,1)/2 along y: (((l + 2c) + r)_a + ((l + 2c) + r)_b) / 8
                    m = mulr(0.125f, addr(addr(addr(a[2 * i], mulr(2.f, a[1 + 2 * i])), a[2 + 2 * i]),
                                                    addr(addr(b[2 * i], mulr(2.f, b[1 + 2 * i])), b[2 + 2 * i])));
                q[i] = quant(K.co, K.cs, m, K.clo, K.chi);
            }
            if (nc == 4) stn<ESZ, 4>(pl ? vp : up, o, q); else for (int i = 0; i < nc; ++i) st1<ESZ>(pl ? vp : up, o + i, q[i]);
        }
    }
}

}  // namespace

extern "C" {

int sn_yuv_blur(const uint8_t* src, int S, const sn_yuv_fmt* fmt, const sn_yuv_blur_window* win, const float* lin, const float* rinv, uint8_t* dst, int T,
                int H, int W, void* stream) {
    sn_clear_error();
    YuvK K;
    YuvGeo G;
    if (!valid_payloads(dst, fmt, T, H, W) || !src || !aligned_payload(fmt, src) || !make_consts(fmt, &K)) return SN_EINVAL;
    if (S < 1 || !win || !make_geo(fmt, H, W, nullptr, &G)) return SN_EINVAL;
    if (win->n < 1 || win->n > SN_BLUR_MAX_TAPS || !(win->n & 1)) return SN_EINVAL;
    if (win->lo < 0 || win->lo > win->hi || win->hi >= S) return SN_EINVAL;             // every clamped index is one of the S payloads
    if (win->c0 < win->lo || (long long)win->c0 + T - 1 > win->hi) return SN_EINVAL;    // every output's own frame lies in the window
    if (!lin != !rinv || ((uintptr_t)lin & 3) || ((uintptr_t)rinv & 3)) return SN_EINVAL;
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    if (a < b + (size_t)T * G.frame_bytes && b < a + (size_t)S * G.frame_bytes) return SN_EINVAL;   // other lanes read src while this one writes dst
    BlurK B;
    B.n = win->n; B.c0 = win->c0; B.lo = win->lo; B.hi = win->hi;
    B.inv_n = (float)(1.0 / (double)win->n);
    B.k = (float)(1.0 / 4095.0);
    const dim3 block(32, 8), grid(((W + 7) / 8 + 31) / 32, ((H + 1) / 2 + 7) / 8, T);
    if (grid.y > 65535) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    with_esz_chroma(fmt, [&](auto esz, auto ch) {
        if (lin) hipLaunchKernelGGL((blur_yuv_kernel<esz(), ch(), true>), grid, block, 0, s, src, dst, lin, rinv, K, B, G);
        else hipLaunchKernelGGL((blur_yuv_kernel<esz(), ch(), false>), grid, block, 0, s, src, dst, lin, rinv, K, B, G);
    });
    return sn_check_launch();
}

}  // extern "C"
