// Noise added to a clean stream on the device (gfx950), for the experiment `restore_video --add_noise` makes: planar Y'CbCr payloads in, planar
// Y'CbCr payloads of the same format out, whole frames.
//
//   sn_yuv_degrade : T payloads -> T payloads: per pixel the ingest of sn_ingest_yuv (float32, not rounded to a module dtype), plus Gaussian noise on
//                    R', G' and B' whose sigma is a 16-knot curve at the pixel's own clean luma code, then the egress of sn_egress_yuv.
//
// The three steps are composed in registers: no float frame reaches memory.  The arithmetic (order of operations, constants) is stated in
// include/shiftnet_hip.h and restated in float32 by tests/degrade_ref.py, which the kernel equals bit for bit; every float product and sum is rounded
// separately (contraction is off for this file: no FMA).  The two ends are the arithmetic of csrc/sn_yuv.hip through csrc/sn_yuv_color.h.
//
// The noise of a sample is a table lookup, gauss[hash >> 16], of a counter-based hash of (seed, frame, channel, row, column): a pure function of the
// sample's position in the stream.  That is what lets a thread recompute the pixel left of its span, which the left-sited 4:2:0 filter reads and a
// neighbouring thread owns, and what makes the bytes the same for every launch geometry and every way of cutting the stream into launches.
//
// A bandwidth kernel with a gather: 1.5 B per pixel in and out at 8-bit 4:2:0, and three 4 B reads per pixel at random places of the 256 KB table,
// which stays in L2.  The thread geometry is that of the two edge kernels: a thread owns four horizontally adjacent 2x2 luma blocks (8 x 2 pixels),
// the 8 pixels of a row are one 8 / 16 B load and one store where the address is aligned; a thread whose span is not aligned or touches the frame
// edge takes the element-wise path with the same arithmetic.
#include "sn_yuv_color.h"
#pragma clang fp contract(off)

namespace {

struct DegradeK {
    float k[SN_NLF_BANDS];          // the curve, already divided by 255
    float lo, scale;                // the black luma code, 16 / (white - black)
    uint32_t seed, t0;
};

// The noisy pixel (ye, xe) of the frame with key fk: Y, un, vn are its luma code and chroma numerators.  kn: the knots in LDS.
template <int CH>
__device__ __forceinline__ void noisy_rgb(const YuvK& K, const float* kn, float lo, float scale, const float* __restrict__ gauss, uint32_t fk, int ye, int xe,
                                          int Y, int un, int vn, float* r, float* g, float* b) {
    float R, G, B;
    yuv_to_rgb<CH>(K, Y, un, vn, &R, &G, &B);
    // the curve at the clean luma code: sn_noise_map_level's interpolation
    const float u = fminf(fmaxf(subr(mulr(subr((float)Y, lo), scale), 0.5f), 0.f), 15.f);
    const int i = imin((int)u, SN_NLF_BANDS - 2);                          // u >= 0: the conversion is the floor
    const float f = subr(u, (float)i);
    const float s = addr(kn[i], mulr(f, subr(kn[i + 1], kn[i])));
    *r = addr(R, mulr(s, gauss[hash_sample(dither_row_key(fk, 3, ye), xe) >> 16]));
    *g = addr(G, mulr(s, gauss[hash_sample(dither_row_key(fk, 4, ye), xe) >> 16]));
    *b = addr(B, mulr(s, gauss[hash_sample(dither_row_key(fk, 5, ye), xe) >> 16]));
}

template <int ESZ, int CH>
__global__ __launch_bounds__(256) void degrade_yuv_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dstp, const float* __restrict__ gauss,
                                                        const YuvK K, const DegradeK N, const YuvGeo G) {
    __shared__ float kn[SN_NLF_BANDS];                                     // the per-pixel lookup is an LDS read and not private memory
    const int tid = threadIdx.y * 32 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < SN_NLF_BANDS; ++j) if (tid == j) kn[j] = N.k[j];
    __syncthreads();
    const int t = blockIdx.z;
    const int x0 = (blockIdx.x * 32 + threadIdx.x) * 8, y0 = (blockIdx.y * 8 + threadIdx.y) * 2;
    const int H = G.h, W = G.w, py = G.py, pc = G.pc;
    if (x0 >= W || y0 >= H) return;
    const int cw = CH == SN_YUV_444 ? W : (W + 1) >> 1, ch = CH == SN_YUV_444 ? H : (H + 1) >> 1;
    const uint8_t* ibase = src + (size_t)t * G.frame_bytes;
    const uint8_t* iyp = ibase + G.oy;
    const uint8_t* iup = ibase + G.ou;
    const uint8_t* ivp = ibase + G.ov;
    const uint32_t fk = hash_frame_key(N.seed, N.t0 + (uint32_t)t);
    const bool inner = x0 + 8 <= W;
    // R', G', B' of pixels x0 - 1 .. x0 + 7 (index 0 .. 8) of rows y0, y0 + 1, coordinates clamped to the H x W frame: a clamped pixel is the frame's
    // pixel at the clamped place, noise included
    float c[3][2][9];
    const bool interior = inner && y0 + 2 <= H;
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
                for (int k = 0; k < 8; ++k)
                    noisy_rgb<CH>(K, kn, N.lo, N.scale, gauss, fk, y0 + r, x0 + k, Y[r][k], U[k], V[k], &c[0][r][1 + k], &c[1][r][1 + k], &c[2][r][1 + k]);
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
                for (int k = 0; k < 8; ++k)
                    noisy_rgb<CH>(K, kn, N.lo, N.scale, gauss, fk, y0 + r, x0 + k, Y[r][k], num[0][r][k], num[1][r][k], &c[0][r][1 + k], &c[1][r][1 + k],
                                  &c[2][r][1 + k]);
        }
    }
    // element-wise: index k of row r, pixel (min(y0 + r, H - 1), clamp(x0 + k - 1, 0, W - 1))
    const auto element = [&](int r, int k) {
        const int ye = imin(y0 + r, H - 1), xe = imin(imax(x0 + k - 1, 0), W - 1);
        const int y = ld1<ESZ>(iyp, (size_t)ye * py + xe);
        int un, vn;
        if (CH == SN_YUV_444) { un = ld1<ESZ>(iup, (size_t)ye * pc + xe); vn = ld1<ESZ>(ivp, (size_t)ye * pc + xe); }
        else { un = chroma_num<ESZ, CH>(iup, pc, cw, ch, ye, xe); vn = chroma_num<ESZ, CH>(ivp, pc, cw, ch, ye, xe); }
        noisy_rgb<CH>(K, kn, N.lo, N.scale, gauss, fk, ye, xe, y, un, vn, &c[0][r][k], &c[1][r][k], &c[2][r][k]);
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
    // ---- the egress of sn_egress_yuv on those values -------------------------------------------------------------------------------------------
    uint8_t* base = dstp + (size_t)t * G.frame_bytes;
    uint8_t* yp = base + G.oy;
    uint8_t* up = base + G.ou;
    uint8_t* vp = base + G.ov;
    float yv[2][9], cb[2][9], cr[2][9];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = CH == SN_YUV_420_LEFT ? 0 : 1; k < 9; ++k) {
            const float R = clamp01(c[0][r][k]), Gn = clamp01(c[1][r][k]), B = clamp01(c[2][r][k]);
            const float y = addr(addr(mulr(K.kr, R), mulr(K.kg, Gn)), mulr(K.kb, B));
            yv[r][k] = y;
            cb[r][k] = mulr(subr(B, y), K.cu);
            cr[r][k] = mulr(subr(R, y), K.cv);
        }
    const int n = imin(8, W - x0);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (y0 + r >= H) break;
        int q[8];
        const size_t o = (size_t)(y0 + r) * py + x0, oc = (size_t)(y0 + r) * pc + x0;
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = quant(K.yo, K.ys, yv[r][1 + k], K.ylo, K.yhi);
        if (inner) stn<ESZ, 8>(yp, o, q); else for (int k = 0; k < n; ++k) st1<ESZ>(yp, o + k, q[k]);
        if (CH == SN_YUV_444) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
                for (int k = 0; k < 8; ++k) q[k] = quant(K.co, K.cs, pl ? cr[r][1 + k] : cb[r][1 + k], K.clo, K.chi);
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

int sn_yuv_degrade(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_degrade_noise* noise, const float* gauss, uint8_t* dst, int T, int H, int W,
                   void* stream) {
    sn_clear_error();
    YuvK K;
    YuvGeo G;
    if (!valid_payloads(dst, fmt, T, H, W) || !src || !aligned_payload(fmt, src) || !make_consts(fmt, &K)) return SN_EINVAL;
    if (!noise || !gauss || ((uintptr_t)gauss & 3) || noise->t0 < 0 || !make_geo(fmt, H, W, nullptr, &G)) return SN_EINVAL;
    DegradeK N;
    for (int i = 0; i < SN_NLF_BANDS; ++i) {
        const float k = noise->knots[i];
        if (!(k >= 0.f) || k - k != 0.f) return SN_EINVAL;                  // negative, NaN, infinity
        N.k[i] = (float)((double)k / 255.0);                               // a float64 expression rounded once, as the constants of make_consts
    }
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    const size_t bytes = (size_t)T * G.frame_bytes;
    if (a < b + bytes && b < a + bytes) return SN_EINVAL;                 // the kernel reads neighbours in src while other lanes write dst
    N.lo = (float)K.ylo;                                                  // the curve's knots sit between the format's black and white luma codes
    N.scale = (float)(16.0 / ((double)K.yhi - (double)K.ylo));
    N.seed = noise->seed; N.t0 = (uint32_t)noise->t0;
    const dim3 block(32, 8), grid(((W + 7) / 8 + 31) / 32, ((H + 1) / 2 + 7) / 8, T);
    if (grid.y > 65535) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    with_esz_chroma(fmt, [&](auto esz, auto ch) {
        hipLaunchKernelGGL((degrade_yuv_kernel<esz(), ch()>), grid, block, 0, s, src, dst, gauss, K, N, G);
    });
    return sn_check_launch();
}

}  // extern "C"
