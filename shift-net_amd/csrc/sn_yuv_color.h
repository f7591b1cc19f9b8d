// The colour arithmetic that the units converting between planar Y'CbCr payloads and R'G'B' share: csrc/sn_yuv.hip (the colour edges) and
// csrc/sn_degrade.hip (both edges composed around added noise).  The constants of a format, a pixel's way in (chroma numerators, matrix, clamp),
// the rounding of a value to a code, and the integer hash that keys the dither and the noise.  The arithmetic is stated in include/shiftnet_hip.h.
//
// Contraction stays off (sn_yuv.h): every float product and sum below is rounded separately.
#pragma once
#include "sn_yuv.h"
#pragma clang fp contract(off)

namespace {

struct YuvK {
    // ingest: R = ky*(Y - yoff) + crv*(V - coff), G = (ky*(Y - yoff) + cgu*(U - coff)) + cgv*(V - coff), B = ky*(Y - yoff) + cbu*(U - coff)
    float ky, crv, cgu, cgv, cbu;
    // egress: Y' = (kr*R + kg*G) + kb*B, Cb = (B - Y')*cu, Cr = (R - Y')*cv; code = rint(off + scale * value)
    float kr, kg, kb, cu, cv, ys, yo, cs, co;
    int yoff, coff, ylo, yhi, clo, chi;
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// ---- ingest -------------------------------------------------------------------------------------------------------------------
// CH: SN_YUV_444 / SN_YUV_420_CENTER / SN_YUV_420_LEFT.  Chroma reaches the matrix as an integer numerator over DEN (1 / 16 / 8):
//   centre: (3 * (3 * C[j][i] + C[jn][i]) + (3 * C[j][in] + C[jn][in])) / 16 with (j, i) = (y >> 1, x >> 1) and jn / in the neighbour
//           on the side of the luma sample (odd: +1, even: -1), clamped to the plane;
//   left:   v(c) = 3 * C[j][c] + C[jn][c]; even x: 2 * v(i) / 8, odd x: (v(i) + v(min(i + 1, cw - 1))) / 8.
template <int CH> struct Den { static constexpr int value = CH == SN_YUV_444 ? 1 : (CH == SN_YUV_420_CENTER ? 16 : 8); };

template <int CH> __device__ __forceinline__ void yuv_to_rgb(const YuvK& K, int y, int un, int vn, float* r, float* g, float* b) {
    constexpr float inv = 1.0f / Den<CH>::value;
    const float yd = (float)(y - K.yoff);
    const float ud = mulr((float)(un - Den<CH>::value * K.coff), inv);        // exact: a power of two times an integer < 2^15
    const float vd = mulr((float)(vn - Den<CH>::value * K.coff), inv);
    const float yy = mulr(K.ky, yd);
    *r = clamp01(addr(yy, mulr(K.crv, vd)));
    *g = clamp01(addr(addr(yy, mulr(K.cgu, ud)), mulr(K.cgv, vd)));
    *b = clamp01(addr(yy, mulr(K.cbu, ud)));
}

template <int ESZ, int CH> __device__ __forceinline__ int chroma_num(const uint8_t* p, int pc, int cw, int ch, int ye, int xe) {
    const int j = ye >> 1, i = xe >> 1;
    const int jn = imin(imax(j + ((ye & 1) ? 1 : -1), 0), ch - 1);
    const size_t rj = (size_t)j * pc, rn = (size_t)jn * pc;
    if (CH == SN_YUV_420_CENTER) {
        const int in = imin(imax(i + ((xe & 1) ? 1 : -1), 0), cw - 1);
        return 3 * (3 * ld1<ESZ>(p, rj + i) + ld1<ESZ>(p, rn + i)) + (3 * ld1<ESZ>(p, rj + in) + ld1<ESZ>(p, rn + in));
    }
    const int v0 = 3 * ld1<ESZ>(p, rj + i) + ld1<ESZ>(p, rn + i);
    if (!(xe & 1)) return 2 * v0;
    const int i1 = imin(i + 1, cw - 1);
    return v0 + (3 * ld1<ESZ>(p, rj + i1) + ld1<ESZ>(p, rn + i1));
}

// ---- egress -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int quant(float off, float scale, float v, int lo, int hi) {
    return imin(imax(__float2int_rn(addr(off, mulr(scale, v))), lo), hi);
}

// ---- the hash of the dither and of the added noise -----------------------------------------------------------------------------------
// key = (y * 0x9E3779B1) ^ (x * 0x85EBCA77) ^ (frame * 0xC2B2AE3D) ^ (plane * 0x27D4EB2F) ^ seed, then the murmur3 finaliser (uint32 arithmetic wraps).
// The dither of the egress uses planes 0 .. 2 (Y, Cb, Cr), the noise of sn_yuv_degrade planes 3 .. 5 (R', G', B') of the same seed space.
__device__ __forceinline__ uint32_t hash_frame_key(uint32_t seed, uint32_t frame) { return (frame * 0xC2B2AE3Du) ^ seed; }
// plane p, row y of the plane: the part of the key that a row of samples shares
__device__ __forceinline__ uint32_t dither_row_key(uint32_t fk, int p, int y) { return fk ^ ((uint32_t)p * 0x27D4EB2Fu) ^ ((uint32_t)y * 0x9E3779B1u); }
// the sample at column x of that row
__device__ __forceinline__ uint32_t hash_sample(uint32_t rk, int x) {
    uint32_t k = rk ^ ((uint32_t)x * 0x85EBCA77u);
    k ^= k >> 16; k *= 0x85EBCA6Bu; k ^= k >> 13; k *= 0xC2B2AE35u; k ^= k >> 16;
    return k;
}

// constants: float64 expressions rounded once to float32 (tests/yuv_ref.py: constants() evaluates the same expressions)
inline bool make_consts(const sn_yuv_fmt* f, YuvK* K) {
    if (!valid_fmt(f) || f->matrix < 0 || f->matrix > 1 || f->range < 0 || f->range > 1) return false;
    const double kr = f->matrix == SN_YUV_BT709 ? 0.2126 : 0.299, kb = f->matrix == SN_YUV_BT709 ? 0.0722 : 0.114;
    const double kg = 1.0 - kr - kb;
    const int s = 1 << (f->bits - 8), top = (1 << f->bits) - 1;
    const bool full = f->range == SN_YUV_FULL;
    const double yo = full ? 0.0 : 16.0 * s, ys = full ? (double)top : 219.0 * s, cs = full ? (double)top : 224.0 * s, co = 128.0 * s;
    K->ky = (float)(1.0 / ys);
    K->crv = (float)(2.0 * (1.0 - kr) / cs);
    K->cgu = (float)(-2.0 * kb * (1.0 - kb) / kg / cs);
    K->cgv = (float)(-2.0 * kr * (1.0 - kr) / kg / cs);
    K->cbu = (float)(2.0 * (1.0 - kb) / cs);
    K->kr = (float)kr; K->kg = (float)kg; K->kb = (float)kb;
    K->cu = (float)(1.0 / (2.0 * (1.0 - kb)));
    K->cv = (float)(1.0 / (2.0 * (1.0 - kr)));
    K->ys = (float)ys; K->yo = (float)yo; K->cs = (float)cs; K->co = (float)co;
    K->yoff = (int)yo; K->coff = (int)co;
    K->ylo = full ? 0 : 16 * s; K->yhi = full ? top : 235 * s; K->clo = full ? 0 : 16 * s; K->chi = full ? top : 240 * s;
    return true;
}

}  // namespace
