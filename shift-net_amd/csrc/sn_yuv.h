// What the two units that read planar Y'CbCr payloads share: csrc/sn_yuv.hip (the colour edges) and csrc/sn_yuv_stats.hip (the luma statistics).
// Sample loads and stores, the picture geometry of a launch, the checks every entry point makes of its format and payload arguments, and the
// dispatch that turns a format into template arguments.  A frame payload is Y4M's (include/shiftnet_hip.h).
//
// Contraction is off from here to the end of the unit that includes this file: mulr / addr / subr below, and every float expression of the kernels
// that use them, round each product and sum separately (no FMA), which the bit-for-bit tests of both units rely on.
#pragma once
#include "sn_common.h"
#include "../../include/shiftnet_hip.h"
#include <type_traits>
#pragma clang fp contract(off)

namespace {

// The picture a launch works on, inside payloads of a larger (or the same) stream: h x w luma samples, planes with the stream's row pitches.
// Everything that clamps (chroma neighbours, edge replication, the egress filters) clamps to h x w and its chroma planes: the kernels compute
// what they would on the cropped stream.  The wide loads and stores test the address itself, so a picture whose rows are not aligned takes
// the element-wise path on its own.
struct YuvGeo {
    int h, w;                   // the picture, in luma samples
    int py, pc;                 // row pitch of the luma and of the chroma planes, in samples
    size_t oy, ou, ov;          // byte offset of the picture's first Y / U / V sample from the start of a payload
    size_t frame_bytes;         // payload to payload
};

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
// separately rounded float32 product / sum / difference.  Written with the operators under the pragma above: the __fmul_rn / __fadd_rn
// of the HIP headers are compiled with the default contraction mode, and their results fuse into v_fma_f32 after inlining.
__device__ __forceinline__ float mulr(float a, float b) { return a * b; }
__device__ __forceinline__ float addr(float a, float b) { return a + b; }
__device__ __forceinline__ float subr(float a, float b) { return a - b; }

template <int ESZ> __device__ __forceinline__ int ld1(const uint8_t* p, size_t i) {
    return ESZ == 1 ? (int)p[i] : (int)((const uint16_t*)p)[i];
}
template <int ESZ> __device__ __forceinline__ void st1(uint8_t* p, size_t i, int v) {
    if (ESZ == 1) p[i] = (uint8_t)v; else ((uint16_t*)p)[i] = (uint16_t)v;
}
// N consecutive samples starting at element i, all inside the plane: one N * ESZ byte load if the address allows it
template <int ESZ, int N> __device__ __forceinline__ void ldn(const uint8_t* p, size_t i, int* v) {
    const uint8_t* a = p + i * ESZ;
    if (((uintptr_t)a & (N * ESZ - 1)) == 0) {
        uint32_t w[N * ESZ / 4];
        if (N * ESZ == 4) w[0] = *(const uint32_t*)a;
        else if (N * ESZ == 8) { const uint2 q = *(const uint2*)a; w[0] = q.x; w[1] = q.y; }
        else { const uint4 q = *(const uint4*)a; w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w; }
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = ESZ == 1 ? (int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu) : (int)((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = ld1<ESZ>(p, i + k);
    }
}
template <int ESZ, int N> __device__ __forceinline__ void stn(uint8_t* p, size_t i, const int* v) {
    uint8_t* a = p + i * ESZ;
    if (((uintptr_t)a & (N * ESZ - 1)) == 0) {
        uint32_t w[N * ESZ / 4];
#pragma unroll
        for (int k = 0; k < N * ESZ / 4; ++k) w[k] = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            if (ESZ == 1) w[k >> 2] |= (uint32_t)v[k] << (8 * (k & 3)); else w[k >> 1] |= (uint32_t)v[k] << (16 * (k & 1));
        }
        if (N * ESZ == 4) *(uint32_t*)a = w[0];
        else if (N * ESZ == 8) *(uint2*)a = make_uint2(w[0], w[1]);
        else *(uint4*)a = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) st1<ESZ>(p, i + k, v[k]);
    }
}

// 8 consecutive elements of an RGB or noise-plane tensor starting at i, of which the first n (1..8) exist; vec: the caller knows that element i is
// 16 B (32 B for f32) aligned
__device__ __forceinline__ void st8_any(void* p, int dt, size_t i, bool vec, int n, const float* v) {
    if (vec) {
        if (dt == SN_F32) {
            *(float4*)((float*)p + i) = make_float4(v[0], v[1], v[2], v[3]);
            *(float4*)((float*)p + i + 4) = make_float4(v[4], v[5], v[6], v[7]);
        } else if (dt == SN_BF16) {
            *(uint4*)((uint16_t*)p + i) = pack8(v);
        } else {
            *(uint4*)((uint16_t*)p + i) = make_uint4(pack_h2(v[0], v[1]), pack_h2(v[2], v[3]), pack_h2(v[4], v[5]), pack_h2(v[6], v[7]));
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) if (k < n) st_any(p, dt, i + k, v[k]);
    }
}

// ---- host: format, payload, geometry ------------------------------------------------------------------------------------------------------
inline bool valid_fmt(const sn_yuv_fmt* f) { return f && (f->bits == 8 || f->bits == 10) && f->chroma >= 0 && f->chroma <= 2; }
// a payload argument at 10 bit is an array of 16-bit words
inline bool aligned_payload(const sn_yuv_fmt* f, const void* p) { return f->bits == 8 || ((uintptr_t)p & 1) == 0; }
// what every entry point asks of its payloads: T of them (a grid dimension), H x W samples of a known format, at an address the kernels can read
inline bool valid_payloads(const void* p, const sn_yuv_fmt* f, int T, int H, int W) {
    return p && valid_fmt(f) && T >= 1 && T <= 65535 && H >= 1 && W >= 1 && aligned_payload(f, p);
}

inline size_t frame_bytes_of(const sn_yuv_fmt* f, int H, int W) {
    const size_t esz = f->bits == 8 ? 1 : 2;
    const size_t c = f->chroma == SN_YUV_444 ? (size_t)H * W : (size_t)((H + 1) / 2) * ((W + 1) / 2);
    return ((size_t)H * W + 2 * c) * esz;
}

// The picture of a launch: the whole H x W frame (rect == nullptr) or rect inside it.  false: rect does not lie inside the frame, or at
// 4:2:0 it would share a chroma sample with its surroundings (x0, y0 odd; w or h odd without reaching the frame's far edge).
inline bool make_geo(const sn_yuv_fmt* f, int H, int W, const sn_yuv_rect* rect, YuvGeo* G) {
    const size_t esz = f->bits == 8 ? 1 : 2;
    const bool sub = f->chroma != SN_YUV_444;
    const int cw = sub ? (W + 1) / 2 : W, ch = sub ? (H + 1) / 2 : H;
    int x0 = 0, y0 = 0, w = W, h = H;
    if (rect) {
        x0 = rect->x0; y0 = rect->y0; w = rect->w; h = rect->h;
        if (x0 < 0 || y0 < 0 || w < 1 || h < 1 || x0 > W - w || y0 > H - h) return false;
        if (sub && ((x0 & 1) || (y0 & 1) || ((w & 1) && x0 + w != W) || ((h & 1) && y0 + h != H))) return false;
    }
    G->h = h; G->w = w; G->py = W; G->pc = cw;
    G->frame_bytes = frame_bytes_of(f, H, W);
    const size_t oc = sub ? (size_t)(y0 >> 1) * cw + (x0 >> 1) : (size_t)y0 * W + x0;
    G->oy = ((size_t)y0 * W + x0) * esz;
    G->ou = ((size_t)H * W + oc) * esz;
    G->ov = G->ou + (size_t)cw * ch * esz;
    return true;
}

// ---- host: from a (valid) format to template arguments ------------------------------------------------------------------------------------
// f(ESZ) or f(ESZ, CH) is called once, with the sample size in bytes and the chroma mode of fmt as std::integral_constant values: inside a generic
// lambda `esz()` and `ch()` are constant expressions, so  with_esz_chroma(fmt, [&](auto esz, auto ch) { launch kernel<esz(), ch()> });  instantiates
// the kernel for every format and launches the one that fmt names.
template <int V> using YuvConst = std::integral_constant<int, V>;
template <typename F> inline void with_esz(const sn_yuv_fmt* fmt, F&& f) {
    if (fmt->bits == 8) f(YuvConst<1>{}); else f(YuvConst<2>{});
}
template <typename F> inline void with_esz_chroma(const sn_yuv_fmt* fmt, F&& f) {
    with_esz(fmt, [&](auto esz) {
        if (fmt->chroma == SN_YUV_444) f(esz, YuvConst<SN_YUV_444>{});
        else if (fmt->chroma == SN_YUV_420_CENTER) f(esz, YuvConst<SN_YUV_420_CENTER>{});
        else f(esz, YuvConst<SN_YUV_420_LEFT>{});
    });
}

}  // namespace
