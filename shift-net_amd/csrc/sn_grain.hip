// Grain put back on a restored stream on the device (gfx950), for `restore_video --grain`: planar Y'CbCr payloads in, planar Y'CbCr payloads of the
// same format out, whole frames or a picture rectangle, in place if asked.
//
//   sn_yuv_grain : T payloads -> T payloads: per sample of every plane a spatially correlated Gaussian field -- a white field, gauss[hash >> 16] of
//                  the counter hash that keys the dither and sn_yuv_degrade, under a separable 5-tap filter -- times a 16-knot curve at the luma
//                  code read, added in the code domain and rounded.
//
// The arithmetic (order of operations, constants) is stated in include/shiftnet_hip.h and restated in float32 by tests/grain_ref.py, which the kernel
// equals byte for byte; every float product and sum is rounded separately (contraction is off for this file: no FMA).
//
// A direct form costs 25 gathers from the 256 KB table per sample.  Here a workgroup owns a tile of 256 x 16 luma samples, as the edge kernels cut
// the picture (32 x 8 threads of 8 x 2 samples): the white field of the tile plus a halo of 2, 20 x 260 samples, is gathered once into LDS (1.27
// gathers per sample), the horizontal pass goes LDS to LDS (two 16 B reads, four outputs, one 16 B write), the vertical pass LDS to registers (six
// rows of a thread's 8 columns).  The chroma planes follow in the same two buffers, each on its own lattice (128 x 8 at 4:2:0), and only where the
// chroma share is not 0.  41 KB of LDS: three workgroups a CU.  The halo comes from the hash, never from memory, and a thread reads its own samples
// before it stores them: dst == src is legal.  White grain (taps 1, 0, 0) needs no neighbour and takes a path without LDS, with the same bytes.
#include "sn_yuv_color.h"
#pragma clang fp contract(off)

namespace {

constexpr int GR_TW = 256, GR_TH = 16;                  // a workgroup's tile in luma samples
constexpr int GR_ROWS = GR_TH + 4;                      // with the halo of 2 above and below
constexpr int GR_GP = GR_TW + 4;                        // row pitch of the white field: the halo of 2 left and right; a multiple of 4 (16 B rows)

struct GrainK {
    float k[SN_NLF_BANDS];          // the curve in luma codes of the format
    float lo, scale;                // the black luma code, 16 / (white - black)
    float chroma, w0, w1, w2;
    uint32_t seed, t0;
    int cmode;                      // chroma planes: 0 untouched (in place, share 0), 1 copied (share 0), 2 grained
};

__device__ __forceinline__ float fir5(const GrainK& N, float a, float b, float c, float d, float e) {
    return addr(addr(addr(addr(mulr(N.w2, a), mulr(N.w1, b)), mulr(N.w0, c)), mulr(N.w1, d)), mulr(N.w2, e));
}

__device__ __forceinline__ float white(const float* __restrict__ gauss, uint32_t fk, int plane, int y, int x) {
    return gauss[hash_sample(dither_row_key(fk, plane, y), x) >> 16];
}

// The curve at a luma code: sn_yuv_degrade's interpolation.  kn: the knots in LDS.
__device__ __forceinline__ float level_at(const float* kn, const GrainK& N, int Y) {
    const float u = fminf(fmaxf(subr(mulr(subr((float)Y, N.lo), N.scale), 0.5f), 0.f), 15.f);
    const int i = imin((int)u, SN_NLF_BANDS - 2);                          // u >= 0: the conversion is the floor
    return addr(kn[i], mulr(subr(u, (float)i), subr(kn[i + 1], kn[i])));
}

// One plane's tile of TW x TH samples at (ty0, tx0) of a ph x pw plane, all 256 threads: the white field of rows ty0 - 2 .. and columns tx0 - 2 ..
// into gb, its horizontal pass into hb (row r of hb is plane row ty0 - 2 + r, column c plane column tx0 + c).  Only what the plane has is made.
template <int TW, int TH>
__device__ __forceinline__ void stage_field(float* gb, float* hb, const float* __restrict__ gauss, const GrainK& N, uint32_t fk, int plane, int ty0, int tx0,
                                            int ph, int pw, int tid) {
    const int nr = imin(TH, ph - ty0) + 4, nc = imin(TW, pw - tx0) + 4, nq = (nc - 1) >> 2;      // nq: quads of columns, ceil((nc - 4) / 4)
    for (int idx = tid; idx < nr * (TW + 4); idx += 256) {
        const int r = idx / (TW + 4), c = idx - r * (TW + 4);
        if (c < nc) gb[r * GR_GP + c] = white(gauss, fk, plane, ty0 - 2 + r, tx0 - 2 + c);
    }
    __syncthreads();
    for (int idx = tid; idx < nr * (TW / 4); idx += 256) {
        const int r = idx / (TW / 4), q = idx - r * (TW / 4);
        if (q >= nq) continue;
        const float4 a = *(const float4*)&gb[r * GR_GP + 4 * q], b = *(const float4*)&gb[r * GR_GP + 4 * q + 4];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = fir5(N, v[k], v[k + 1], v[k + 2], v[k + 3], v[k + 4]);
        *(float4*)&hb[r * GR_TW + 4 * q] = make_float4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
}

// The vertical pass for a thread's NX x NY samples at (ly, lx) of the tile: rows ly .. ly + NY + 3 of hb
template <int NX, int NY>
__device__ __forceinline__ void column_pass(const float* hb, const GrainK& N, int ly, int lx, float (*c)[8]) {
    float v[NY + 4][NX];
#pragma unroll
    for (int r = 0; r < NY + 4; ++r)
#pragma unroll
        for (int q = 0; q < NX / 4; ++q) {
            const float4 a = *(const float4*)&hb[(ly + r) * GR_TW + lx + 4 * q];
            v[r][4 * q] = a.x; v[r][4 * q + 1] = a.y; v[r][4 * q + 2] = a.z; v[r][4 * q + 3] = a.w;
        }
#pragma unroll
    for (int r = 0; r < NY; ++r)
#pragma unroll
        for (int k = 0; k < NX; ++k) c[r][k] = fir5(N, v[r][k], v[r + 1][k], v[r + 2][k], v[r + 3][k], v[r + 4][k]);
}

template <int ESZ, int CH, bool WHITE>
__global__ __launch_bounds__(256) void grain_yuv_kernel(const uint8_t* src, uint8_t* dstp, const float* __restrict__ gauss, const YuvK K, const GrainK N,
                                                      const YuvGeo G) {
    constexpr int CNX = CH == SN_YUV_444 ? 8 : 4, CNY = CH == SN_YUV_444 ? 2 : 1;      // a thread's chroma samples
    constexpr int CTW = CH == SN_YUV_444 ? GR_TW : GR_TW / 2, CTH = CH == SN_YUV_444 ? GR_TH : GR_TH / 2;
    __shared__ float kn[SN_NLF_BANDS];
    __shared__ __attribute__((aligned(16))) float gb[WHITE ? 4 : GR_ROWS * GR_GP];
    __shared__ __attribute__((aligned(16))) float hb[WHITE ? 4 : GR_ROWS * GR_TW];
    const int tid = threadIdx.y * 32 + threadIdx.x;
    if (tid < SN_NLF_BANDS) kn[tid] = N.k[tid];
    __syncthreads();
    const int t = blockIdx.z;
    const int tx0 = blockIdx.x * GR_TW, ty0 = blockIdx.y * GR_TH;
    const int x0 = tx0 + threadIdx.x * 8, y0 = ty0 + threadIdx.y * 2;
    const int H = G.h, W = G.w, py = G.py, pc = G.pc;
    const bool active = x0 < W && y0 < H;                  // the others help with the tile's field and own nothing
    const int cw = CH == SN_YUV_444 ? W : (W + 1) >> 1, ch = CH == SN_YUV_444 ? H : (H + 1) >> 1;
    const int cx0 = CH == SN_YUV_444 ? x0 : x0 >> 1, cy0 = CH == SN_YUV_444 ? y0 : y0 >> 1;
    const int ctx0 = CH == SN_YUV_444 ? tx0 : tx0 >> 1, cty0 = CH == SN_YUV_444 ? ty0 : ty0 >> 1;
    const uint8_t* ibase = src + (size_t)t * G.frame_bytes;
    uint8_t* obase = dstp + (size_t)t * G.frame_bytes;
    const uint32_t fk = hash_frame_key(N.seed, N.t0 + (uint32_t)t);
    const bool inner = x0 + 8 <= W;
    const int n = imin(8, W - x0), ncx = imin(CNX, cw - cx0);
    const bool cinner = ncx == CNX;
    // ---- everything the thread reads from memory, before anything is stored: its 8 x 2 luma codes (coordinates clamped to the picture) and its chroma
    int Y[2][8], Cq[2][CNY][CNX];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 8; ++k) Y[r][k] = 0;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
        for (int r = 0; r < CNY; ++r)
#pragma unroll
            for (int k = 0; k < CNX; ++k) Cq[pl][r][k] = 0;
    if (active) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const size_t row = (size_t)imin(y0 + r, H - 1) * py;
            if (inner) ldn<ESZ, 8>(ibase + G.oy, row + x0, Y[r]);
            else {
#pragma unroll
                for (int k = 0; k < 8; ++k) Y[r][k] = ld1<ESZ>(ibase + G.oy, row + imin(x0 + k, W - 1));
            }
        }
        if (N.cmode) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const uint8_t* cp = ibase + (pl ? G.ov : G.ou);
#pragma unroll
                for (int r = 0; r < CNY; ++r) {
                    if (cy0 + r >= ch) break;
                    const size_t o = (size_t)(cy0 + r) * pc + cx0;
                    if (cinner) ldn<ESZ, CNX>(cp, o, Cq[pl][r]);
                    else for (int k = 0; k < ncx; ++k) Cq[pl][r][k] = ld1<ESZ>(cp, o + k);
                }
            }
        }
    }
    // ---- luma: plane 6 ---------------------------------------------------------------------------------------------------------------------------
    float c[2][8];
    if constexpr (WHITE) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 8; ++k) c[r][k] = active ? white(gauss, fk, 6, y0 + r, x0 + k) : 0.f;
    } else {
        stage_field<GR_TW, GR_TH>(gb, hb, gauss, N, fk, 6, ty0, tx0, H, W, tid);
        if (active) column_pass<8, 2>(hb, N, threadIdx.y * 2, threadIdx.x * 8, c);
    }
    int Yo[2][8];
    if (active) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int v = Y[r][k];
                const int q = __float2int_rn(addr((float)v, mulr(level_at(kn, N, v), c[r][k])));
                Yo[r][k] = imin(imax(q, imin(K.ylo, v)), imax(K.yhi, v));
            }
    }
    // ---- chroma: planes 7 and 8, each on its own lattice; the level is the curve at the luma code read at the sample's place --------------------
    int Co[2][CNY][CNX];
    if (N.cmode == 2) {
        float s[CNY][CNX];
#pragma unroll
        for (int r = 0; r < CNY; ++r)
#pragma unroll
            for (int k = 0; k < CNX; ++k) {
                int ym;                                    // 4:2:0: the rounded mean of the sample's 2 x 2 luma block, clamped to the picture as loaded
                if constexpr (CH == SN_YUV_444) ym = Y[r][k];
                else ym = (Y[0][2 * k] + Y[0][2 * k + 1] + Y[1][2 * k] + Y[1][2 * k + 1] + 2) >> 2;
                s[r][k] = mulr(N.chroma, level_at(kn, N, ym));
            }
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            float cc[2][8];
            if constexpr (WHITE) {
#pragma unroll
                for (int r = 0; r < CNY; ++r)
#pragma unroll
                    for (int k = 0; k < CNX; ++k) cc[r][k] = active ? white(gauss, fk, 7 + pl, cy0 + r, cx0 + k) : 0.f;
            } else {
                stage_field<CTW, CTH>(gb, hb, gauss, N, fk, 7 + pl, cty0, ctx0, ch, cw, tid);
                if (active) column_pass<CNX, CNY>(hb, N, threadIdx.y * CNY, threadIdx.x * CNX, cc);
            }
            if (active) {
#pragma unroll
                for (int r = 0; r < CNY; ++r)
#pragma unroll
                    for (int k = 0; k < CNX; ++k) {
                        const int v = Cq[pl][r][k];
                        const int q = __float2int_rn(addr((float)v, mulr(s[r][k], cc[r][k])));
                        Co[pl][r][k] = imin(imax(q, imin(K.clo, v)), imax(K.chi, v));
                    }
            }
        }
    } else {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int r = 0; r < CNY; ++r)
#pragma unroll
                for (int k = 0; k < CNX; ++k) Co[pl][r][k] = Cq[pl][r][k];
    }
    if (!active) return;
    // ---- the stores: wide where the address allows ---------------------------------------------------------------------------------------------
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (y0 + r >= H) break;
        const size_t o = (size_t)(y0 + r) * py + x0;
        if (inner) stn<ESZ, 8>(obase + G.oy, o, Yo[r]); else for (int k = 0; k < n; ++k) st1<ESZ>(obase + G.oy, o + k, Yo[r][k]);
    }
    if (N.cmode) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            uint8_t* cp = obase + (pl ? G.ov : G.ou);
#pragma unroll
            for (int r = 0; r < CNY; ++r) {
                if (cy0 + r >= ch) break;
                const size_t o = (size_t)(cy0 + r) * pc + cx0;
                if (cinner) stn<ESZ, CNX>(cp, o, Co[pl][r]); else for (int k = 0; k < ncx; ++k) st1<ESZ>(cp, o + k, Co[pl][r][k]);
            }
        }
    }
}

inline bool finite_nonneg(float v) { return v >= 0.f && v - v == 0.f; }      // refuses negative, NaN, infinity

}  // namespace

extern "C" {

int sn_yuv_grain(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const sn_yuv_grain_noise* grain, const float* gauss, uint8_t* dst,
                 int T, int H, int W, void* stream) {
    sn_clear_error();
    YuvK K;
    YuvGeo G;
    if (!valid_payloads(dst, fmt, T, H, W) || !src || !aligned_payload(fmt, src) || !make_consts(fmt, &K)) return SN_EINVAL;
    if (!grain || !gauss || ((uintptr_t)gauss & 3) || grain->t0 < 0 || !make_geo(fmt, H, W, rect, &G)) return SN_EINVAL;
    GrainK N;
    for (int i = 0; i < SN_NLF_BANDS; ++i) {
        if (!finite_nonneg(grain->knots[i])) return SN_EINVAL;
        N.k[i] = grain->knots[i];
    }
    const float w0 = grain->taps[0], w1 = grain->taps[1], w2 = grain->taps[2];
    if (!finite_nonneg(grain->chroma) || !finite_nonneg(w0) || !finite_nonneg(w1) || !finite_nonneg(w2) || !(w0 > 0.f)) return SN_EINVAL;
    const double energy = (double)w0 * w0 + 2.0 * ((double)w1 * w1) + 2.0 * ((double)w2 * w2);
    if (!(energy >= 1.0 - 1e-3 && energy <= 1.0 + 1e-3)) return SN_EINVAL;
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    const size_t bytes = (size_t)T * G.frame_bytes;
    if (a != b && a < b + bytes && b < a + bytes) return SN_EINVAL;       // in place, or apart: a thread stores only what it alone has read
    N.lo = (float)K.ylo;
    N.scale = (float)(16.0 / ((double)K.yhi - (double)K.ylo));
    N.chroma = grain->chroma; N.w0 = w0; N.w1 = w1; N.w2 = w2;
    N.seed = grain->seed; N.t0 = (uint32_t)grain->t0;
    N.cmode = grain->chroma != 0.f ? 2 : (a == b ? 0 : 1);
    const bool white = w0 == 1.f && w1 == 0.f && w2 == 0.f;
    const dim3 block(32, 8), grid((G.w + GR_TW - 1) / GR_TW, (G.h + GR_TH - 1) / GR_TH, T);
    if (grid.y > 65535) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    with_esz_chroma(fmt, [&](auto esz, auto ch) {
        if (white) hipLaunchKernelGGL((grain_yuv_kernel<esz(), ch(), true>), grid, block, 0, s, src, dst, gauss, K, N, G);
        else hipLaunchKernelGGL((grain_yuv_kernel<esz(), ch(), false>), grid, block, 0, s, src, dst, gauss, K, N, G);
    });
    return sn_check_launch();
}

}  // extern "C"
