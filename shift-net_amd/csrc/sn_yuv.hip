// Y'CbCr <-> RGB edges of the video restorer on the device (gfx950): planar YUV frames as a Y4M stream carries them in,
// planar YUV frames out.  4:2:0 crosses PCIe at 1.5 B per pixel (8 bit) and no float frame touches the host.
//
//   sn_ingest_yuv : T payloads [Y plane][U plane][V plane] -> [T][3][Hp][Wp] RGB of the module dtype in [0,1]; pixels outside H x W
//                   replicate the edge pixel, so one launch gives the network a legal size for any input size;
//   sn_egress_yuv : [T][3][Hp][Wp] RGB (float32 or module dtype) -> T payloads of H x W (the crop of the padding);
//   sn_egress_yuv_dither : the same with triangular noise of +-1 code added before the rounding (SN_DITHER_TPDF), an integer hash of the
//                   sample's position: instantiations of their own of the same kernel, the entry points without _dither launch the others;
//   sn_egress_yuv_mix : the same, dithered or not, blended in the code domain with the code every sample had on the way in (SN_MIX_AMOUNT: "70 % of the
//                   correction", separately for luma and chroma; amount 0 is the input byte for byte) or the difference input minus result around
//                   mid-grey (SN_MIX_REMOVED): a further template parameter of the same kernel, which then reads the T input payloads beside dst;
//   sn_yuv_thumb  : T payloads -> [T][ceil(H/8)][ceil(W/8)] uint16 sums of the luma codes of every 8 x 8 block (the scene-cut measure of
//                   shiftnet_amd/scenes.py is computed from these on the host); integer arithmetic, the chroma planes are not read.
//   sn_yuv_noise_hist : T payloads -> [T][2 (2^bits - 1) + 1] uint32 histograms of |a - b - c + d| over the 2 x 2 luma blocks whose four codes lie
//                   strictly between lo and hi (the blind noise estimate of shiftnet_amd/noise.py is computed from these on the host); integer
//                   arithmetic, the chroma planes are not read.
//   sn_yuv_noise_hist_bands : the same statistic split into 16 bands of the block's brightness, v saturated to NBV = 128 / 512 bins: [T][16][NBV]
//                   uint32 (the noise-level function of shiftnet_amd/noise.py is estimated from these on the host); rect or the whole frame.
//   sn_noise_map_level : T payloads and the 16 knots of a noise-level function -> [T][1][Hp][Wp] of the module dtype or float32: the function at the
//                   low-passed luma of every pixel (bilinear between the means of the 8 x 8 blocks): the denoisers' noise plane; rect or the whole frame.
//   sn_yuv_rowcol_sums : T payloads -> [T][H] and [T][W] uint32 sums of the luma codes of every row and every column (the letterbox rule of
//                   shiftnet_amd/picture.py is evaluated on these on the host); integer arithmetic, the chroma planes are not read.
//   sn_ingest_yuv_rect / sn_egress_yuv_rect / sn_yuv_noise_hist_rect : the first, second and fourth restricted to a picture rectangle of the
//                   stream.  They are the same kernels: every kernel sees "its frame" as h x w samples whose planes have a row pitch and a
//                   first sample of their own (YuvGeo); the entry points without _rect pass the whole frame.
//
// The arithmetic (order of operations, constants) is stated in include/shiftnet_hip.h and restated in float32 by tests/yuv_ref.py,
// which these kernels equal bit for bit.  Every float product and sum is rounded separately (contraction is off for this file: no
// FMA); the chroma upsampling is integer arithmetic and therefore exact.
//
// Both are bandwidth kernels.  A thread owns four horizontally adjacent 2x2 luma blocks (8 x 2 pixels), so that every chroma sample is
// produced once and the 8 pixels of a row are one 8 / 16 B load and one 16 / 2 x 16 B store where the address is aligned; a thread
// whose span is not aligned, or touches the frame edge or the padding, takes the element-wise path with the same arithmetic.
#include "sn_common.h"
#include "../../include/shiftnet_hip.h"
#pragma clang fp contract(off)

namespace {

struct YuvK {
    // ingest: R = ky*(Y - yoff) + crv*(V - coff), G = (ky*(Y - yoff) + cgu*(U - coff)) + cgv*(V - coff), B = ky*(Y - yoff) + cbu*(U - coff)
    float ky, crv, cgu, cgv, cbu;
    // egress: Y' = (kr*R + kg*G) + kb*B, Cb = (B - Y')*cu, Cr = (R - Y')*cv; code = rint(off + scale * value)
    float kr, kg, kb, cu, cv, ys, yo, cs, co;
    int yoff, coff, ylo, yhi, clo, chi;
};

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
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

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

// ---- RGB tensor elements ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ld_any(const void* p, int dt, size_t i) {
    return dt == SN_F32 ? ((const float*)p)[i] : (dt == SN_F16 ? __half2float(((const __half*)p)[i]) : bf_to_f(((const bf16_t*)p)[i]));
}
__device__ __forceinline__ void st_any(void* p, int dt, size_t i, float v) {       // as st_any of sn_io.hip
    if (dt == SN_F32) ((float*)p)[i] = v;
    else if (dt == SN_F16) ((__half*)p)[i] = __float2half(v);
    else ((bf16_t*)p)[i] = f_to_bf(v);
}
__device__ __forceinline__ float h_lo(uint32_t u) { return __half2float(__ushort_as_half((unsigned short)(u & 0xffffu))); }
__device__ __forceinline__ float h_hi(uint32_t u) { return __half2float(__ushort_as_half((unsigned short)(u >> 16))); }
// 8 consecutive elements starting at i (all inside the tensor); vec: the caller knows that element i is 16 B (32 B for f32) aligned
__device__ __forceinline__ void ld8_any(const void* p, int dt, size_t i, bool vec, float* v) {
    if (vec) {
        if (dt == SN_F32) {
            const float4 a = *(const float4*)((const float*)p + i), b = *(const float4*)((const float*)p + i + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
            const uint4 q = *(const uint4*)((const uint16_t*)p + i);
            if (dt == SN_BF16) unpack8(q, v);
            else { v[0] = h_lo(q.x); v[1] = h_hi(q.x); v[2] = h_lo(q.y); v[3] = h_hi(q.y); v[4] = h_lo(q.z); v[5] = h_hi(q.z); v[6] = h_lo(q.w); v[7] = h_hi(q.w); }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = ld_any(p, dt, i + k);
    }
}
// 8 consecutive elements starting at i, of which the first n (1..8) exist
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

template <int ESZ, int CH>
__global__ __launch_bounds__(256) void ingest_yuv_kernel(const uint8_t* __restrict__ src, void* __restrict__ dst, int dt, const YuvK K,
                                                       const YuvGeo G, int Hp, int Wp, int dst_vec) {
    const int t = blockIdx.z;
    const int x0 = (blockIdx.x * 32 + threadIdx.x) * 8, y0 = (blockIdx.y * 8 + threadIdx.y) * 2;
    if (x0 >= Wp || y0 >= Hp) return;
    const int H = G.h, W = G.w, py = G.py, pc = G.pc;
    const int cw = CH == SN_YUV_444 ? W : (W + 1) >> 1, ch = CH == SN_YUV_444 ? H : (H + 1) >> 1;
    const uint8_t* base = src + (size_t)t * G.frame_bytes;
    const uint8_t* yp = base + G.oy;
    const uint8_t* up = base + G.ou;
    const uint8_t* vp = base + G.ov;
    float rgb[3][2][8];
    if (x0 + 8 <= W && y0 + 2 <= H) {                      // interior: whole blocks, wide loads
        int Y[2][8];
#pragma unroll
        for (int r = 0; r < 2; ++r) ldn<ESZ, 8>(yp, (size_t)(y0 + r) * py + x0, Y[r]);
        if (CH == SN_YUV_444) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                int U[8], V[8];
                ldn<ESZ, 8>(up, (size_t)(y0 + r) * pc + x0, U);
                ldn<ESZ, 8>(vp, (size_t)(y0 + r) * pc + x0, V);
#pragma unroll
                for (int k = 0; k < 8; ++k) yuv_to_rgb<CH>(K, Y[r][k], U[k], V[k], &rgb[0][r][k], &rgb[1][r][k], &rgb[2][r][k]);
            }
        } else {
            const int j = y0 >> 1, c0 = x0 >> 1;
            const int jr[3] = {imax(j - 1, 0), j, imin(j + 1, ch - 1)};
            int num[2][2][8];                               // [plane][row][pixel]
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const uint8_t* cp = pl ? vp : up;
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
                for (int k = 0; k < 8; ++k) yuv_to_rgb<CH>(K, Y[r][k], num[0][r][k], num[1][r][k], &rgb[0][r][k], &rgb[1][r][k], &rgb[2][r][k]);
        }
    } else {                                               // frame edge and padding: pixel (y, x) is pixel (min(y, H-1), min(x, W-1))
        for (int r = 0; r < 2; ++r) {
            const int ye = imin(y0 + r, H - 1);
            for (int k = 0; k < 8; ++k) {
                const int xe = imin(x0 + k, W - 1);
                const int y = ld1<ESZ>(yp, (size_t)ye * py + xe);
                int un, vn;
                if (CH == SN_YUV_444) { un = ld1<ESZ>(up, (size_t)ye * pc + xe); vn = ld1<ESZ>(vp, (size_t)ye * pc + xe); }
                else { un = chroma_num<ESZ, CH>(up, pc, cw, ch, ye, xe); vn = chroma_num<ESZ, CH>(vp, pc, cw, ch, ye, xe); }
                yuv_to_rgb<CH>(K, y, un, vn, &rgb[0][r][k], &rgb[1][r][k], &rgb[2][r][k]);
            }
        }
    }
    const int n = imin(8, Wp - x0);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 2; ++r)
            if (y0 + r < Hp) st8_any(dst, dt, (((size_t)t * 3 + c) * Hp + (y0 + r)) * Wp + x0, dst_vec != 0, n, rgb[c][r]);
}

// ---- egress -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int quant(float off, float scale, float v, int lo, int hi) {
    return imin(imax(__float2int_rn(addr(off, mulr(scale, v))), lo), hi);
}

// The dither of a launch.  DITHER is a template parameter of the kernel: SN_DITHER_NONE carries nothing and every line below that touches a
// key is dead in it, so the instantiations the entry points without _dither launch are the ones they launched before there was a dither.
template <int DITHER> struct DitherK {};
template <> struct DitherK<SN_DITHER_TPDF> { uint32_t seed; uint32_t t0; };
template <int DITHER> __device__ __forceinline__ uint32_t dither_frame_key(const DitherK<DITHER>&, int) { return 0u; }
template <> __device__ __forceinline__ uint32_t dither_frame_key<SN_DITHER_TPDF>(const DitherK<SN_DITHER_TPDF>& D, int t) {
    return ((D.t0 + (uint32_t)t) * 0xC2B2AE3Du) ^ D.seed;
}
// plane p, row y of the plane: the part of the key that a row of samples shares (uint32 arithmetic wraps)
__device__ __forceinline__ uint32_t dither_row_key(uint32_t fk, int p, int y) { return fk ^ ((uint32_t)p * 0x27D4EB2Fu) ^ ((uint32_t)y * 0x9E3779B1u); }
// the sample at column x of that row: the murmur3 finaliser of the key, two 12-bit fields of it summed to a triangle on (-1, 1); exact in float32
__device__ __forceinline__ float dither_tpdf(uint32_t rk, int x) {
    uint32_t k = rk ^ ((uint32_t)x * 0x85EBCA77u);
    k ^= k >> 16; k *= 0x85EBCA6Bu; k ^= k >> 13; k *= 0xC2B2AE35u; k ^= k >> 16;
    return mulr((float)((int)(k & 0xFFFu) + (int)((k >> 12) & 0xFFFu) - 4095), 1.0f / 4096.0f);
}
// code = clamp(rint((off + scale * v) + d)); without dither the line above
template <int DITHER> __device__ __forceinline__ int quantd(float off, float scale, float v, int lo, int hi, uint32_t rk, int x) {
    if (DITHER == SN_DITHER_NONE) return quant(off, scale, v, lo, hi);
    return imin(imax(__float2int_rn(addr(addr(off, mulr(scale, v)), dither_tpdf(rk, x))), lo), hi);
}

// The mix of a launch (sn_egress_yuv_mix): the code the same sample had on the way in is read beside the value on the way out.  MIX is a template
// parameter of the kernel as DITHER is: SN_MIX_OFF carries nothing, reads nothing and every line below that touches `in` is dead in it, so the
// instantiations of the entry points without _mix are the ones they launched before there was a mix.
constexpr int SN_MIX_OFF = -1;
template <int MIX> struct MixK { const uint8_t* in; float ay, ac; };       // in: T payloads laid out as dst; AMOUNT: the amounts, REMOVED: the gains
template <> struct MixK<SN_MIX_OFF> {};
template <int MIX> __device__ __forceinline__ const uint8_t* mix_in(const MixK<MIX>& M) { return M.in; }
template <> __device__ __forceinline__ const uint8_t* mix_in<SN_MIX_OFF>(const MixK<SN_MIX_OFF>&) { return nullptr; }
template <int MIX> __device__ __forceinline__ float mix_a(const MixK<MIX>& M, bool chroma) { return chroma ? M.ac : M.ay; }
template <> __device__ __forceinline__ float mix_a<SN_MIX_OFF>(const MixK<SN_MIX_OFF>&, bool) { return 0.f; }
// v = off + scale * value as quantd forms it, e = float(code_in), d the sample's dither (0 without one):
//   AMOUNT : a == 0: code_in;  otherwise clamp(rint((e + a * (v - e)) + d), min(lo, code_in), max(hi, code_in))
//   REMOVED: clamp(rint((co + a * (e - v)) + d), lo, hi)
template <int DITHER, int MIX>
__device__ __forceinline__ int quantm(float off, float scale, float v, int lo, int hi, uint32_t rk, int x, int cin, float a, float co) {
    if (MIX == SN_MIX_OFF) return quantd<DITHER>(off, scale, v, lo, hi, rk, x);
    const float val = addr(off, mulr(scale, v)), e = (float)cin;
    float m = MIX == SN_MIX_AMOUNT ? addr(e, mulr(a, subr(val, e))) : addr(co, mulr(a, subr(e, val)));
    if (DITHER != SN_DITHER_NONE) m = addr(m, dither_tpdf(rk, x));
    if (MIX == SN_MIX_AMOUNT) { lo = imin(lo, cin); hi = imax(hi, cin); }
    const int c = imin(imax(__float2int_rn(m), lo), hi);
    return MIX == SN_MIX_AMOUNT && a == 0.f ? cin : c;
}
// the N codes of `in` beside a store of N samples at element i: the wide load where all N exist, the first n element-wise otherwise (the others are not stored)
template <int ESZ, int N, int MIX> __device__ __forceinline__ void mix_ld(const uint8_t* p, size_t i, bool all, int n, int* e) {
    if (MIX != SN_MIX_OFF && all) { ldn<ESZ, N>(p, i, e); return; }
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = MIX != SN_MIX_OFF && k < n ? ld1<ESZ>(p, i + k) : 0;
}

template <int ESZ, int CH, int DITHER = SN_DITHER_NONE, int MIX = SN_MIX_OFF>
__global__ __launch_bounds__(256) void egress_yuv_kernel(const void* __restrict__ out, int dt, uint8_t* __restrict__ dstp, const YuvK K,
                                                       const YuvGeo G, int Hp, int Wp, int src_vec, const DitherK<DITHER> D, const MixK<MIX> M) {
    const int t = blockIdx.z;
    const int x0 = (blockIdx.x * 32 + threadIdx.x) * 8, y0 = (blockIdx.y * 8 + threadIdx.y) * 2;
    const int H = G.h, W = G.w, py = G.py, pc = G.pc;
    if (x0 >= W || y0 >= H) return;
    const int cw = CH == SN_YUV_444 ? W : (W + 1) >> 1;
    uint8_t* base = dstp + (size_t)t * G.frame_bytes;
    uint8_t* yp = base + G.oy;
    uint8_t* up = base + G.ou;
    uint8_t* vp = base + G.ov;
    // the payloads that came in: the sample that belongs to a sample of dst sits at the same byte offset
    const uint8_t* ibase = MIX == SN_MIX_OFF ? nullptr : mix_in<MIX>(M) + (size_t)t * G.frame_bytes;
    const uint8_t* iyp = ibase + (MIX == SN_MIX_OFF ? 0 : G.oy);
    const uint8_t* iup = ibase + (MIX == SN_MIX_OFF ? 0 : G.ou);
    const uint8_t* ivp = ibase + (MIX == SN_MIX_OFF ? 0 : G.ov);
    const float ay = mix_a<MIX>(M, false), ac = mix_a<MIX>(M, true);
    const bool inner = x0 + 8 <= W;
    // Y', Cb, Cr of pixels x0 - 1 .. x0 + 7 (index 0 .. 8) of rows y0, y0 + 1, coordinates clamped to the H x W frame
    float yv[2][9], cb[2][9], cr[2][9];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int ye = imin(y0 + r, H - 1);
        float c[3][9];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const size_t row = (((size_t)t * 3 + q) * Hp + ye) * Wp;
            if (inner) ld8_any(out, dt, row + x0, src_vec != 0, &c[q][1]);
            else for (int k = 0; k < 8; ++k) c[q][1 + k] = ld_any(out, dt, row + imin(x0 + k, W - 1));
            c[q][0] = CH == SN_YUV_420_LEFT ? ld_any(out, dt, row + imax(x0 - 1, 0)) : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float R = clamp01(c[0][k]), G = clamp01(c[1][k]), B = clamp01(c[2][k]);
            const float y = addr(addr(mulr(K.kr, R), mulr(K.kg, G)), mulr(K.kb, B));
            yv[r][k] = y;
            cb[r][k] = mulr(subr(B, y), K.cu);
            cr[r][k] = mulr(subr(R, y), K.cv);
        }
    }
    const int n = imin(8, W - x0);
    const uint32_t fk = dither_frame_key<DITHER>(D, t);    // the sample positions count from the picture's first sample: x0, y0 do
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (y0 + r >= H) break;
        int q[8], e[8];
        const size_t o = (size_t)(y0 + r) * py + x0, oc = (size_t)(y0 + r) * pc + x0;
        mix_ld<ESZ, 8, MIX>(iyp, o, inner, n, e);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            q[k] = quantm<DITHER, MIX>(K.yo, K.ys, yv[r][1 + k], K.ylo, K.yhi, dither_row_key(fk, 0, y0 + r), x0 + k, e[k], ay, K.co);
        if (inner) stn<ESZ, 8>(yp, o, q); else for (int k = 0; k < n; ++k) st1<ESZ>(yp, o + k, q[k]);
        if (CH == SN_YUV_444) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                mix_ld<ESZ, 8, MIX>(pl ? ivp : iup, oc, inner, n, e);
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    q[k] = quantm<DITHER, MIX>(K.co, K.cs, pl ? cr[r][1 + k] : cb[r][1 + k], K.clo, K.chi, dither_row_key(fk, 1 + pl, y0 + r), x0 + k, e[k],
                                               ac, K.co);
                if (inner) stn<ESZ, 8>(pl ? vp : up, oc, q); else for (int k = 0; k < n; ++k) st1<ESZ>(pl ? vp : up, oc + k, q[k]);
            }
        }
    }
    if (CH != SN_YUV_444) {
        const int c0 = x0 >> 1, nc = imin(4, cw - c0);
        const size_t o = (size_t)(y0 >> 1) * pc + c0;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            int q[4], e[4];
            if constexpr (MIX != SN_MIX_OFF) mix_ld<ESZ, 4, MIX>(pl ? ivp : iup, o, nc == 4, nc, e);
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
                // (constexpr: with the call below alone the dithered 4:2:0 instantiations without a mix come out with one s_mov scheduled elsewhere)
                if constexpr (MIX == SN_MIX_OFF) q[i] = quantd<DITHER>(K.co, K.cs, m, K.clo, K.chi, dither_row_key(fk, 1 + pl, y0 >> 1), c0 + i);
                else q[i] = quantm<DITHER, MIX>(K.co, K.cs, m, K.clo, K.chi, dither_row_key(fk, 1 + pl, y0 >> 1), c0 + i, e[i], ac, K.co);
            }
            if (nc == 4) stn<ESZ, 4>(pl ? vp : up, o, q); else for (int i = 0; i < nc; ++i) st1<ESZ>(pl ? vp : up, o + i, q[i]);
        }
    }
}

// ---- thumbnail ------------------------------------------------------------------------------------------------------------------
// A lane owns one 8 x 8 luma block: 8 rows of one 8 B (10 bit: 16 B) load where the address allows it, element-wise on the right edge
// (x0 + 8 > W: only the pixels inside the frame are read and summed) and where the row's address is not aligned.  Neighbouring lanes
// own neighbouring blocks of a block row, so a wave's load covers 512 (1024) consecutive bytes of a luma row and its store 128 bytes.
// No atomics and no cross-lane step: the sum is an exact integer, the same for every launch geometry (64 x 1023 = 65 472 < 2^16).
template <int ESZ>
__global__ __launch_bounds__(256) void yuv_thumb_kernel(const uint8_t* __restrict__ src, uint16_t* __restrict__ dst, int H, int W, int hb, int wb,
                                                      size_t frame_bytes) {
    const int t = blockIdx.z;
    const int bx = blockIdx.x * 32 + threadIdx.x, by = blockIdx.y * 8 + threadIdx.y;
    if (bx >= wb || by >= hb) return;
    const uint8_t* yp = src + (size_t)t * frame_bytes;
    const int x0 = bx * 8, y0 = by * 8;
    const int rows = imin(8, H - y0), n = imin(8, W - x0);
    int sum = 0;
    if (n == 8) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (r < rows) {
                int v[8];
                ldn<ESZ, 8>(yp, (size_t)(y0 + r) * W + x0, v);
                sum += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
            }
        }
    } else {
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < n; ++k) sum += ld1<ESZ>(yp, (size_t)(y0 + r) * W + x0 + k);
    }
    dst[((size_t)t * hb + by) * wb + bx] = (uint16_t)sum;
}

// ---- noise histogram ------------------------------------------------------------------------------------------------------------
// v = |a - b - c + d| of every non-overlapping 2 x 2 luma block (twice its Haar HH coefficient), counted where all four codes lie strictly
// between lo and hi.  A lane owns four horizontally adjacent blocks (8 x 2 pixels: one 8 B / 16 B load per row where the ADDRESS allows it,
// element-wise otherwise and where fewer than four blocks are left on the right edge); a workgroup walks units gridDim.x * 256 apart of one
// frame and keeps that frame's histogram in LDS: bins >= LOW in one array of NB words, bins < LOW -- where nearly all of the mass lies --
// in 32 copies, copy (lane & 31) at word v * 32 + (lane & 31).  An LDS instruction is served in lane groups 0..31 and 32..63 and a b32
// access banks by word mod 32, so the 32 lanes of a group hit 32 different banks whatever their v: a wave's add to the low bins never
// meets a bank conflict or a second lane on its own address.  At the end the copies are summed and the non-zero bins added to dst with
// one global atomic each.  Integer sums commute: the result is the same for every geometry and every schedule.
template <int ESZ> struct NoiseK {
    static constexpr int NB = 2 * ((ESZ == 1 ? 256 : 1024) - 1) + 1;      // 511 / 2047
    static constexpr int LOW = ESZ == 1 ? 32 : 128;                       // the same range of noise levels at both depths
};

template <int ESZ>
__global__ __launch_bounds__(256) void yuv_noise_hist_kernel(const uint8_t* __restrict__ src, uint32_t* __restrict__ dst, int lo, int hi, int W,
                                                           int hb, int wb, int ux, size_t origin, size_t frame_bytes) {
    constexpr int NB = NoiseK<ESZ>::NB, LOW = NoiseK<ESZ>::LOW;
    __shared__ uint32_t low[LOW * 32];
    __shared__ uint32_t hist[NB];
    const int tid = threadIdx.x, t = blockIdx.y, cp = tid & 31;
    for (int i = tid; i < LOW * 32; i += 256) low[i] = 0;
    for (int i = tid; i < NB; i += 256) hist[i] = 0;
    __syncthreads();
    const uint8_t* yp = src + (size_t)t * frame_bytes + origin;           // W: the luma row pitch; origin: the byte offset of block (0, 0)
    const int units = ux * hb;                                            // hb, wb: whole 2 x 2 blocks; ux = ceil(wb / 4) units per block row
    for (int u = blockIdx.x * 256 + tid; u < units; u += gridDim.x * 256) {
        const int by = u / ux, bx0 = (u - by * ux) * 4;
        const int nb = imin(4, wb - bx0);
        const size_t r0 = (size_t)(2 * by) * W + 2 * bx0, r1 = r0 + W;
        int a[8], b[8];
        if (nb == 4) {
            ldn<ESZ, 8>(yp, r0, a);
            ldn<ESZ, 8>(yp, r1, b);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {                                 // pixels 2 bx0 .. 2 (bx0 + nb) - 1 < 2 wb <= W exist; the others are not read
                const bool in = k < 2 * nb;
                a[k] = in ? ld1<ESZ>(yp, r0 + k) : 0;
                b[k] = in ? ld1<ESZ>(yp, r1 + k) : 0;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = a[2 * k], q = a[2 * k + 1], r = b[2 * k], s = b[2 * k + 1];
            const int mn = imin(imin(p, q), imin(r, s)), mx = imax(imax(p, q), imax(r, s));
            if (k < nb && mn > lo && mx < hi) {
                const int d = p - q - r + s, v = d < 0 ? -d : d;          // 0 .. 2 (2^bits - 1) = NB - 1
                if (v < LOW) atomicAdd(&low[v * 32 + cp], 1u);
                else atomicAdd(&hist[v], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* out = dst + (size_t)t * NB;
    for (int i = tid; i < NB; i += 256) {
        uint32_t n = hist[i];
        if (i < LOW) {
#pragma unroll 8
            for (int c = 0; c < 32; ++c) n += low[i * 32 + ((c + i) & 31)];   // rotated by the bin: the lanes of a group read 32 different banks
        }
        if (n) atomicAdd(&out[i], n);
    }
}

// ---- noise histogram by brightness band -------------------------------------------------------------------------------------------------
// yuv_noise_hist_kernel split by the block's brightness: band = (4 (S - 4 lo)) / (hi - lo) with S = a + b + c + d, 0 .. 15 for every block that
// counts (each code is > lo and < hi, so 4 <= S - 4 lo <= 4 (hi - lo) - 4), and v saturated to NBV - 1.  The same units, loads and walk; the
// workgroup's histogram is [16][NBV] words of LDS.  A band is a range of brightness and neighbouring blocks are mostly of one brightness, so a wave's
// adds still meet in a few (band, v) pairs: the bins v < LOW of every band are kept in COPIES copies, copy (lane & (COPIES - 1)) at word
// (band * LOW + v) * COPIES + copy.  At 8 bit COPIES = 32 and the 32 lanes of a lane group hit 32 different banks whatever their bins; at 10 bit
// LOW covers the same range of noise levels (64 bins) and 32 copies of 16 x 64 bins do not fit: 8 copies, neighbouring lanes on different copies, lanes
// 8 apart share one.  The other bins go to the plain array.  Integer sums commute: the result is the same for every geometry and every schedule.
template <int ESZ> struct BandK {
    static constexpr int NBV = ESZ == 1 ? 128 : 512;
    static constexpr int LOW = ESZ == 1 ? 16 : 64;
    static constexpr int COPIES = ESZ == 1 ? 32 : 8;
    static constexpr int LOWW = SN_NLF_BANDS * LOW * COPIES;             // 8192 words at both depths
    static constexpr int HISTW = SN_NLF_BANDS * NBV;                     // 2048 / 8192 words
};

template <int ESZ>
__global__ __launch_bounds__(256) void yuv_noise_hist_bands_kernel(const uint8_t* __restrict__ src, uint32_t* __restrict__ dst, int lo, int hi, int W,
                                                                 int hb, int wb, int ux, size_t origin, size_t frame_bytes) {
    constexpr int NBV = BandK<ESZ>::NBV, LOW = BandK<ESZ>::LOW, COPIES = BandK<ESZ>::COPIES, LOWW = BandK<ESZ>::LOWW, HISTW = BandK<ESZ>::HISTW;
    __shared__ __attribute__((aligned(16))) uint32_t low[LOWW];
    __shared__ __attribute__((aligned(16))) uint32_t hist[HISTW];
    const int tid = threadIdx.x, t = blockIdx.y, cp = tid & (COPIES - 1);
    for (int i = tid; i < LOWW / 4; i += 256) ((uint4*)low)[i] = make_uint4(0u, 0u, 0u, 0u);
    for (int i = tid; i < HISTW / 4; i += 256) ((uint4*)hist)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const uint8_t* yp = src + (size_t)t * frame_bytes + origin;           // as yuv_noise_hist_kernel: W is the luma row pitch, origin the byte offset of block (0, 0)
    const int units = ux * hb;
    const uint32_t span = (uint32_t)(hi - lo);
    for (int u = blockIdx.x * 256 + tid; u < units; u += gridDim.x * 256) {
        const int by = u / ux, bx0 = (u - by * ux) * 4;
        const int nb = imin(4, wb - bx0);
        const size_t r0 = (size_t)(2 * by) * W + 2 * bx0, r1 = r0 + W;
        int a[8], b[8];
        if (nb == 4) {
            ldn<ESZ, 8>(yp, r0, a);
            ldn<ESZ, 8>(yp, r1, b);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {                                 // pixels 2 bx0 .. 2 (bx0 + nb) - 1 < 2 wb <= W exist; the others are not read
                const bool in = k < 2 * nb;
                a[k] = in ? ld1<ESZ>(yp, r0 + k) : 0;
                b[k] = in ? ld1<ESZ>(yp, r1 + k) : 0;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = a[2 * k], q = a[2 * k + 1], r = b[2 * k], s = b[2 * k + 1];
            const int mn = imin(imin(p, q), imin(r, s)), mx = imax(imax(p, q), imax(r, s));
            if (k < nb && mn > lo && mx < hi) {
                const int d = p - q - r + s, v = imin(d < 0 ? -d : d, NBV - 1);
                const int band = (int)((uint32_t)(4 * ((p + q) + (r + s) - 4 * lo)) / span);      // 0 .. 15 (above)
                if (v < LOW) atomicAdd(&low[(band * LOW + v) * COPIES + cp], 1u);
                else atomicAdd(&hist[band * NBV + v], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* out = dst + (size_t)t * HISTW;
    for (int i = tid; i < HISTW; i += 256) {
        uint32_t n = hist[i];
        const int band = i / NBV, v = i - band * NBV;
        if (v < LOW) {
            const uint32_t* c = low + (band * LOW + v) * COPIES;
            const int rot = (i * COPIES) >> 5;                            // consecutive bins start on different copies: the lanes of a group read 32 different banks
#pragma unroll 8
            for (int k = 0; k < COPIES; ++k) n += c[(k + rot) & (COPIES - 1)];
        }
        if (n) atomicAdd(&out[i], n);
    }
}

// ---- noise map from a noise-level function ------------------------------------------------------------------------------------------------
// dst[t][0][y][x] = curve(low-passed luma at (y, x)): the arithmetic is stated in include/shiftnet_hip.h (sn_noise_map_level) and restated in float32 by
// tests/nlf_ref.py.  One launch.  A workgroup of 256 lanes writes a tile of NM_TW x NM_TH = 128 x 32 pixels of the padded plane.  The bilinear
// interpolation of a tile's pixels reads the means of the 16 x 4 blocks of 8 x 8 luma samples under it and of one block more on every side, block
// indices clamped to the picture: NM_GW x NM_GH = 18 x 6 cells.  Step 1: a lane takes one 8-sample row of one cell (one 8 B / 16 B load where
// the address allows it, element-wise otherwise and on the picture's right edge), neighbouring lanes neighbouring cells of the same luma row, and adds
// the row's integer sum to the cell's word in LDS.  Step 2: cell mean = float(sum) / float(count), one correctly rounded division.  Step 3: a lane
// owns 8 x 2 pixels, reads the four means and the two knots of each from LDS and stores 8 elements per row at once where the address allows it.  The 16
// knots arrive as a kernel argument and are put into LDS by 16 lanes, so that the per-pixel lookup is an LDS read and not private memory.
// The luma is read about 1.7 times (108 cells for 64 blocks), mostly from L2; the tile's output is written once.
constexpr int NM_TW = 128, NM_TH = 32, NM_GW = NM_TW / 8 + 2, NM_GH = NM_TH / 8 + 2, NM_CELLS = NM_GW * NM_GH;
struct NlfK { float k[SN_NLF_BANDS]; float lo, scale; };

template <int ESZ>
__global__ __launch_bounds__(256) void noise_map_level_kernel(const uint8_t* __restrict__ src, void* __restrict__ dst, int dt, const NlfK K, const YuvGeo G,
                                                            int Hp, int Wp, int dst_vec) {
    __shared__ int sum[NM_CELLS];
    __shared__ float mean[NM_CELLS];
    __shared__ float kn[SN_NLF_BANDS];
    const int tid = threadIdx.x, t = blockIdx.z;
    const int h = G.h, w = G.w, py = G.py;
    const int nbx = (w + 7) >> 3, nby = (h + 7) >> 3;
    const int X0 = blockIdx.x * NM_TW, Y0 = blockIdx.y * NM_TH;
    // cell (gy, gx) is block (clamp(tby - 1 + gy), clamp(tbx - 1 + gx)).  A tile that lies in the padding altogether looks at the last blocks.
    const int tbx = imin(X0 >> 3, (w - 1) >> 3), tby = imin(Y0 >> 3, (h - 1) >> 3);
    for (int i = tid; i < NM_CELLS; i += 256) sum[i] = 0;
#pragma unroll
    for (int j = 0; j < SN_NLF_BANDS; ++j) if (tid == j) kn[j] = K.k[j];
    __syncthreads();
    const uint8_t* yp = src + (size_t)t * G.frame_bytes + G.oy;
    for (int i = tid; i < NM_CELLS * 8; i += 256) {
        const int gx = i % NM_GW, q = i / NM_GW, r = q & 7, gy = q >> 3;
        const int bx = imin(imax(tbx - 1 + gx, 0), nbx - 1), by = imin(imax(tby - 1 + gy, 0), nby - 1);
        const int x0 = bx * 8, y = by * 8 + r, n = imin(8, w - x0);       // n >= 1: bx < nbx
        if (y < h) {
            const size_t o = (size_t)y * py + x0;
            int s = 0;
            if (n == 8) {
                int v[8];
                ldn<ESZ, 8>(yp, o, v);
                s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
            } else {
                for (int k = 0; k < n; ++k) s += ld1<ESZ>(yp, o + k);
            }
            atomicAdd(&sum[gy * NM_GW + gx], s);
        }
    }
    __syncthreads();
    for (int i = tid; i < NM_CELLS; i += 256) {
        const int gx = i % NM_GW, gy = i / NM_GW;
        const int bx = imin(imax(tbx - 1 + gx, 0), nbx - 1), by = imin(imax(tby - 1 + gy, 0), nby - 1);
        const int cnt = imin(8, w - bx * 8) * imin(8, h - by * 8);
        mean[i] = (float)sum[i] / (float)cnt;
    }
    __syncthreads();
    const int x0 = X0 + (tid & 15) * 8, y0 = Y0 + (tid >> 4) * 2;
    if (x0 >= Wp) return;
    const int n = imin(8, Wp - x0);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = y0 + r;
        if (y >= Hp) break;
        const int ny = 2 * imin(y, h - 1) - 7;                            // (ye - 3.5) / 8 in sixteenths
        const int cy = (ny >> 4) - (tby - 1);                             // the cell above: 0 .. NM_GH - 2
        const float ay = mulr((float)(ny & 15), 0.0625f);
        const float* m0 = mean + cy * NM_GW;
        const float* m1 = m0 + NM_GW;
        float val[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int nx = 2 * imin(x0 + k, w - 1) - 7;
            const int cx = (nx >> 4) - (tbx - 1);                         // the cell to the left: 0 .. NM_GW - 2
            const float ax = mulr((float)(nx & 15), 0.0625f);
            const float top = addr(m0[cx], mulr(ax, subr(m0[cx + 1], m0[cx])));
            const float bot = addr(m1[cx], mulr(ax, subr(m1[cx + 1], m1[cx])));
            const float m = addr(top, mulr(ay, subr(bot, top)));
            const float u = fminf(fmaxf(subr(mulr(subr(m, K.lo), K.scale), 0.5f), 0.f), 15.f);
            const int i = imin((int)u, SN_NLF_BANDS - 2);                  // u >= 0: the conversion is the floor
            const float f = subr(u, (float)i);
            val[k] = addr(kn[i], mulr(f, subr(kn[i + 1], kn[i])));
        }
        st8_any(dst, dt, ((size_t)t * Hp + y) * Wp + x0, dst_vec != 0, n, val);
    }
}

// ---- row and column sums ------------------------------------------------------------------------------------------------------------
// A lane owns 8 consecutive pixels of a row (one 8 B / 16 B load where the ADDRESS allows it, element-wise otherwise and on the right edge, where
// only the pixels inside the frame are read); a wave (blockDim.x = 64: threadIdx.y is the wave) covers 512 consecutive pixels and walks down a strip
// of ROWCOL_STRIP rows.  Per row the lanes' sums are added across the wave and lane 0 adds the wave's sum to rows[t][y]: one integer atomic per
// wave and row.  Each lane keeps 8 column accumulators over the strip and adds them to cols[t][x] at the end: one integer atomic per lane and
// column.  Integer sums commute: the result is the same for every geometry and every schedule.  (16 x 1023 and 512 x 1023 fit an int.)
constexpr int ROWCOL_STRIP = 16;

__device__ __forceinline__ int wave_sum_i(int x) {                         // the sum over the 64 lanes, in every lane
    x += dpp_movi<0xB1>(x);      // quad_perm [1,0,3,2]
    x += dpp_movi<0x4E>(x);      // quad_perm [2,3,0,1]
    x += dpp_movi<0x141>(x);     // row_half_mirror
    x += dpp_movi<0x140>(x);     // row_mirror: the sum of the DPP row of 16
    x += __shfl_xor(x, 16, 64);
    x += __shfl_xor(x, 32, 64);
    return x;
}

template <int ESZ>
__global__ __launch_bounds__(256) void yuv_rowcol_kernel(const uint8_t* __restrict__ src, uint32_t* __restrict__ rows, uint32_t* __restrict__ cols,
                                                       int H, int W, size_t frame_bytes) {
    const int t = blockIdx.z, lane = threadIdx.x;
    const int x0 = (blockIdx.x * 64 + lane) * 8, y0 = (blockIdx.y * 4 + threadIdx.y) * ROWCOL_STRIP;
    if (y0 >= H) return;                                                  // the whole wave: every lane of a wave that stays takes part in the sums
    const uint8_t* yp = src + (size_t)t * frame_bytes;
    const int n = imin(8, W - x0);                                        // <= 0: a lane beyond the right edge reads nothing and adds zeros
    const int y1 = imin(y0 + ROWCOL_STRIP, H);
    int acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0;
    for (int y = y0; y < y1; ++y) {
        int v[8];
        if (n == 8) {
            ldn<ESZ, 8>(yp, (size_t)y * W + x0, v);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = k < n ? ld1<ESZ>(yp, (size_t)y * W + x0 + k) : 0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += v[k];
        const int s = wave_sum_i(((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])));
        if (lane == 0) atomicAdd(&rows[(size_t)t * H + y], (uint32_t)s);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < n) atomicAdd(&cols[(size_t)t * W + x0 + k], (uint32_t)acc[k]);
}

// constants: float64 expressions rounded once to float32 (tests/yuv_ref.py: constants() evaluates the same expressions)
bool make_consts(const sn_yuv_fmt* f, YuvK* K) {
    if (!f || (f->bits != 8 && f->bits != 10) || f->chroma < 0 || f->chroma > 2 || f->matrix < 0 || f->matrix > 1 || f->range < 0 || f->range > 1) return false;
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

size_t frame_bytes_of(const sn_yuv_fmt* f, int H, int W) {
    const size_t esz = f->bits == 8 ? 1 : 2;
    const size_t c = f->chroma == SN_YUV_444 ? (size_t)H * W : (size_t)((H + 1) / 2) * ((W + 1) / 2);
    return ((size_t)H * W + 2 * c) * esz;
}

// The picture of a launch: the whole H x W frame (rect == nullptr) or rect inside it.  false: rect does not lie inside the frame, or at
// 4:2:0 it would share a chroma sample with its surroundings (x0, y0 odd; w or h odd without reaching the frame's far edge).
bool make_geo(const sn_yuv_fmt* f, int H, int W, const sn_yuv_rect* rect, YuvGeo* G) {
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

}  // namespace

extern "C" {

// TAIL: further template arguments after <ESZ, CH>, with their leading comma (empty for the kernels that have none)
#define SN_YUV_DISPATCH_T(KERNEL, TAIL, ...)                                                                                \
    do {                                                                                                                   \
        if (fmt->bits == 8) {                                                                                              \
            if (fmt->chroma == SN_YUV_444) hipLaunchKernelGGL((KERNEL<1, SN_YUV_444 TAIL>), grid, block, 0, s, __VA_ARGS__); \
            else if (fmt->chroma == SN_YUV_420_CENTER) hipLaunchKernelGGL((KERNEL<1, SN_YUV_420_CENTER TAIL>), grid, block, 0, s, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<1, SN_YUV_420_LEFT TAIL>), grid, block, 0, s, __VA_ARGS__);                      \
        } else {                                                                                                           \
            if (fmt->chroma == SN_YUV_444) hipLaunchKernelGGL((KERNEL<2, SN_YUV_444 TAIL>), grid, block, 0, s, __VA_ARGS__); \
            else if (fmt->chroma == SN_YUV_420_CENTER) hipLaunchKernelGGL((KERNEL<2, SN_YUV_420_CENTER TAIL>), grid, block, 0, s, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<2, SN_YUV_420_LEFT TAIL>), grid, block, 0, s, __VA_ARGS__);                      \
        }                                                                                                                  \
    } while (0)
#define SN_YUV_DISPATCH(KERNEL, ...) SN_YUV_DISPATCH_T(KERNEL, , __VA_ARGS__)
#define SN_YUV_TAIL_TPDF , SN_DITHER_TPDF
#define SN_YUV_TAIL_AMOUNT , SN_DITHER_NONE, SN_MIX_AMOUNT
#define SN_YUV_TAIL_AMOUNT_TPDF , SN_DITHER_TPDF, SN_MIX_AMOUNT
#define SN_YUV_TAIL_REMOVED , SN_DITHER_NONE, SN_MIX_REMOVED
#define SN_YUV_TAIL_REMOVED_TPDF , SN_DITHER_TPDF, SN_MIX_REMOVED

static int ingest_yuv(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, void* dst, int dst_dtype, int T, int H, int W, int Hp, int Wp,
                      void* stream) {
    sn_clear_error();
    YuvK K;
    YuvGeo G;
    if (!src || !dst || !make_consts(fmt, &K) || dst_dtype < 0 || dst_dtype > 2 || T < 1 || T > 65535 || H < 1 || W < 1) return SN_EINVAL;
    if (!make_geo(fmt, H, W, rect, &G) || Hp < G.h || Wp < G.w) return SN_EINVAL;
    if (fmt->bits == 10 && ((uintptr_t)src & 1)) return SN_EINVAL;
    const int dst_vec = Wp % 8 == 0 && ((uintptr_t)dst & 15) == 0;       // every 8-pixel span of a row is 16 B (f32: 32 B) aligned
    const dim3 block(32, 8), grid(((Wp + 7) / 8 + 31) / 32, ((Hp + 1) / 2 + 7) / 8, T);
    if (grid.y > 65535) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    SN_YUV_DISPATCH(ingest_yuv_kernel, src, dst, dst_dtype, K, G, Hp, Wp, dst_vec);
    return sn_check_launch();
}

int sn_ingest_yuv(const uint8_t* src, const sn_yuv_fmt* fmt, void* dst, int dst_dtype, int T, int H, int W, int Hp, int Wp, void* stream) {
    return ingest_yuv(src, fmt, nullptr, dst, dst_dtype, T, H, W, Hp, Wp, stream);
}

int sn_ingest_yuv_rect(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, void* dst, int dst_dtype, int T, int H, int W, int Hp, int Wp,
                       void* stream) {
    if (!rect) { sn_clear_error(); return SN_EINVAL; }
    return ingest_yuv(src, fmt, rect, dst, dst_dtype, T, H, W, Hp, Wp, stream);
}

// mix == nullptr: the entry points without _mix, `in` is not looked at
static int egress_yuv(const void* out, int out_dtype, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const sn_yuv_dither* dither, const sn_yuv_mix* mix,
                      const uint8_t* in, uint8_t* dst, int T, int H, int W, int Hp, int Wp, void* stream) {
    sn_clear_error();
    YuvK K;
    YuvGeo G;
    if (!out || !dst || !make_consts(fmt, &K) || out_dtype < 0 || out_dtype > 2 || T < 1 || T > 65535 || H < 1 || W < 1) return SN_EINVAL;
    if (!make_geo(fmt, H, W, rect, &G) || Hp < G.h || Wp < G.w) return SN_EINVAL;
    if (fmt->bits == 10 && ((uintptr_t)dst & 1)) return SN_EINVAL;
    if (mix) {
        if (!in || (fmt->bits == 10 && ((uintptr_t)in & 1))) return SN_EINVAL;
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)dst;
        const size_t bytes = (size_t)T * G.frame_bytes;
        if (a < b + bytes && b < a + bytes) return SN_EINVAL;             // the kernel reads `in` while other lanes write dst
    }
    const int src_vec = Wp % 8 == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 block(32, 8), grid(((G.w + 7) / 8 + 31) / 32, ((G.h + 1) / 2 + 7) / 8, T);
    if (grid.y > 65535) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool tpdf = dither && dither->mode == SN_DITHER_TPDF;
    const DitherK<SN_DITHER_TPDF> D{tpdf ? dither->seed : 0u, tpdf ? (uint32_t)dither->t0 : 0u};
    const DitherK<SN_DITHER_NONE> D0{};
    if (mix && mix->mode == SN_MIX_AMOUNT) {
        const MixK<SN_MIX_AMOUNT> M{in, mix->ay, mix->ac};
        if (tpdf) SN_YUV_DISPATCH_T(egress_yuv_kernel, SN_YUV_TAIL_AMOUNT_TPDF, out, out_dtype, dst, K, G, Hp, Wp, src_vec, D, M);
        else SN_YUV_DISPATCH_T(egress_yuv_kernel, SN_YUV_TAIL_AMOUNT, out, out_dtype, dst, K, G, Hp, Wp, src_vec, D0, M);
    } else if (mix) {
        const MixK<SN_MIX_REMOVED> M{in, mix->ay, mix->ac};
        if (tpdf) SN_YUV_DISPATCH_T(egress_yuv_kernel, SN_YUV_TAIL_REMOVED_TPDF, out, out_dtype, dst, K, G, Hp, Wp, src_vec, D, M);
        else SN_YUV_DISPATCH_T(egress_yuv_kernel, SN_YUV_TAIL_REMOVED, out, out_dtype, dst, K, G, Hp, Wp, src_vec, D0, M);
    } else if (tpdf) {
        SN_YUV_DISPATCH_T(egress_yuv_kernel, SN_YUV_TAIL_TPDF, out, out_dtype, dst, K, G, Hp, Wp, src_vec, D, MixK<SN_MIX_OFF>{});
    } else {
        SN_YUV_DISPATCH(egress_yuv_kernel, out, out_dtype, dst, K, G, Hp, Wp, src_vec, D0, MixK<SN_MIX_OFF>{});
    }
    return sn_check_launch();
}

int sn_egress_yuv(const void* out, int out_dtype, const sn_yuv_fmt* fmt, uint8_t* dst, int T, int H, int W, int Hp, int Wp, void* stream) {
    return egress_yuv(out, out_dtype, fmt, nullptr, nullptr, nullptr, nullptr, dst, T, H, W, Hp, Wp, stream);
}

int sn_egress_yuv_rect(const void* out, int out_dtype, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, uint8_t* dst, int T, int H, int W, int Hp, int Wp,
                       void* stream) {
    if (!rect) { sn_clear_error(); return SN_EINVAL; }
    return egress_yuv(out, out_dtype, fmt, rect, nullptr, nullptr, nullptr, dst, T, H, W, Hp, Wp, stream);
}

static bool bad_dither(const sn_yuv_dither* dither) {
    return (dither->mode != SN_DITHER_NONE && dither->mode != SN_DITHER_TPDF) || dither->t0 < 0;
}

int sn_egress_yuv_dither(const void* out, int out_dtype, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const sn_yuv_dither* dither, uint8_t* dst, int T,
                         int H, int W, int Hp, int Wp, void* stream) {
    if (!dither || bad_dither(dither)) { sn_clear_error(); return SN_EINVAL; }
    return egress_yuv(out, out_dtype, fmt, rect, dither, nullptr, nullptr, dst, T, H, W, Hp, Wp, stream);
}

int sn_egress_yuv_mix(const void* out, int out_dtype, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const sn_yuv_dither* dither, const sn_yuv_mix* mix,
                      const uint8_t* in, uint8_t* dst, int T, int H, int W, int Hp, int Wp, void* stream) {
    const auto finite = [](float v) { return v - v == 0.f; };             // false for NaN and for the infinities
    if ((dither && bad_dither(dither)) || !mix || !in || (mix->mode != SN_MIX_AMOUNT && mix->mode != SN_MIX_REMOVED) || !finite(mix->ay) || !finite(mix->ac) ||
        (mix->mode == SN_MIX_AMOUNT && (mix->ay < 0.f || mix->ay > 1.f || mix->ac < 0.f || mix->ac > 1.f))) { sn_clear_error(); return SN_EINVAL; }
    return egress_yuv(out, out_dtype, fmt, rect, dither, mix, in, dst, T, H, W, Hp, Wp, stream);
}

int sn_yuv_thumb(const uint8_t* src, const sn_yuv_fmt* fmt, uint16_t* dst, int T, int H, int W, void* stream) {
    sn_clear_error();
    if (!src || !dst || !fmt || (fmt->bits != 8 && fmt->bits != 10) || fmt->chroma < 0 || fmt->chroma > 2 || T < 1 || T > 65535 || H < 1 || W < 1) return SN_EINVAL;
    if (((uintptr_t)dst & 1) || (fmt->bits == 10 && ((uintptr_t)src & 1))) return SN_EINVAL;
    const size_t fb = frame_bytes_of(fmt, H, W);
    const int hb = (H + 7) / 8, wb = (W + 7) / 8;
    const dim3 block(32, 8), grid((wb + 31) / 32, (hb + 7) / 8, T);
    if (grid.y > 65535) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (fmt->bits == 8) hipLaunchKernelGGL((yuv_thumb_kernel<1>), grid, block, 0, s, src, dst, H, W, hb, wb, fb);
    else hipLaunchKernelGGL((yuv_thumb_kernel<2>), grid, block, 0, s, src, dst, H, W, hb, wb, fb);
    return sn_check_launch();
}

static int noise_hist(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, uint32_t* dst, int lo, int hi, int T, int H, int W, void* stream) {
    sn_clear_error();
    if (!src || !dst || !fmt || (fmt->bits != 8 && fmt->bits != 10) || fmt->chroma < 0 || fmt->chroma > 2 || T < 1 || T > 65535 || H < 1 || W < 1 || lo > hi) return SN_EINVAL;
    if (((uintptr_t)dst & 3) || (fmt->bits == 10 && ((uintptr_t)src & 1))) return SN_EINVAL;
    YuvGeo G;
    if (!make_geo(fmt, H, W, rect, &G)) return SN_EINVAL;
    const size_t fb = G.frame_bytes;
    const int nbins = fmt->bits == 8 ? NoiseK<1>::NB : NoiseK<2>::NB;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(dst, 0, (size_t)T * nbins * sizeof(uint32_t), s) != hipSuccess) return sn_check_launch();      // dst is overwritten, not added to
    const int hb = G.h / 2, wb = G.w / 2, ux = (wb + 3) / 4;               // the block grid is anchored at the picture's first sample
    if (hb < 1 || wb < 1) return sn_check_launch();                        // no whole block: all-zero histograms
    const long long units = (long long)ux * hb;
    if (units > 0x7fffffffLL - 1024 * 256) return SN_EINVAL;
    // about 8 units (32 blocks) per lane: the zeroing, the sum of the copies and the flush are paid once per 8192 blocks and a 720p frame is 29 workgroups
    const int gx = (int)((units + 2047) / 2048 < 1024 ? (units + 2047) / 2048 : 1024);
    const dim3 block(256), grid(gx, T);
    if (fmt->bits == 8) hipLaunchKernelGGL((yuv_noise_hist_kernel<1>), grid, block, 0, s, src, dst, lo, hi, W, hb, wb, ux, G.oy, fb);
    else hipLaunchKernelGGL((yuv_noise_hist_kernel<2>), grid, block, 0, s, src, dst, lo, hi, W, hb, wb, ux, G.oy, fb);
    return sn_check_launch();
}

int sn_yuv_noise_hist(const uint8_t* src, const sn_yuv_fmt* fmt, uint32_t* dst, int lo, int hi, int T, int H, int W, void* stream) {
    return noise_hist(src, fmt, nullptr, dst, lo, hi, T, H, W, stream);
}

int sn_yuv_noise_hist_rect(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, uint32_t* dst, int lo, int hi, int T, int H, int W,
                           void* stream) {
    if (!rect) { sn_clear_error(); return SN_EINVAL; }
    return noise_hist(src, fmt, rect, dst, lo, hi, T, H, W, stream);
}

int sn_yuv_noise_hist_bands(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, uint32_t* dst, int lo, int hi, int T, int H, int W,
                            void* stream) {
    sn_clear_error();
    if (!src || !dst || !fmt || (fmt->bits != 8 && fmt->bits != 10) || fmt->chroma < 0 || fmt->chroma > 2 || T < 1 || T > 65535 || H < 1 || W < 1 || lo > hi) return SN_EINVAL;
    if (lo < -(1 << 24) || hi > (1 << 24)) return SN_EINVAL;               // the band is 32-bit arithmetic: 4 (S - 4 lo) must fit
    if (((uintptr_t)dst & 3) || (fmt->bits == 10 && ((uintptr_t)src & 1))) return SN_EINVAL;
    YuvGeo G;
    if (!make_geo(fmt, H, W, rect, &G)) return SN_EINVAL;
    const int words = fmt->bits == 8 ? BandK<1>::HISTW : BandK<2>::HISTW;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(dst, 0, (size_t)T * words * sizeof(uint32_t), s) != hipSuccess) return sn_check_launch();     // dst is overwritten, not added to
    const int hb = G.h / 2, wb = G.w / 2, ux = (wb + 3) / 4;               // the block grid of sn_yuv_noise_hist_rect
    if (hb < 1 || wb < 1) return sn_check_launch();                        // no whole block: all-zero histograms
    const long long units = (long long)ux * hb;
    if (units > 0x7fffffffLL - 1024 * 256) return SN_EINVAL;
    // about 16 units (64 blocks) per lane: the zeroing and the flush of 40 / 64 KB of LDS are paid once per 16384 blocks and a 720p frame is 15 workgroups
    const int gx = (int)((units + 4095) / 4096 < 1024 ? (units + 4095) / 4096 : 1024);
    const dim3 block(256), grid(gx, T);
    if (fmt->bits == 8) hipLaunchKernelGGL((yuv_noise_hist_bands_kernel<1>), grid, block, 0, s, src, dst, lo, hi, W, hb, wb, ux, G.oy, G.frame_bytes);
    else hipLaunchKernelGGL((yuv_noise_hist_bands_kernel<2>), grid, block, 0, s, src, dst, lo, hi, W, hb, wb, ux, G.oy, G.frame_bytes);
    return sn_check_launch();
}

int sn_noise_map_level(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const float* knots, int lo, int hi, void* dst, int dst_dtype,
                       int T, int H, int W, int Hp, int Wp, void* stream) {
    sn_clear_error();
    if (!src || !dst || !knots || !fmt || (fmt->bits != 8 && fmt->bits != 10) || fmt->chroma < 0 || fmt->chroma > 2 || dst_dtype < 0 || dst_dtype > 2 ||
        T < 1 || T > 65535 || H < 1 || W < 1 || lo >= hi) return SN_EINVAL;
    if (lo < -(1 << 24) || hi > (1 << 24)) return SN_EINVAL;               // float(lo) is exact
    if (fmt->bits == 10 && ((uintptr_t)src & 1)) return SN_EINVAL;
    YuvGeo G;
    if (!make_geo(fmt, H, W, rect, &G) || Hp < G.h || Wp < G.w) return SN_EINVAL;
    NlfK K;
    for (int i = 0; i < SN_NLF_BANDS; ++i) {
        if (!(knots[i] == knots[i]) || knots[i] - knots[i] != 0.f) return SN_EINVAL;      // NaN, infinity
        K.k[i] = knots[i];
    }
    K.lo = (float)lo;
    K.scale = (float)(16.0 / ((double)hi - (double)lo));                   // a float64 expression rounded once, as the constants of make_consts
    const int dst_vec = Wp % 8 == 0 && ((uintptr_t)dst & 15) == 0;       // every 8-pixel span of a row is 16 B (f32: 32 B) aligned
    const dim3 block(256), grid((Wp + NM_TW - 1) / NM_TW, (Hp + NM_TH - 1) / NM_TH, T);
    if (grid.y > 65535) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (fmt->bits == 8) hipLaunchKernelGGL((noise_map_level_kernel<1>), grid, block, 0, s, src, dst, dst_dtype, K, G, Hp, Wp, dst_vec);
    else hipLaunchKernelGGL((noise_map_level_kernel<2>), grid, block, 0, s, src, dst, dst_dtype, K, G, Hp, Wp, dst_vec);
    return sn_check_launch();
}

int sn_yuv_rowcol_sums(const uint8_t* src, const sn_yuv_fmt* fmt, uint32_t* rows, uint32_t* cols, int T, int H, int W, void* stream) {
    sn_clear_error();
    if (!src || !rows || !cols || !fmt || (fmt->bits != 8 && fmt->bits != 10) || fmt->chroma < 0 || fmt->chroma > 2 || T < 1 || T > 65535 || H < 1 || W < 1 ||
        H > 65535 || W > 65535) return SN_EINVAL;
    if (((uintptr_t)rows & 3) || ((uintptr_t)cols & 3) || (fmt->bits == 10 && ((uintptr_t)src & 1))) return SN_EINVAL;
    const size_t fb = frame_bytes_of(fmt, H, W);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(rows, 0, (size_t)T * H * sizeof(uint32_t), s) != hipSuccess) return sn_check_launch();       // both are overwritten, not added to
    if (hipMemsetAsync(cols, 0, (size_t)T * W * sizeof(uint32_t), s) != hipSuccess) return sn_check_launch();
    const dim3 block(64, 4), grid((W + 511) / 512, (H + 4 * ROWCOL_STRIP - 1) / (4 * ROWCOL_STRIP), T);
    if (fmt->bits == 8) hipLaunchKernelGGL((yuv_rowcol_kernel<1>), grid, block, 0, s, src, rows, cols, H, W, fb);
    else hipLaunchKernelGGL((yuv_rowcol_kernel<2>), grid, block, 0, s, src, rows, cols, H, W, fb);
    return sn_check_launch();
}

}  // extern "C"
