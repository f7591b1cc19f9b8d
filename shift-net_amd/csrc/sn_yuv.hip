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
//   sn_ingest_yuv_rect / sn_egress_yuv_rect : the first two restricted to a picture rectangle of the stream.  They are the same kernels: every
//                   kernel sees "its frame" as h x w samples whose planes have a row pitch and a first sample of their own (YuvGeo, sn_yuv.h);
//                   the entry points without _rect pass the whole frame.
// The statistics the restorer takes from the same payloads' luma are another unit, csrc/sn_yuv_stats.hip.
//
// The arithmetic (order of operations, constants) is stated in include/shiftnet_hip.h and restated in float32 by tests/yuv_ref.py,
// which these kernels equal bit for bit.  Every float product and sum is rounded separately (contraction is off for this file: no
// FMA); the chroma upsampling is integer arithmetic and therefore exact.
//
// Both are bandwidth kernels.  A thread owns four horizontally adjacent 2x2 luma blocks (8 x 2 pixels), so that every chroma sample is
// produced once and the 8 pixels of a row are one 8 / 16 B load and one 16 / 2 x 16 B store where the address is aligned; a thread
// whose span is not aligned, or touches the frame edge or the padding, takes the element-wise path with the same arithmetic.
#include "sn_yuv_color.h"
#pragma clang fp contract(off)

namespace {

// ---- RGB tensor elements ---------------------------------------------------------------------------------------------------
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

// ---- ingest (the chroma numerators and the matrix: sn_yuv_color.h) ----------------------------------------------------------------------
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
// The dither of a launch.  DITHER is a template parameter of the kernel: SN_DITHER_NONE carries nothing and every line below that touches a
// key is dead in it, so the instantiations the entry points without _dither launch are the ones they launched before there was a dither.
template <int DITHER> struct DitherK { static constexpr int mode = DITHER; };
template <> struct DitherK<SN_DITHER_TPDF> { static constexpr int mode = SN_DITHER_TPDF; uint32_t seed; uint32_t t0; };
template <int DITHER> __device__ __forceinline__ uint32_t dither_frame_key(const DitherK<DITHER>&, int) { return 0u; }
template <> __device__ __forceinline__ uint32_t dither_frame_key<SN_DITHER_TPDF>(const DitherK<SN_DITHER_TPDF>& D, int t) {
    return hash_frame_key(D.seed, D.t0 + (uint32_t)t);
}
// the sample at column x of that row (the keys and the hash: sn_yuv_color.h): two 12-bit fields of it summed to a triangle on (-1, 1); exact in float32
__device__ __forceinline__ float dither_tpdf(uint32_t rk, int x) {
    const uint32_t k = hash_sample(rk, x);
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
template <int MIX> struct MixK { static constexpr int mode = MIX; const uint8_t* in; float ay, ac; };   // in: T payloads laid out as dst; AMOUNT: the amounts, REMOVED: the gains
template <> struct MixK<SN_MIX_OFF> { static constexpr int mode = SN_MIX_OFF; };
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

}  // namespace

extern "C" {

static int ingest_yuv(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, void* dst, int dst_dtype, int T, int H, int W, int Hp, int Wp,
                      void* stream) {
    sn_clear_error();
    YuvK K;
    YuvGeo G;
    if (!valid_payloads(src, fmt, T, H, W) || !dst || !make_consts(fmt, &K) || dst_dtype < 0 || dst_dtype > 2) return SN_EINVAL;
    if (!make_geo(fmt, H, W, rect, &G) || Hp < G.h || Wp < G.w) return SN_EINVAL;
    const int dst_vec = Wp % 8 == 0 && ((uintptr_t)dst & 15) == 0;       // every 8-pixel span of a row is 16 B (f32: 32 B) aligned
    const dim3 block(32, 8), grid(((Wp + 7) / 8 + 31) / 32, ((Hp + 1) / 2 + 7) / 8, T);
    if (grid.y > 65535) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    with_esz_chroma(fmt, [&](auto esz, auto ch) {
        hipLaunchKernelGGL((ingest_yuv_kernel<esz(), ch()>), grid, block, 0, s, src, dst, dst_dtype, K, G, Hp, Wp, dst_vec);
    });
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
    if (!out || !valid_payloads(dst, fmt, T, H, W) || !make_consts(fmt, &K) || out_dtype < 0 || out_dtype > 2) return SN_EINVAL;
    if (!make_geo(fmt, H, W, rect, &G) || Hp < G.h || Wp < G.w) return SN_EINVAL;
    if (mix) {
        if (!in || !aligned_payload(fmt, in)) return SN_EINVAL;
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)dst;
        const size_t bytes = (size_t)T * G.frame_bytes;
        if (a < b + bytes && b < a + bytes) return SN_EINVAL;             // the kernel reads `in` while other lanes write dst
    }
    const int src_vec = Wp % 8 == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 block(32, 8), grid(((G.w + 7) / 8 + 31) / 32, ((G.h + 1) / 2 + 7) / 8, T);
    if (grid.y > 65535) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool tpdf = dither && dither->mode == SN_DITHER_TPDF;
    // D: a DitherK, M: a MixK.  Their modes are the kernel's last two template arguments: SN_DITHER_NONE and SN_MIX_OFF are the instantiations of sn_egress_yuv
    const auto launch = [&](auto D, auto M) {
        with_esz_chroma(fmt, [&](auto esz, auto ch) {
            hipLaunchKernelGGL((egress_yuv_kernel<esz(), ch(), decltype(D)::mode, decltype(M)::mode>), grid, block, 0, s, out, out_dtype, dst, K, G, Hp, Wp,
                               src_vec, D, M);
        });
    };
    const auto with_dither = [&](auto M) {
        if (tpdf) launch(DitherK<SN_DITHER_TPDF>{dither->seed, (uint32_t)dither->t0}, M); else launch(DitherK<SN_DITHER_NONE>{}, M);
    };
    if (!mix) with_dither(MixK<SN_MIX_OFF>{});
    else if (mix->mode == SN_MIX_AMOUNT) with_dither(MixK<SN_MIX_AMOUNT>{in, mix->ay, mix->ac});
    else with_dither(MixK<SN_MIX_REMOVED>{in, mix->ay, mix->ac});
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

}  // extern "C"
