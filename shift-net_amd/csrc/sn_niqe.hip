// The per-pixel part of NIQE (Mittal, Soundararajan, Bovik: "Making a 'Completely Blind' Image Quality Analyzer", 2013) on the luma plane of planar
// Y'CbCr payloads (gfx950): the payloads are those of csrc/sn_yuv.hip, the chroma planes are not read, and of the format only the bit depth and the
// range decide anything.
//
//   sn_yuv_niqe_sums : T payloads -> [T][2][nbh][nbw][5][5] doubles: per frame, scale (1, 2) and 96 x 96 block of the picture's top-left 96 nbh x 96 nbw
//                      samples, five sums of each of five maps -- the locally normalised luma and its products with four neighbours -- from which
//                      shiftnet_amd/niqe.py fits the block's 18 features per scale on the host, in float64.
//
// The arithmetic is stated in include/shiftnet_hip.h and restated by tests/niqe_ref.py: float64 from the codes on, every product and sum rounded
// separately (contraction is off for this file: no FMA).  It was float32 up to the map value, on the values themselves: I * I reaches 55 000, where a
// float32 ulp is 2^-8, and on the near-flat areas a denoiser writes (variances of 0.1 to 1) m2 - mu mu had lost its digits -- sums 8e-3 from the
// reference where the tests allowed 2e-5 -- and a flat area of some codes (49, 98, 125, 196) left a residue of one sign.  Three things
// changed together:
//   * float64.  A value is exact in it (code times a 24-bit constant) and so is the 2 x 2 mean of scale 2.
//   * Per workgroup the filters run on J = I - p, the deviations from the block's own first sample p = I(Y0, X0): I - mu and m2 - mu mu do not
//     change under a shift, J is exact, and J J is a hundred to ten thousand times smaller than I I.  In a flat area J = 0, so every product and sum
//     is 0 and n = 0 / (0 + 1) = 0 at every code, whatever the taps add up to.  Halo samples that belong to a neighbouring block use this block's p.
//   * The taps are the float32 taps widened and divided by their own 7-tap sum.  The float32 roundings of NIQE's window add up to 1 - 5.6e-9; where
//     J is not small (a block whose first sample is dark and whose other half is bright) that deficit times J is an offset of mu of one sign, and the
//     sums came out 2.3e-4 from the reference.  Divided by their sum the taps add up to 1 to an ulp and what is left is the rounding of each tap:
//     3e-8 of the sums, on every kind of frame.
//
// One workgroup of NQ_T = 512 lanes owns one (frame, scale, block): blockIdx = (block, scale - 1, frame).  A block of scale S has side B = 96 / S, and
// its B x B normalised coefficients have to be in LDS together (72 KB of doubles at scale 1), because the four products reach across the block with
// a wrap.  Beside them the workgroup filters in strips of NQ_R = 16 rows:
//   1. stage: the strip's NQ_R + 6 rows (3 rows of halo above and below) of B + 8 samples (4 to the left and to the right: the filter needs 3, and
//      with 4 a lane loads a group of 4 samples -- at scale 2 the 2 x 8 luma samples under them -- that lies wholly inside or wholly outside the cropped
//      picture, whose width is a multiple of 96).  Inside it is one 4 B / 8 B (scale 2: two of 8 B / 16 B) load where the ADDRESS allows it, element-wise
//      otherwise; outside the group is the replicated edge sample.  Rows are clamped to the cropped picture of that scale in the same way.  Scale 2 is
//      computed here, from the payload: there is no half-size image in memory.  What is stored is J.
//   2. rows: the horizontal 7-tap sums of J and of J * J of all NQ_R + 6 rows;
//   3. columns: the vertical 7-tap sums of those, mu and m2, and n = (J - mu) / (sqrt(|m2 - mu mu|) + 1) into the block's coefficients, as doubles.
// Consecutive lanes take consecutive samples of a row in all three steps: LDS addresses are consecutive doubles, no bank conflicts beyond the row ends.
// LDS: 73 728 B coefficients + 18 304 B strip + 2 x 16 896 B row sums + 1 600 B for the reduction = 127 424 B, static: one workgroup per CU's 160 KiB,
// which is why it has 512 lanes (two waves per SIMD) where the float32 kernel had two workgroups of 256.
// Then the sums: lane l takes the samples l, l + NQ_T, ... of the block in row-major order, forms the five map values of each (four LDS reads of
// neighbours, indices wrapped inside the block) and keeps 10 integer counts and 15 double sums in registers; the 25 values are added across the wave by
// cross-lane moves in a fixed butterfly, across the eight waves through LDS in a fixed order, and lanes 0 .. 24 store the block's 25 doubles with plain
// stores.  No atomics, and every double is the result of one fixed sequence of operations whatever the grid looks like and whenever the workgroup runs:
// the result does not depend on the launch geometry or the schedule, and two launches give the same bits -- not because the sums commute, as the
// integer sums of csrc/sn_yuv_stats.hip do, but because nothing about the order is left open.
#include "sn_yuv.h"
#include <cmath>
#pragma clang fp contract(off)

namespace {

#ifndef SN_NIQE_LANES
#define SN_NIQE_LANES 512                                                 // one-off builds for A/B runs may set another multiple of 64
#endif
constexpr int NQ_T = SN_NIQE_LANES;                                       // lanes of a workgroup
constexpr int NQ_W = NQ_T / 64;                                           // its waves
constexpr int NQ_R = 16;                                                  // rows of a strip; divides 96 and 48
constexpr int NQ_ROWS = NQ_R + 6;                                         // with the halo
constexpr int NQ_SW = SN_NIQE_BLOCK + 8;                                  // the strip's row pitch at scale 1, in samples
constexpr int NQ_VALS = SN_NIQE_MAPS * SN_NIQE_SUMS;
static_assert(SN_NIQE_BLOCK % (2 * NQ_R) == 0 && SN_NIQE_BLOCK % 8 == 0, "strips and sample groups tile a block at both scales");
static_assert(NQ_T % 64 == 0 && NQ_T >= 64 && NQ_T <= 1024 && NQ_T >= NQ_VALS, "whole waves, and a lane per value of the result");

struct NiqeK {
    double g[7];                                                          // filled by the kernel from win7
    double scale;                                                         // v = offset + code * scale
    double offset;
};

// the value of a luma code on the 16 .. 235 scale: limited range code * 2^-(bits - 8) (offset 0), full range 16 + code * (219 / (2^bits - 1)), the
// constant rounded to float32: a product of a 10-bit and a 24-bit number and a sum that fits 53 bits -- both exact
__device__ __forceinline__ double niqe_value(int code, double scale, double offset) { return offset + (double)code * scale; }

// 4 consecutive samples of scale S from (row y, column x0) of that scale's picture, all inside the crop
template <int ESZ, int S>
__device__ __forceinline__ void niqe_load4(const uint8_t* yp, int py, int y, int x0, double scale, double offset, double* v) {
    if constexpr (S == 1) {
        int c[4];
        ldn<ESZ, 4>(yp, (size_t)y * py + x0, c);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = niqe_value(c[k], scale, offset);
    } else {
        int a[8], b[8];
        ldn<ESZ, 8>(yp, (size_t)(2 * y) * py + 2 * x0, a);
        ldn<ESZ, 8>(yp, (size_t)(2 * y + 1) * py + 2 * x0, b);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double v00 = niqe_value(a[2 * k], scale, offset), v01 = niqe_value(a[2 * k + 1], scale, offset);
            const double v10 = niqe_value(b[2 * k], scale, offset), v11 = niqe_value(b[2 * k + 1], scale, offset);
            v[k] = 0.25 * ((v00 + v01) + (v10 + v11));
        }
    }
}

// the seven products of a 7-tap sum, added from the outside in: the small outer taps first and the centre tap last
__device__ __forceinline__ double niqe_sum7(const double* t) { return (((t[0] + t[6]) + (t[1] + t[5])) + (t[2] + t[4])) + t[3]; }

__device__ __forceinline__ double wave_sum_d(double x) {                   // the sum over the 64 lanes in a fixed butterfly, in every lane
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

template <int ESZ, int S>
__device__ __forceinline__ void niqe_block(const uint8_t* yp, int py, int hs, int ws, int by, int bx, const NiqeK& K, double* coef, double* strip, double* h1,
                                           double* h2, double* part, double* out) {
    constexpr int B = SN_NIQE_BLOCK / S, SW = B + 8, GROUPS = SW / 4;
    const int tid = threadIdx.x;
    const int Y0 = by * B, X0 = bx * B;                                   // the block's first sample in the hs x ws picture of scale S
    double piv[4];
    niqe_load4<ESZ, S>(yp, py, Y0, X0, K.scale, K.offset, piv);           // X0 is a multiple of 4: a group inside the crop
    const double p = piv[0];                                              // the pivot: the same in every lane
    for (int y0 = 0; y0 < B; y0 += NQ_R) {
        // 1. stage rows Y0 + y0 - 3 .. + NQ_R + 2, columns X0 - 4 .. X0 + B + 3, clamped to the cropped picture, minus the pivot
        for (int i = tid; i < NQ_ROWS * GROUPS; i += NQ_T) {
            const int r = i / GROUPS, g = i - r * GROUPS;
            const int y = imin(imax(Y0 + y0 - 3 + r, 0), hs - 1), x0 = X0 - 4 + 4 * g;      // x0 is a multiple of 4 and so is ws: a group is in or out
            double v[4];
            if (x0 >= 0 && x0 < ws) {
                niqe_load4<ESZ, S>(yp, py, y, x0, K.scale, K.offset, v);
            } else {                                                      // the replicated edge sample: the first of the first group, or the last of the last
                double e[4];
                niqe_load4<ESZ, S>(yp, py, y, x0 < 0 ? 0 : ws - 4, K.scale, K.offset, e);
                v[0] = v[1] = v[2] = v[3] = x0 < 0 ? e[0] : e[3];
            }
            double* q = strip + r * SW + 4 * g;
            *(double2*)q = make_double2(v[0] - p, v[1] - p);
            *(double2*)(q + 2) = make_double2(v[2] - p, v[3] - p);
        }
        __syncthreads();
        // 2. the row sums: sample x of the block is strip column x + 4
        for (int i = tid; i < NQ_ROWS * B; i += NQ_T) {
            const int r = i / B, x = i - r * B;
            const double* q0 = strip + r * SW + x + 1;
            double a[7], q[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const double j = q0[k];
                a[k] = K.g[k] * j;
                q[k] = K.g[k] * (j * j);
            }
            h1[i] = niqe_sum7(a);
            h2[i] = niqe_sum7(q);
        }
        __syncthreads();
        // 3. the column sums and the coefficient
        for (int i = tid; i < NQ_R * B; i += NQ_T) {
            const int r = i / B, x = i - r * B;
            const double* p1 = h1 + r * B + x;
            const double* p2 = h2 + r * B + x;
            double a[7], q[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                a[k] = K.g[k] * p1[k * B];
                q[k] = K.g[k] * p2[k * B];
            }
            const double mu = niqe_sum7(a), m2 = niqe_sum7(q);
            const double j = strip[(r + 3) * SW + x + 4];
            coef[(y0 + r) * B + x] = (j - mu) / (sqrt(fabs(m2 - mu * mu)) + 1.);
        }
        __syncthreads();                                                  // the next strip overwrites strip, h1 and h2; after the last one coef is complete
    }
    // the five maps and their sums
    int neg[SN_NIQE_MAPS], pos[SN_NIQE_MAPS];
    double sn[SN_NIQE_MAPS], sp[SN_NIQE_MAPS], sa[SN_NIQE_MAPS];
#pragma unroll
    for (int k = 0; k < SN_NIQE_MAPS; ++k) { neg[k] = 0; pos[k] = 0; sn[k] = 0.; sp[k] = 0.; sa[k] = 0.; }
    for (int i = tid; i < B * B; i += NQ_T) {
        const int y = i / B, x = i - y * B;
        const int yu = y == 0 ? B - 1 : y - 1, xl = x == 0 ? B - 1 : x - 1, xr = x == B - 1 ? 0 : x + 1;
        const double n = coef[i];
        const double m[SN_NIQE_MAPS] = {n, n * coef[y * B + xl], n * coef[yu * B + x], n * coef[yu * B + xl], n * coef[yu * B + xr]};
#pragma unroll
        for (int k = 0; k < SN_NIQE_MAPS; ++k) {
            const double q = m[k] * m[k];
            if (m[k] < 0.) { neg[k] += 1; sn[k] += q; }
            if (m[k] > 0.) { pos[k] += 1; sp[k] += q; }
            sa[k] += fabs(m[k]);
        }
    }
    double v[NQ_VALS];
#pragma unroll
    for (int k = 0; k < SN_NIQE_MAPS; ++k) {
        v[5 * k] = (double)neg[k]; v[5 * k + 1] = sn[k]; v[5 * k + 2] = (double)pos[k]; v[5 * k + 3] = sp[k]; v[5 * k + 4] = sa[k];
    }
#pragma unroll
    for (int k = 0; k < NQ_VALS; ++k) v[k] = wave_sum_d(v[k]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NQ_VALS; ++k) part[(tid >> 6) * NQ_VALS + k] = v[k];
    }
    __syncthreads();
    if (tid < NQ_VALS) {                                                  // wave 0 first, the last wave last
        double s = part[tid];
        for (int w = 1; w < NQ_W; ++w) s += part[w * NQ_VALS + tid];
        out[tid] = s;
    }
}

template <int ESZ>
__global__ __launch_bounds__(NQ_T) void yuv_niqe_sums_kernel(const uint8_t* __restrict__ src, const float* __restrict__ win7, double* __restrict__ dst, int py,
                                                           int nbh, int nbw, double scale, double offset, size_t origin, size_t frame_bytes) {
    __shared__ __attribute__((aligned(16))) double coef[SN_NIQE_BLOCK * SN_NIQE_BLOCK];
    __shared__ __attribute__((aligned(16))) double strip[NQ_ROWS * NQ_SW];
    __shared__ double h1[NQ_ROWS * SN_NIQE_BLOCK];
    __shared__ double h2[NQ_ROWS * SN_NIQE_BLOCK];
    __shared__ double part[NQ_W * NQ_VALS];
    const int blk = blockIdx.x, s = blockIdx.y, t = blockIdx.z;           // s: 0 is scale 1, 1 is scale 2
    const int by = blk / nbw, bx = blk - by * nbw;
    NiqeK K;
    double w[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) w[k] = (double)win7[k];
    const double wsum = niqe_sum7(w);                                     // the widened taps over their own sum: they add up to 1 to an ulp
#pragma unroll
    for (int k = 0; k < 7; ++k) K.g[k] = w[k] / wsum;
    K.scale = scale;
    K.offset = offset;
    const uint8_t* yp = src + (size_t)t * frame_bytes + origin;           // py: the luma row pitch; origin: the byte offset of the picture's first sample
    double* out = dst + ((((size_t)t * 2 + s) * nbh + by) * nbw + bx) * NQ_VALS;
    if (s == 0) niqe_block<ESZ, 1>(yp, py, SN_NIQE_BLOCK * nbh, SN_NIQE_BLOCK * nbw, by, bx, K, coef, strip, h1, h2, part, out);
    else niqe_block<ESZ, 2>(yp, py, SN_NIQE_BLOCK / 2 * nbh, SN_NIQE_BLOCK / 2 * nbw, by, bx, K, coef, strip, h1, h2, part, out);
}

}  // namespace

extern "C" {

int sn_yuv_niqe_sums(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const float* win7, double* dst, int T, int H, int W, void* stream) {
    sn_clear_error();
    if (!valid_payloads(src, fmt, T, H, W) || !win7 || ((uintptr_t)win7 & 3) || !dst || ((uintptr_t)dst & 7)) return SN_EINVAL;
    YuvGeo G;
    if (!make_geo(fmt, H, W, rect, &G)) return SN_EINVAL;
    const int nbh = G.h / SN_NIQE_BLOCK, nbw = G.w / SN_NIQE_BLOCK;       // whole blocks of the picture's top-left corner: the rest is not read
    if (nbh < 1 || nbw < 1) return SN_EINVAL;                              // no block, no sums
    if ((long long)nbh * nbw > 0x7fffffffLL) return SN_EINVAL;             // a grid dimension
    double scale, offset = 0.;
    if (fmt->range == SN_YUV_FULL) {                                       // a float64 expression rounded once to float32, as the constants of make_consts
        scale = (double)(float)(219.0 / (double)((1 << fmt->bits) - 1));
        offset = 16.;
    } else {
        scale = fmt->bits == 8 ? 1. : 0.25;
    }
    const dim3 block(NQ_T), grid((unsigned)(nbh * nbw), 2, T);
    hipStream_t s = (hipStream_t)stream;
    with_esz(fmt, [&](auto esz) {
        hipLaunchKernelGGL((yuv_niqe_sums_kernel<esz()>), grid, block, 0, s, src, win7, dst, G.py, nbh, nbw, scale, offset, G.oy, G.frame_bytes);
    });
    return sn_check_launch();
}

}  // extern "C"
