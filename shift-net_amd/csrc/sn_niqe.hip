// The per-pixel part of NIQE (Mittal, Soundararajan, Bovik: "Making a 'Completely Blind' Image Quality Analyzer", 2013) on the luma plane of planar
// Y'CbCr payloads (gfx950): the payloads are those of csrc/sn_yuv.hip, the chroma planes are not read, and of the format only the bit depth and the
// range decide anything.
//
//   sn_yuv_niqe_sums : T payloads -> [T][2][nbh][nbw][5][5] doubles: per frame, scale (1, 2) and 96 x 96 block of the picture's top-left 96 nbh x 96 nbw
//                      samples, five sums of each of five maps -- the locally normalised luma and its products with four neighbours -- from which
//                      shiftnet_amd/niqe.py fits the block's 18 features per scale on the host, in float64.
//
// The arithmetic is stated in include/shiftnet_hip.h and restated in float64 by tests/niqe_ref.py: float32 with every product and sum rounded separately
// (contraction is off for this file: no FMA) up to the map value m, float64 from there on.
//
// One workgroup of 256 lanes owns one (frame, scale, block): blockIdx = (block, scale - 1, frame).  A block of scale S has side B = 96 / S, and its B x B
// normalised coefficients have to be in LDS together (36 KB at scale 1), because the four products reach across the block with a wrap.  Beside them the
// workgroup filters in strips of NQ_R = 16 rows:
//   1. stage: the strip's NQ_R + 6 rows (3 rows of halo above and below) of B + 8 samples (4 to the left and to the right: the filter needs 3, and
//      with 4 a lane loads a group of 4 samples -- at scale 2 the 2 x 8 luma samples under them -- that lies wholly inside or wholly outside the cropped
//      picture, whose width is a multiple of 96).  Inside it is one 4 B / 8 B (scale 2: two of 8 B / 16 B) load where the ADDRESS allows it, element-wise
//      otherwise; outside the group is the replicated edge sample.  Rows are clamped to the cropped picture of that scale in the same way.  Scale 2 is
//      computed here, from the payload: there is no half-size image in memory.
//   2. rows: the horizontal 7-tap sums of I and of I * I of all NQ_R + 6 rows;
//   3. columns: the vertical 7-tap sums of those, mu and m2, and n = (I - mu) / (sqrt(|m2 - mu mu|) + 1) into the block's coefficients.
// Consecutive lanes take consecutive samples of a row in all three steps: LDS addresses are consecutive words, no bank conflicts beyond the row ends.
// LDS: 36 864 B coefficients + 9 152 B strip + 2 x 8 448 B row sums + 800 B for the reduction = 63 712 B, static, under the 64 KB a workgroup gets
// without dynamic LDS; two workgroups fit a CU's 160 KiB.
// Then the sums: lane l takes the samples l, l + 256, ... of the block in row-major order, forms the five map values of each (four LDS reads of
// neighbours, indices wrapped inside the block) and keeps 10 integer counts and 15 double sums in registers; the 25 values are added across the wave by
// cross-lane moves in a fixed butterfly, across the four waves through LDS in a fixed order, and lanes 0 .. 24 store the block's 25 doubles with plain
// stores.  No atomics, and every double is the result of one fixed sequence of operations whatever the grid looks like and whenever the workgroup runs:
// the result does not depend on the launch geometry or the schedule, and two launches give the same bits -- not because the sums commute, as the
// integer sums of csrc/sn_yuv_stats.hip do, but because nothing about the order is left open.
#include "sn_yuv.h"
#pragma clang fp contract(off)

namespace {

constexpr int NQ_R = 16;                                                  // rows of a strip; divides 96 and 48
constexpr int NQ_ROWS = NQ_R + 6;                                         // with the halo
constexpr int NQ_SW = SN_NIQE_BLOCK + 8;                                  // the strip's row pitch at scale 1, in samples
constexpr int NQ_VALS = SN_NIQE_MAPS * SN_NIQE_SUMS;
static_assert(SN_NIQE_BLOCK % (2 * NQ_R) == 0 && SN_NIQE_BLOCK % 8 == 0, "strips and sample groups tile a block at both scales");

struct NiqeK {
    float g[7];                                                           // filled by the kernel from win7
    float scale;                                                          // v = offset + code * scale
    float offset;
};

// the value of a luma code on the 16 .. 235 scale: limited range code * 2^-(bits - 8) (offset 0: exact), full range 16 + code * (219 / (2^bits - 1))
__device__ __forceinline__ float niqe_value(int code, float scale, float offset) { return addr(offset, mulr((float)code, scale)); }

// 4 consecutive samples of scale S from (row y, column x0) of that scale's picture, all inside the crop
template <int ESZ, int S>
__device__ __forceinline__ void niqe_load4(const uint8_t* yp, int py, int y, int x0, float scale, float offset, float* v) {
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
            const float v00 = niqe_value(a[2 * k], scale, offset), v01 = niqe_value(a[2 * k + 1], scale, offset);
            const float v10 = niqe_value(b[2 * k], scale, offset), v11 = niqe_value(b[2 * k + 1], scale, offset);
            v[k] = mulr(0.25f, addr(addr(v00, v01), addr(v10, v11)));
        }
    }
}

// the seven products of a 7-tap sum, added from the outside in: the small outer taps first and the centre tap last.  With the taps of NIQE's window a
// constant picture then filters to exactly itself (the float32 taps add up to 1 in this order; from tap 0 upwards they give 1 + 2^-23), so a flat area has
// coefficients of exactly zero at both scales instead of a rounding residue of one sign
__device__ __forceinline__ float niqe_sum7(const float* t) { return addr(addr(addr(addr(t[0], t[6]), addr(t[1], t[5])), addr(t[2], t[4])), t[3]); }

__device__ __forceinline__ double wave_sum_d(double x) {                   // the sum over the 64 lanes in a fixed butterfly, in every lane
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

template <int ESZ, int S>
__device__ __forceinline__ void niqe_block(const uint8_t* yp, int py, int hs, int ws, int by, int bx, const NiqeK& K, float* coef, float* strip, float* h1,
                                           float* h2, double* part, double* out) {
    constexpr int B = SN_NIQE_BLOCK / S, SW = B + 8, GROUPS = SW / 4;
    const int tid = threadIdx.x;
    const int Y0 = by * B, X0 = bx * B;                                   // the block's first sample in the hs x ws picture of scale S
    for (int y0 = 0; y0 < B; y0 += NQ_R) {
        // 1. stage rows Y0 + y0 - 3 .. + NQ_R + 2, columns X0 - 4 .. X0 + B + 3, clamped to the cropped picture
        for (int i = tid; i < NQ_ROWS * GROUPS; i += 256) {
            const int r = i / GROUPS, g = i - r * GROUPS;
            const int y = imin(imax(Y0 + y0 - 3 + r, 0), hs - 1), x0 = X0 - 4 + 4 * g;      // x0 is a multiple of 4 and so is ws: a group is in or out
            float v[4];
            if (x0 >= 0 && x0 < ws) {
                niqe_load4<ESZ, S>(yp, py, y, x0, K.scale, K.offset, v);
            } else {                                                      // the replicated edge sample: the first of the first group, or the last of the last
                float e[4];
                niqe_load4<ESZ, S>(yp, py, y, x0 < 0 ? 0 : ws - 4, K.scale, K.offset, e);
                v[0] = v[1] = v[2] = v[3] = x0 < 0 ? e[0] : e[3];
            }
            *(float4*)(strip + r * SW + 4 * g) = make_float4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        // 2. the row sums: sample x of the block is strip column x + 4
        for (int i = tid; i < NQ_ROWS * B; i += 256) {
            const int r = i / B, x = i - r * B;
            const float* p = strip + r * SW + x + 1;
            float a[7], q[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                a[k] = mulr(K.g[k], p[k]);
                q[k] = mulr(K.g[k], mulr(p[k], p[k]));
            }
            h1[i] = niqe_sum7(a);
            h2[i] = niqe_sum7(q);
        }
        __syncthreads();
        // 3. the column sums and the coefficient
        for (int i = tid; i < NQ_R * B; i += 256) {
            const int r = i / B, x = i - r * B;
            const float* p1 = h1 + r * B + x;
            const float* p2 = h2 + r * B + x;
            float a[7], q[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                a[k] = mulr(K.g[k], p1[k * B]);
                q[k] = mulr(K.g[k], p2[k * B]);
            }
            const float mu = niqe_sum7(a), m2 = niqe_sum7(q);
            const float v = strip[(r + 3) * SW + x + 4];
            coef[(y0 + r) * B + x] = subr(v, mu) / addr(sqrtf(fabsf(subr(m2, mulr(mu, mu)))), 1.f);
        }
        __syncthreads();                                                  // the next strip overwrites strip, h1 and h2; after the last one coef is complete
    }
    // the five maps and their sums
    int neg[SN_NIQE_MAPS], pos[SN_NIQE_MAPS];
    double sn[SN_NIQE_MAPS], sp[SN_NIQE_MAPS], sa[SN_NIQE_MAPS];
#pragma unroll
    for (int k = 0; k < SN_NIQE_MAPS; ++k) { neg[k] = 0; pos[k] = 0; sn[k] = 0.; sp[k] = 0.; sa[k] = 0.; }
    for (int i = tid; i < B * B; i += 256) {
        const int y = i / B, x = i - y * B;
        const int yu = y == 0 ? B - 1 : y - 1, xl = x == 0 ? B - 1 : x - 1, xr = x == B - 1 ? 0 : x + 1;
        const float n = coef[i];
        const float m[SN_NIQE_MAPS] = {n, mulr(n, coef[y * B + xl]), mulr(n, coef[yu * B + x]), mulr(n, coef[yu * B + xl]), mulr(n, coef[yu * B + xr])};
#pragma unroll
        for (int k = 0; k < SN_NIQE_MAPS; ++k) {
            const double d = (double)m[k], q = d * d;
            if (m[k] < 0.f) { neg[k] += 1; sn[k] += q; }
            if (m[k] > 0.f) { pos[k] += 1; sp[k] += q; }
            sa[k] += fabs(d);
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
    if (tid < NQ_VALS) out[tid] = (part[tid] + part[NQ_VALS + tid]) + (part[2 * NQ_VALS + tid] + part[3 * NQ_VALS + tid]);
}

template <int ESZ>
__global__ __launch_bounds__(256) void yuv_niqe_sums_kernel(const uint8_t* __restrict__ src, const float* __restrict__ win7, double* __restrict__ dst, int py,
                                                          int nbh, int nbw, float scale, float offset, size_t origin, size_t frame_bytes) {
    __shared__ __attribute__((aligned(16))) float coef[SN_NIQE_BLOCK * SN_NIQE_BLOCK];
    __shared__ __attribute__((aligned(16))) float strip[NQ_ROWS * NQ_SW];
    __shared__ float h1[NQ_ROWS * SN_NIQE_BLOCK];
    __shared__ float h2[NQ_ROWS * SN_NIQE_BLOCK];
    __shared__ double part[4 * NQ_VALS];
    const int blk = blockIdx.x, s = blockIdx.y, t = blockIdx.z;           // s: 0 is scale 1, 1 is scale 2
    const int by = blk / nbw, bx = blk - by * nbw;
    NiqeK K;
#pragma unroll
    for (int k = 0; k < 7; ++k) K.g[k] = win7[k];
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
    float scale, offset = 0.f;
    if (fmt->range == SN_YUV_FULL) {                                       // a float64 expression rounded once, as the constants of make_consts
        scale = (float)(219.0 / (double)((1 << fmt->bits) - 1));
        offset = 16.f;
    } else {
        scale = fmt->bits == 8 ? 1.f : 0.25f;
    }
    const dim3 block(256), grid((unsigned)(nbh * nbw), 2, T);
    hipStream_t s = (hipStream_t)stream;
    with_esz(fmt, [&](auto esz) {
        hipLaunchKernelGGL((yuv_niqe_sums_kernel<esz()>), grid, block, 0, s, src, win7, dst, G.py, nbh, nbw, scale, offset, G.oy, G.frame_bytes);
    });
    return sn_check_launch();
}

}  // extern "C"
