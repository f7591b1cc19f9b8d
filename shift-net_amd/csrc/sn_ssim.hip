// Full-reference quality on the luma plane of planar Y'CbCr payloads (gfx950): SSIM (Wang, Bovik, Sheikh, Simoncelli: "Image quality assessment: from
// error visibility to structural similarity", 2004) of two sets of payloads, as the Y-channel SSIM of the evaluation harnesses defines it -- an 11 x 11
// Gaussian window of sigma 1.5, the border replicated, every position counted.  The payloads are those of csrc/sn_yuv.hip, the chroma planes are not
// read, and of the format only the bit depth decides anything.  (PSNR needs no kernel of its own: sn_yuv_diff_stats of csrc/sn_yuv_stats.hip has the
// exact sums of squared differences of all three planes.)
//
//   sn_yuv_ssim_sums : two sets of T payloads -> [T][nty][ntx] doubles: per frame and SN_SSIM_TILE x SN_SSIM_TILE tile of the picture, the sum of the
//                      SSIM map over the tile's positions; shiftnet_amd/fullref.py adds the tiles and divides by h w on the host, in float64.
//
// The arithmetic is stated in include/shiftnet_hip.h and restated by tests/ssim_ref.py: float64 from the codes on, every product and sum rounded
// separately (contraction is off for this file: no FMA).  It was float32 up to the map value, on codes minus mid-grey: on near-flat areas far from
// mid-grey G(a a) - G(a)^2 is tiny against its terms and is divided by something close to C2, and a frame of code 2 with one code of noise came out
// 2e-5 from the reference, a tile 6e-5 -- beyond the 1e-5 the header promises.  In float64 the codes need no centring (a product of two 16-bit
// words is exact) and the frame's SSIM is within 1e-12 of the float64 restatement.
//
// One workgroup of 256 lanes owns one (frame, tile): blockIdx = (tile, 0, frame).
//   1. stage: the tile's SN_SSIM_TILE + 10 rows (5 rows of halo above and below) of SN_SSIM_TILE + 16 samples of a and of b into LDS, as float32 codes
//      (exact).  8 columns to the left and to the right: the filter needs 5, and with 8 a lane loads a group of 4 samples that starts at a
//      multiple of 4 of the picture -- one 4 B / 8 B load where the group lies inside the picture and the ADDRESS allows it, element-wise with clamped
//      coordinates otherwise.  Rows are clamped to the picture in the same way: the replication is at the picture's edge, not at the frame's.
//   2. rows: the horizontal 11-tap sums of the five maps a, b, a a, b b, a b of all SN_SSIM_TILE + 10 rows, float64, into LDS;
//   3. columns: the vertical 11-tap sums of those into registers, four positions per lane, the map value of each, and the lane's float64 sum over its
//      positions inside the picture.
// Consecutive lanes take consecutive samples of a row in steps 2 and 3: LDS addresses are consecutive words, no bank conflicts beyond the row ends.
// LDS: 2 x 8 064 B staged windows + 5 x 10 752 B row sums + 32 B for the reduction = 69 920 B, static; two workgroups fit a CU's 160 KiB.
// The lane sums are added across the wave by cross-lane moves in a fixed butterfly, across the four waves through LDS in a fixed order, and lane 0 stores
// the tile's double with a plain store.  No atomics, and the double is the result of one fixed sequence of operations whatever the grid looks like and
// whenever the workgroup runs: two launches give the same bits, as sn_yuv_niqe_sums (csrc/sn_niqe.hip) guarantees for its sums.
#include "sn_yuv.h"
#include <cmath>
#pragma clang fp contract(off)

namespace {

constexpr int SS_T = SN_SSIM_TILE;
constexpr int SS_TAPS = 11, SS_HALO = SS_TAPS / 2;
constexpr int SS_ROWS = SS_T + 2 * SS_HALO;                               // staged and row-filtered rows
constexpr int SS_LEFT = 8;                                                // staged columns left (and right) of the tile
constexpr int SS_SW = SS_T + 2 * SS_LEFT;                                 // the staged window's row pitch, in samples
constexpr int SS_GROUPS = SS_SW / 4;
static_assert(SS_T % 4 == 0 && SS_LEFT % 4 == 0 && SS_LEFT >= SS_HALO, "a group of 4 staged samples starts at a multiple of 4 of the picture");
static_assert((SS_T * SS_T) % 256 == 0, "every lane takes the same number of positions");

struct SsimK {
    double g[SS_TAPS];                                                    // the window's separable factor
    double c1, c2;                                                        // (0.01 p)^2, (0.03 p)^2, p = 2^bits - 1
};

// the eleven products of an 11-tap sum, added from the outside in: the small outer taps first, the centre tap last
__device__ __forceinline__ double ssim_sum11(const double* t) {
    return (((((t[0] + t[10]) + (t[1] + t[9])) + (t[2] + t[8])) + (t[3] + t[7])) + (t[4] + t[6])) + t[5];
}

__device__ __forceinline__ double ssim_wave_sum(double x) {                // the sum over the 64 lanes in a fixed butterfly, in every lane
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// rows Y0 - 5 .. Y0 + SS_T + 4, columns X0 - 8 .. X0 + SS_T + 7 of one luma plane, clamped to the h x w picture
template <int ESZ>
__device__ __forceinline__ void ssim_stage(const uint8_t* yp, int py, int h, int w, int Y0, int X0, float* win) {
    for (int i = threadIdx.x; i < SS_ROWS * SS_GROUPS; i += 256) {
        const int r = i / SS_GROUPS, g = i - r * SS_GROUPS;
        const int y = imin(imax(Y0 - SS_HALO + r, 0), h - 1), x0 = X0 - SS_LEFT + 4 * g;
        int c[4];
        if (x0 >= 0 && x0 + 3 < w) {
            ldn<ESZ, 4>(yp, (size_t)y * py + x0, c);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = ld1<ESZ>(yp, (size_t)y * py + imin(imax(x0 + k, 0), w - 1));
        }
        *(float4*)(win + r * SS_SW + 4 * g) = make_float4((float)c[0], (float)c[1], (float)c[2], (float)c[3]);
    }
}

template <int ESZ>
__global__ __launch_bounds__(256) void yuv_ssim_sums_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, double* __restrict__ dst,
                                                          YuvGeo G, int ntx, int tiles, SsimK K) {
    __shared__ __attribute__((aligned(16))) float wa[SS_ROWS * SS_SW];
    __shared__ __attribute__((aligned(16))) float wb[SS_ROWS * SS_SW];
    __shared__ double rows[5][SS_ROWS * SS_T];
    __shared__ double part[4];
    const int tid = threadIdx.x, tile = blockIdx.x, t = blockIdx.z;
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int Y0 = ty * SS_T, X0 = tx * SS_T;                             // the tile's first position in the h x w picture
    ssim_stage<ESZ>(a + (size_t)t * G.frame_bytes + G.oy, G.py, G.h, G.w, Y0, X0, wa);
    ssim_stage<ESZ>(b + (size_t)t * G.frame_bytes + G.oy, G.py, G.h, G.w, Y0, X0, wb);
    __syncthreads();
    // 2. the row sums of the five maps: position x of the tile is staged column x + SS_LEFT, its first tap SS_HALO to the left of that
    for (int i = tid; i < SS_ROWS * SS_T; i += 256) {
        const int r = i / SS_T, x = i - r * SS_T;
        const float* pa = wa + r * SS_SW + x + (SS_LEFT - SS_HALO);
        const float* pb = wb + r * SS_SW + x + (SS_LEFT - SS_HALO);
        double va[SS_TAPS], vb[SS_TAPS], vaa[SS_TAPS], vbb[SS_TAPS], vab[SS_TAPS];
#pragma unroll
        for (int k = 0; k < SS_TAPS; ++k) {
            const double ea = (double)pa[k], eb = (double)pb[k];
            va[k] = K.g[k] * ea;
            vb[k] = K.g[k] * eb;
            vaa[k] = K.g[k] * (ea * ea);
            vbb[k] = K.g[k] * (eb * eb);
            vab[k] = K.g[k] * (ea * eb);
        }
        rows[0][i] = ssim_sum11(va);
        rows[1][i] = ssim_sum11(vb);
        rows[2][i] = ssim_sum11(vaa);
        rows[3][i] = ssim_sum11(vbb);
        rows[4][i] = ssim_sum11(vab);
    }
    __syncthreads();
    // 3. the column sums, the map, the lane's sum over its positions inside the picture
    double sum = 0.;
    for (int i = tid; i < SS_T * SS_T; i += 256) {
        const int y = i / SS_T, x = i - y * SS_T;
        double m[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const double* p = rows[q] + y * SS_T + x;
            double v[SS_TAPS];
#pragma unroll
            for (int k = 0; k < SS_TAPS; ++k) v[k] = K.g[k] * p[k * SS_T];
            m[q] = ssim_sum11(v);
        }
        const double mab = m[0] * m[1], maa = m[0] * m[0], mbb = m[1] * m[1];
        const double saa = m[2] - maa, sbb = m[3] - mbb, sab = m[4] - mab;
        const double num = (2. * mab + K.c1) * (2. * sab + K.c2);
        const double den = ((maa + mbb) + K.c1) * ((saa + sbb) + K.c2);
        if (Y0 + y < G.h && X0 + x < G.w) sum += num / den;
    }
    sum = ssim_wave_sum(sum);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) dst[(size_t)t * tiles + tile] = (part[0] + part[1]) + (part[2] + part[3]);
}

}  // namespace

extern "C" {

int sn_yuv_ssim_sums(const uint8_t* a, const uint8_t* b, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, double* dst, int T, int H, int W, void* stream) {
    sn_clear_error();
    if (!valid_payloads(a, fmt, T, H, W) || !b || !aligned_payload(fmt, b) || !dst || ((uintptr_t)dst & 7)) return SN_EINVAL;
    YuvGeo G;
    if (!make_geo(fmt, H, W, rect, &G)) return SN_EINVAL;
    const int nty = (G.h - 1) / SS_T + 1, ntx = (G.w - 1) / SS_T + 1;      // ceil, without leaving int at 2^31 - 1
    if ((long long)nty * ntx > 0x7fffffffLL - 1024 * 256) return SN_EINVAL;      // the bound sn_yuv_diff_stats puts on its units; the tile index is a grid dimension
    SsimK K;
    double g[SS_TAPS], s = 0.;
    for (int i = 0; i < SS_TAPS; ++i) { g[i] = std::exp(-(double)((i - SS_HALO) * (i - SS_HALO)) / (2.0 * 1.5 * 1.5)); s += g[i]; }
    for (int i = 0; i < SS_TAPS; ++i) K.g[i] = g[i] / s;
    const double p = (double)((1 << fmt->bits) - 1);
    K.c1 = (0.01 * p) * (0.01 * p);
    K.c2 = (0.03 * p) * (0.03 * p);
    const dim3 block(256), grid((unsigned)(nty * ntx), 1, T);
    hipStream_t st = (hipStream_t)stream;
    with_esz(fmt, [&](auto esz) { hipLaunchKernelGGL((yuv_ssim_sums_kernel<esz()>), grid, block, 0, st, a, b, dst, G, ntx, nty * ntx, K); });
    return sn_check_launch();
}

}  // extern "C"
