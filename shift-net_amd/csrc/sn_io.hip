// I/O edges of the inference CLIs on the device (gfx950): uint8 frames in, uint8 frames + PSNR sums out.
//
// Upstream converts on the host (inference/test_deblur.py:191-200 numpy2tensor: uint8 HWC -> float64 -> CHW -> float32
// -> x 1/255 -> stack), ships float32 over PCIe (12 B per pixel) and casts on the GPU (:134 in_tensor.half()); results
// come back as float frames for skimage PSNR against the uint8 ground truth (:139-143) and cv2.imwrite (:152).
// Here the uint8 frames cross PCIe (3 B per pixel) and both conversions are HBM-bound kernels:
//   sn_ingest_u8 : [T][H][W][3] u8 -> [T][3][H][W] of the module dtype, value = round_dtype(float(v) * (1/255))  -- bit
//                  identical to numpy2tensor(...).to(dtype);
//   sn_egress_u8 : [T][3][H][W] of the module dtype -> clamp(0,1) * 255 -> (a) [T][H][W][3] u8, rounded to nearest even
//                  like cv2.imwrite's saturate_cast, (b) per-frame sums of squared error of the UNROUNDED value against
//                  the uint8 ground truth (what skimage's PSNR with data_range=255 is computed from), as deterministic
//                  per-workgroup partial sums.
#include "sn_common.h"
#include "../../include/shiftnet_hip.h"
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void ingest_u8_kernel(const uint8_t* __restrict__ src, void* dst, int dt, int HW) {
    const int t = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const uint8_t* s = src + ((size_t)t * HW + i) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) st_any(dst, dt, ((size_t)t * 3 + c) * HW + i, (float)s[c] * (1.0f / 255.0f));
}

#define SN_EGRESS_BLOCKS 64
__global__ __launch_bounds__(256) void egress_u8_kernel(const void* __restrict__ out, int dt, const uint8_t* __restrict__ gt,
                                                      uint8_t* __restrict__ img, float* sse, int HW) {
    __shared__ float red[4];
    const int t = blockIdx.y, tid = threadIdx.x;
    float acc = 0.f;
    for (int i = blockIdx.x * 256 + tid; i < HW; i += SN_EGRESS_BLOCKS * 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = ld_any(out, dt, ((size_t)t * 3 + c) * HW + i);
            v = fminf(fmaxf(v, 0.f), 1.f) * 255.0f;
            const size_t o = ((size_t)t * HW + i) * 3 + c;
            if (img) img[o] = (uint8_t)__float2int_rn(v);
            if (gt) { const float d = v - (float)gt[o]; acc = fmaf(d, d, acc); }
        }
    }
    acc = sum_rows4(row_sum16(acc));
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0 && sse) sse[(size_t)t * SN_EGRESS_BLOCKS + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace

// ---- the CLIs' SSIM (inference/test_deblur.py:25-49) on the device ----------------------------------------------------------
// ssim_calculate(img1, img2): a = img1 / 255, b = img2 / 255 as (C,H,W) float32 volumes; mu = G(a), G(b); sigma = G(a*a) - mu^2,
// G(b*b) - mu^2, G(a*b) - mu1*mu2 with G = scipy.ndimage.gaussian_filter(sd = 1.5): a separable 13-tap Gaussian (radius
// int(4 * 1.5 + 0.5) = 6) along ALL THREE axes -- the 3-channel axis included -- with 'reflect' boundaries (d c b a | a b c d | d c b a);
// the result is the mean of the SSIM map over the volume.
//
// The arithmetic is scipy's and numpy's, rounding for rounding.  gaussian_filter filters one axis after the other in the order C, H, W;
// along an axis it multiplies and adds in float64 with float64 taps and stores the line in the array's dtype, float32.  So do the kernels:
// the five float32 statistics a, b, a a, b b, a b, then per axis a float64 sum of 13 taps rounded ONCE to float32 -- the C axis pointwise (its
// 13 taps folded onto the 3 channels by the reflection: a 3x3 matrix), the H axis from the centre tap and then the pairs from the outside in
// as scipy's symmetric loop adds them, both in the first kernel and stored to scratch; the W axis the same way in the second kernel, which
// then forms the SSIM map in float32 with every product, sum and difference rounded on its own as numpy does (contraction is off from here
// to the end of the file: no FMA) and reduces it deterministically.  What differs from the CLI's number is the order of sums WITHIN float64
// (the folded C axis) and of the final mean (float64 per lane and workgroup here, float32 pairwise there).
// Float32 taps and sums, which this replaced, biased G(a a) - G(a)^2 on near-flat bright frames: +1.5e-4 at code 250 with one code of noise.
#pragma clang fp contract(off)

namespace {

struct SsimW { double g[13]; double m[3][3]; };

__device__ __forceinline__ int reflect_idx(int i, int n) {     // scipy 'reflect' (half-sample symmetric), any distance
    const int period = 2 * n;
    int m = i % period; if (m < 0) m += period;
    return m < n ? m : period - 1 - m;
}

// the 15 planes (channel c, statistic q -> c * 5 + q) of one pixel after the C-axis pass
__device__ __forceinline__ void ssim_cpass(const void* __restrict__ out, int dt, const uint8_t* __restrict__ gt, size_t t, size_t HW, size_t pix,
                                           const SsimW& K, float* f) {
    float s[3][5];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float a = ld_any(out, dt, (t * 3 + c) * HW + pix);
        a = (fminf(fmaxf(a, 0.f), 1.f) * 255.0f) / 255.0f;                      // the CLI: clamp(0,1) * 255, then / 255 inside ssim_calculate
        const float b = (float)gt[(t * HW + pix) * 3 + c] / 255.0f;
        s[c][0] = a; s[c][1] = b; s[c][2] = a * a; s[c][3] = b * b; s[c][4] = a * b;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < 5; ++q) f[c * 5 + q] = (float)((K.m[c][0] * (double)s[0][q] + K.m[c][1] * (double)s[1][q]) + K.m[c][2] * (double)s[2][q]);
}

// C and H axes: one lane per pixel, the C-axis pass of the 13 rows it needs recomputed (pointwise, and these kernels are negligible next to a forward)
__global__ __launch_bounds__(256) void ssim_chpass_kernel(const void* __restrict__ out, int dt, const uint8_t* __restrict__ gt, float* __restrict__ tmp,
                                                        const SsimW K, int H, int W) {
    const int t = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const size_t HW = (size_t)H * W;
    float f0[15], f1[15];
    double acc[15];
    ssim_cpass(out, dt, gt, t, HW, (size_t)y * W + x, K, f0);
#pragma unroll
    for (int p = 0; p < 15; ++p) acc[p] = (double)f0[p] * K.g[6];
    for (int j = 6; j >= 1; --j) {
        ssim_cpass(out, dt, gt, t, HW, (size_t)reflect_idx(y - j, H) * W + x, K, f0);
        ssim_cpass(out, dt, gt, t, HW, (size_t)reflect_idx(y + j, H) * W + x, K, f1);
#pragma unroll
        for (int p = 0; p < 15; ++p) acc[p] += ((double)f0[p] + (double)f1[p]) * K.g[6 - j];
    }
#pragma unroll
    for (int p = 0; p < 15; ++p) tmp[(((size_t)t * 15 + p) * H + y) * W + x] = (float)acc[p];
}

__device__ __forceinline__ double ssim_wave_sum(double x) {     // the sum over the 64 lanes in a fixed butterfly, in every lane
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

#define SN_SSIM_BLOCKS 128
// W axis, the map, the sum: a frame is walked in passes of SN_SSIM_BLOCKS * 256 pixels
__global__ __launch_bounds__(256) void ssim_wpass_kernel(const float* __restrict__ tmp, float* partial, const SsimW K, int H, int W) {
    __shared__ double red[4];
    const int t = blockIdx.y, tid = threadIdx.x;
    const int HW = H * W;
    const float c1 = (float)(0.01 * 0.01), c2 = (float)(0.03 * 0.03);          // numpy: the Python floats 0.01 ** 2, 0.03 ** 2 taken to float32
    double acc = 0.;
    for (int i = blockIdx.x * 256 + tid; i < HW; i += SN_SSIM_BLOCKS * 256) {
        const int y = i / W, x = i - y * W;
        int xl[6], xr[6];
#pragma unroll
        for (int j = 1; j <= 6; ++j) { xl[j - 1] = reflect_idx(x - j, W); xr[j - 1] = reflect_idx(x + j, W); }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float f[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const float* base = tmp + ((size_t)t * 15 + c * 5 + q) * HW + (size_t)y * W;
                double sm = (double)base[x] * K.g[6];
#pragma unroll
                for (int j = 6; j >= 1; --j) sm += ((double)base[xl[j - 1]] + (double)base[xr[j - 1]]) * K.g[6 - j];
                f[q] = (float)sm;
            }
            const float mu1 = f[0], mu2 = f[1];
            const float m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
            const float s1 = f[2] - m11, s2 = f[3] - m22, s12 = f[4] - m12;
            const float num = ((2.f * mu1) * mu2 + c1) * (2.f * s12 + c2);
            const float den = ((m11 + m22) + c1) * ((s1 + s2) + c2);
            acc += (double)(num / den);
        }
    }
    acc = ssim_wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[(size_t)t * SN_SSIM_BLOCKS + blockIdx.x] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}

}  // namespace

extern "C" {

int sn_ssim_blocks(void) { return SN_SSIM_BLOCKS; }

int sn_ssim_u8(const void* out, int out_dtype, const uint8_t* gt, float* scratch, float* partial, int T, int H, int W, void* stream) {
    sn_clear_error();
    if (!out || !gt || !scratch || !partial || out_dtype < 0 || out_dtype > 2 || T < 1 || H < 1 || W < 1) return SN_EINVAL;
    SsimW K;
    double g[13], sum = 0.0;
    for (int k = -6; k <= 6; ++k) { g[k + 6] = exp(-0.5 / (1.5 * 1.5) * (double)(k * k)); sum += g[k + 6]; }      // scipy _gaussian_kernel1d(1.5, 0, 6)
    for (int k = 0; k < 13; ++k) K.g[k] = g[k] / sum;
    for (int c = 0; c < 3; ++c) {
        double m[3] = {0.0, 0.0, 0.0};
        for (int k = -6; k <= 6; ++k) {
            int i = (c + k) % 6; if (i < 0) i += 6;
            m[i < 3 ? i : 5 - i] += g[k + 6] / sum;
        }
        for (int j = 0; j < 3; ++j) K.m[c][j] = m[j];
    }
    hipLaunchKernelGGL(ssim_chpass_kernel, dim3((W + 255) / 256, H, T), dim3(256), 0, (hipStream_t)stream, out, out_dtype, gt, scratch, K, H, W);
    hipLaunchKernelGGL(ssim_wpass_kernel, dim3(SN_SSIM_BLOCKS, T), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, partial, K, H, W);
    return sn_check_launch();
}

int sn_ingest_u8(const uint8_t* src, void* dst, int dst_dtype, int T, int H, int W, void* stream) {
    sn_clear_error();
    if (!src || !dst || dst_dtype < 0 || dst_dtype > 2 || T < 1 || H < 1 || W < 1) return SN_EINVAL;
    const int hw = H * W;
    hipLaunchKernelGGL(ingest_u8_kernel, dim3((hw + 255) / 256, T), dim3(256), 0, (hipStream_t)stream, src, dst, dst_dtype, hw);
    return sn_check_launch();
}

int sn_egress_blocks(void) { return SN_EGRESS_BLOCKS; }

int sn_egress_u8(const void* out, int out_dtype, const uint8_t* gt, uint8_t* img, float* sse, int T, int H, int W, void* stream) {
    sn_clear_error();
    if (!out || out_dtype < 0 || out_dtype > 2 || T < 1 || H < 1 || W < 1 || (gt && !sse) || (!img && !gt)) return SN_EINVAL;
    hipLaunchKernelGGL(egress_u8_kernel, dim3(SN_EGRESS_BLOCKS, T), dim3(256), 0, (hipStream_t)stream, out, out_dtype, gt, img, sse, H * W);
    return sn_check_launch();
}

}  // extern "C"
