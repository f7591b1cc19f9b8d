// The cross-fade of the video restorer's overlapping windows (shiftnet_amd/restore.py, VideoRestorer(window_overlap=V)): the first V frames of a
// window's float32 result are blended with the last V frames of its predecessor's, which restored the same stream frames.
//
//   sn_time_crossfade : prev [V][C][Hp][Wp] f32 (read only), cur [V][C][Hp][Wp] f32 (in place), weights w_prev[V] and w_cur[V] f32:
//                       cur = (w_prev[j] * prev) + (w_cur[j] * cur) on every sample of frame j;
//                       with sq [V][C] u64: sq[j][c] += sum over the h x w picture of q * q, q = rint(clamp(prev - cur, +-8) * 65536), taken before the blend.
//
// The arithmetic is stated in include/shiftnet_hip.h and restated by tests/time_ref.py, which this kernel equals bit for bit.  Every float product
// and sum is rounded separately (contraction is off for this file: no FMA), as in sn_tile.hip and for the same reason.
//
// A bandwidth kernel: 12 bytes moved per sample (prev read, cur read, cur write) and three float operations.  One thread owns 4 consecutive samples
// of a row; where the addresses of its 4 samples in both tensors are 16-byte aligned it moves them as one float4 each way, otherwise sample by sample
// with the same arithmetic.  The test is on the address itself: with a plane of odd size every other plane starts off the 16-byte grid.  Wave64: a
// wave covers 256 consecutive samples of one row, a workgroup 4 rows; the plane, j * C + c, is the grid's z.
// The statistic is a template argument: the instantiation that runs with sq == NULL has none of it.  With it a thread accumulates its q * q in 64
// bits, the wave adds them with cross-lane moves, the four waves through 4 words of LDS, and the workgroup issues ONE 64-bit vector atomic add to its
// plane's word.  Integer sums commute: the result does not depend on the launch geometry or the schedule.
#include "sn_common.h"
#pragma clang fp contract(off)

namespace {

constexpr int TIME_VEC = 4;        // samples per thread
constexpr int TIME_ROWS = 4;       // rows per workgroup (blockDim.y)

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long x) {      // the sum over the 64 lanes, in every lane
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// q * q of one sample's difference, taken before the blend; fmaxf / fminf return the other operand for a NaN, so a NaN difference counts as -8
__device__ __forceinline__ unsigned long long seam_sq(float p, float c) {
    const float d = p - c;
    const long long q = (long long)__builtin_rintf(fminf(fmaxf(d, -8.f), 8.f) * 65536.f);      // |q| <= 2^19: exact in float32 and in the product
    return (unsigned long long)(q * q);
}

template <bool STAT>
__global__ __launch_bounds__(64 * TIME_ROWS) void time_crossfade_kernel(const float* __restrict__ prev, float* __restrict__ cur,
                                                                        const float* __restrict__ w_prev, const float* __restrict__ w_cur,
                                                                        unsigned long long* __restrict__ sq, int C, int Hp, int Wp, int h, int w) {
    __shared__ unsigned long long part[TIME_ROWS];
    const long long x = ((long long)blockIdx.x * 64 + threadIdx.x) * TIME_VEC;      // 64 bit: the last workgroup of a very wide plane passes 2^31
    const size_t z = blockIdx.z;                                                   // the plane: j * C + c in both tensors
    const int j = (int)(z / (size_t)C);
    const float fp = w_prev[j], fc = w_cur[j];
    const float* pp = prev + z * Hp * Wp;
    float* cp = cur + z * Hp * Wp;
    const int n = x >= Wp ? 0 : (Wp - x < TIME_VEC ? (int)(Wp - x) : TIME_VEC);      // samples of the row this thread owns; none beyond the row
    const int ns = x >= w ? 0 : (w - x < TIME_VEC ? (int)(w - x) : TIME_VEC);        // ... and how many of them lie in the picture
    unsigned long long acc = 0;
    if (n > 0) {
        for (int y = blockIdx.y * TIME_ROWS + threadIdx.y; y < Hp; y += gridDim.y * TIME_ROWS) {      // the grid covers every row unless Hp > 4 * 65535
            const float* a = pp + (size_t)y * Wp + x;
            float* c = cp + (size_t)y * Wp + x;
            const int m = (STAT && y < h) ? ns : 0;
            if (n == TIME_VEC && (((uintptr_t)a | (uintptr_t)c) & 15) == 0) {
                const float4 v = *(const float4*)a;
                float4 o = *(const float4*)c;
                if (STAT) {
                    if (0 < m) acc += seam_sq(v.x, o.x);
                    if (1 < m) acc += seam_sq(v.y, o.y);
                    if (2 < m) acc += seam_sq(v.z, o.z);
                    if (3 < m) acc += seam_sq(v.w, o.w);
                }
                o.x = (fp * v.x) + (fc * o.x);
                o.y = (fp * v.y) + (fc * o.y);
                o.z = (fp * v.z) + (fc * o.z);
                o.w = (fp * v.w) + (fc * o.w);
                *(float4*)c = o;
            } else {
#pragma unroll
                for (int k = 0; k < TIME_VEC; ++k)
                    if (k < n) {
                        const float v = a[k], o = c[k];
                        if (STAT && k < m) acc += seam_sq(v, o);
                        c[k] = (fp * v) + (fc * o);
                    }
            }
        }
    }
    if (STAT) {                                                                    // every thread of the workgroup arrives here: nothing above returns
        acc = wave_sum_u64(acc);
        if (threadIdx.x == 0) part[threadIdx.y] = acc;
        __syncthreads();
        if (threadIdx.x == 0 && threadIdx.y == 0) {
            const unsigned long long tot = (part[0] + part[1]) + (part[2] + part[3]);
            if (tot) atomicAdd(&sq[z], tot);
        }
    }
}

}  // namespace

extern "C" int sn_time_crossfade(const float* prev, float* cur, const float* w_prev, const float* w_cur, unsigned long long* sq,
                                 int V, int C, int Hp, int Wp, int h, int w, void* stream) {
    sn_clear_error();
    if (!prev || !cur || !w_prev || !w_cur) return SN_EINVAL;
    if (((uintptr_t)prev | (uintptr_t)cur | (uintptr_t)w_prev | (uintptr_t)w_cur) & 3) return SN_EINVAL;
    if ((uintptr_t)sq & 7) return SN_EINVAL;
    if (V < 1 || C < 1 || Hp < 1 || Wp < 1) return SN_EINVAL;
    if (h < 1 || h > Hp || w < 1 || w > Wp) return SN_EINVAL;
    if ((long long)V * C > 65535) return SN_EINVAL;
    if (sq && (long long)h * w > (1ll << 25)) return SN_EINVAL;                     // 2^25 samples of at most 2^38 each: the plane's sum stays below 2^63
    const int per_wg = 64 * TIME_VEC;
    const int rows = (Hp - 1) / TIME_ROWS + 1;
    const dim3 block(64, TIME_ROWS), grid((Wp - 1) / per_wg + 1, rows < 65535 ? rows : 65535, V * C);
    if (sq) hipLaunchKernelGGL(time_crossfade_kernel<true>, grid, block, 0, (hipStream_t)stream, prev, cur, w_prev, w_cur, sq, C, Hp, Wp, h, w);
    else hipLaunchKernelGGL(time_crossfade_kernel<false>, grid, block, 0, (hipStream_t)stream, prev, cur, w_prev, w_cur, sq, C, Hp, Wp, h, w);
    return sn_check_launch();
}
