// The blend of the tiled video restorer (shiftnet_amd/restore.py, VideoRestorer(tile=...)): the float32 result of one tile's forward is added
// into the window's float32 canvas with the tile's feather weights.
//
//   sn_tile_accumulate : tile [T][C][th][tw] f32, weights wy[th] and wx[tw] f32 -> canvas [T][C][Hc][Wc] f32, the th x tw rectangle at (y0, x0)
//                        of every plane:  canvas = canvas + (wy[y] * wx[x]) * tile.
//
// The arithmetic is stated in include/shiftnet_hip.h and restated by tests/tile_ref.py, which this kernel equals bit for bit.  Every float product
// and sum is rounded separately (contraction is off for this file: no FMA), as in sn_yuv.hip and for the same reason.
//
// A bandwidth kernel: 12 bytes moved per sample (tile read, canvas read, canvas write) and three float operations.  One thread owns 4 consecutive
// samples of a row; where the addresses of its 4 tile samples and of its 4 canvas samples are both 16-byte aligned it moves them as one float4
// each way, otherwise sample by sample with the same arithmetic.  The test is on the address itself: x0 is arbitrary, and so is the parity of a
// row when tw or Wc is no multiple of 4.  Wave64: a wave covers 256 consecutive samples of one row, a workgroup 4 rows; T * C is the grid's z.
// No LDS, no atomics: the tiles of a window are accumulated one launch after the other on one stream, so two launches never touch a sample at once.
#include "sn_common.h"
#pragma clang fp contract(off)

namespace {

constexpr int TILE_VEC = 4;        // samples per thread
constexpr int TILE_ROWS = 4;       // rows per workgroup (blockDim.y)

__global__ __launch_bounds__(64 * TILE_ROWS) void tile_accumulate_kernel(const float* __restrict__ tile, float* __restrict__ canvas,
                                                                         const float* __restrict__ wy, const float* __restrict__ wx,
                                                                         int th, int tw, int Hc, int Wc, int y0, int x0) {
    const long long x = ((long long)blockIdx.x * 64 + threadIdx.x) * TILE_VEC;      // 64 bit: the last workgroup of a very wide tile passes 2^31
    if (x >= tw) return;
    const size_t z = blockIdx.z;                                               // the plane: t * C + c in both tensors
    const float* tp = tile + z * th * tw;
    float* cp = canvas + (z * Hc + y0) * Wc + x0;
    const int n = tw - x < TILE_VEC ? (int)(tw - x) : TILE_VEC;
    float fx[TILE_VEC];
#pragma unroll
    for (int k = 0; k < TILE_VEC; ++k) fx[k] = k < n ? wx[x + k] : 0.f;
    for (int y = blockIdx.y * TILE_ROWS + threadIdx.y; y < th; y += gridDim.y * TILE_ROWS) {      // the grid covers every row unless th > 4 * 65535
        const float fy = wy[y];
        const float* a = tp + (size_t)y * tw + x;
        float* c = cp + (size_t)y * Wc + x;
        if (n == TILE_VEC && (((uintptr_t)a | (uintptr_t)c) & 15) == 0) {
            const float4 v = *(const float4*)a;
            float4 o = *(const float4*)c;
            o.x = o.x + (fy * fx[0]) * v.x;
            o.y = o.y + (fy * fx[1]) * v.y;
            o.z = o.z + (fy * fx[2]) * v.z;
            o.w = o.w + (fy * fx[3]) * v.w;
            *(float4*)c = o;
        } else {
#pragma unroll
            for (int k = 0; k < TILE_VEC; ++k)
                if (k < n) c[k] = c[k] + (fy * fx[k]) * a[k];
        }
    }
}

}  // namespace

extern "C" int sn_tile_accumulate(const float* tile, float* canvas, const float* wy, const float* wx, int T, int C, int th, int tw, int Hc, int Wc,
                                  int y0, int x0, void* stream) {
    sn_clear_error();
    if (!tile || !canvas || !wy || !wx) return SN_EINVAL;
    if (((uintptr_t)tile | (uintptr_t)canvas | (uintptr_t)wy | (uintptr_t)wx) & 3) return SN_EINVAL;
    if (T < 1 || C < 1 || th < 1 || tw < 1 || Hc < 1 || Wc < 1) return SN_EINVAL;
    if (y0 < 0 || x0 < 0 || y0 > Hc - th || x0 > Wc - tw) return SN_EINVAL;      // th <= Hc and tw <= Wc follow; no sum that could overflow
    if ((long long)T * C > 65535) return SN_EINVAL;
    const int per_wg = 64 * TILE_VEC;
    const int rows = (th - 1) / TILE_ROWS + 1;
    const dim3 block(64, TILE_ROWS), grid((tw - 1) / per_wg + 1, rows < 65535 ? rows : 65535, T * C);
    hipLaunchKernelGGL(tile_accumulate_kernel, grid, block, 0, (hipStream_t)stream, tile, canvas, wy, wx, th, tw, Hc, Wc, y0, x0);
    return sn_check_launch();
}
