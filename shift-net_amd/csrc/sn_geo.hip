// The data movement of the self-ensemble (shiftnet_amd/ensemble.py, VideoRestorer(ensemble=...)): the network runs on mirrored, transposed and
// time-reversed copies of a window, and each float32 result is mapped back and added into the window's float32 canvas.
//
//   sn_geo_transform  : src [T][C][H][W] of esz-byte elements -> dst [T][C][H'][W'],  dst[t'][c][y'][x'] = src[t][c][y][x]        (data movement)
//   sn_geo_accumulate : member [T][C][H'][W'] f32 -> canvas [T][C][H][W] f32,  a = init ? member : canvas + member;  canvas = a * scale
//
// (H', W') = (W, H) with SN_GEO_TRANSPOSE, else (H, W).  One index map, stated in include/shiftnet_hip.h and restated by tests/geo_ref.py, defines
// both: u = FLIP_Y ? H' - 1 - y' : y';  v = FLIP_X ? W' - 1 - x' : x';  (y, x) = TRANSPOSE ? (v, u) : (u, v);  t = REVERSE_T ? T - 1 - t' : t'.
// The kernels equal the restatement bit for bit.  The sum and the product of the accumulation are rounded separately (contraction is off for this
// file: no FMA), as in sn_tile.hip and for the same reason.
//
// Both are bandwidth kernels, and both have two paths.  The map pairs a sample of the TRANSFORMED tensor (dst / member) with one of the PLAIN tensor
// (src / canvas); a path walks the pairs, and only what it does with a pair differs between the two kernels.
//
// Without TRANSPOSE (rows_kernel): a row of one tensor is a row of the other, possibly mirrored.  A thread owns 16 bytes of a transformed row -- 4
//   or 8 elements -- and the chunk of the plain row they map to; with FLIP_X that chunk is the mirrored one and the thread reverses the elements in
//   registers.  Where both chunks are whole and both addresses 16-byte aligned they move as one 16-byte access each, otherwise element by element
//   with the same result.  The test is on the address itself: with FLIP_X the mirrored chunk starts at element W - 16 / esz - x, which is aligned
//   only when W * esz is a multiple of 16.  The row and the frame are index arithmetic.  Wave64: a wave covers 1 KiB of a row, a workgroup 4 rows.
//
// With TRANSPOSE (tiles_kernel): a workgroup of 256 threads moves a 64 x 64 tile of the plain tensor through LDS, so that the global accesses of
//   both tensors run along rows: a wave reads 64 consecutive elements of a row of the tensor it reads, and writes 64 consecutive elements -- ascending
//   or, under the flip of that axis, descending -- of a row of the tensor it writes.  One element per lane: a wave's access is 128 B for 2-byte and
//   256 B for 4-byte elements, whole and contiguous but not wide per lane; nothing here needs an alignment beyond the element's own.
//   LDS: the tile is kept as [64][65] 32-bit words whatever esz is (a 2-byte element is widened to a word: 16.25 KiB either way), so one bank
//   computation covers both sizes.  Phase 1 writes lds[r][lane] with ds_write_b32: word address 65 r + lane, bank (65 r + lane) % 32 = (r + lane)
//   % 32; the instruction is served in two 32-lane halves, and within a half the 32 lanes fall on 32 different banks: degree 1, no conflict.  Phase 2
//   reads lds[lane][r] with ds_read_b32: word address 65 lane + r, bank (65 lane + r) % 32 = (lane + r) % 32: again 32 different banks within each
//   half, degree 1.  (With a pitch of 64 words phase 2 would put all 32 lanes of a half on one bank: degree 32.)  So by the bank rule of
//   ds_write_b32 / ds_read_b32 -- bank = (byte address / 4) % 32, conflicts only within a 32-lane half -- the conflict degree is 1 for 2-byte and
//   for 4-byte elements alike; the price of widening is that 2-byte elements use half of each LDS word.  This is computed, not measured.
//
// T * C may exceed what a grid dimension takes: the grid's z is min(T * C, 65535) and every workgroup LOOPS over the planes z, z + gridDim.z, ...;
// rows (tile rows) beyond 65535 grid entries are looped over in the same way.  No atomics: the launches of a window run one after the other on one
// stream, and within a launch every sample of the tensor written belongs to exactly one thread.
#include "sn_common.h"
#pragma clang fp contract(off)

namespace {

constexpr int GEO_ROWS = 4;        // rows per workgroup of rows_kernel (blockDim.y)
constexpr int GEO_TILE = 64;       // side of tiles_kernel's tile
constexpr int GEO_PITCH = 65;      // words per tile row in LDS
constexpr int GEO_GRID_MAX = 65535;

struct geo_shape {
    int op, T, C, H, W;            // H, W: the sides of the plain tensor
};

// what the two entry points do with a pair of samples: P the transformed tensor's, Q the plain tensor's
struct geo_move {                  // sn_geo_transform: P = Q
    template <typename E> __device__ __forceinline__ void wide(E* p, E* q, bool mirror) const {
        uint4 v = *(const uint4*)q;
        if (mirror) {
            v = make_uint4(v.w, v.z, v.y, v.x);
            if (sizeof(E) == 2) {
                v.x = (v.x >> 16) | (v.x << 16); v.y = (v.y >> 16) | (v.y << 16);
                v.z = (v.z >> 16) | (v.z << 16); v.w = (v.w >> 16) | (v.w << 16);
            }
        }
        *(uint4*)p = v;
    }
    template <typename E> __device__ __forceinline__ E load(const E* p, const E* q) const { return *q; }       // phase 1 of a tile: what goes to LDS
    template <typename E> __device__ __forceinline__ void one(E* p, E* q, E staged) const { *p = staged; }     // phase 2: the staged element lands
};

struct geo_add {                   // sn_geo_accumulate: Q = (init ? P : Q + P) * scale
    int init;
    float scale;
    __device__ __forceinline__ float f(float c, float m) const {
        const float a = init ? m : c + m;
        return a * scale;
    }
    __device__ __forceinline__ void wide(float* p, float* q, bool mirror) const {
        float4 m = *(const float4*)p;
        if (mirror) m = make_float4(m.w, m.z, m.y, m.x);
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!init) c = *(const float4*)q;
        c.x = f(c.x, m.x); c.y = f(c.y, m.y); c.z = f(c.z, m.z); c.w = f(c.w, m.w);
        *(float4*)q = c;
    }
    __device__ __forceinline__ float load(const float* p, const float* q) const { return *p; }
    __device__ __forceinline__ void one(float* p, float* q, float staged) const { *q = f(init ? 0.f : *q, staged); }
};

template <typename E, typename F>
__global__ __launch_bounds__(64 * GEO_ROWS) void rows_kernel(E* __restrict__ P, E* __restrict__ Q, geo_shape s, F fn) {
    constexpr int VEC = 16 / (int)sizeof(E);
    const long long x = ((long long)blockIdx.x * 64 + threadIdx.x) * VEC;      // 64 bit: the last workgroup of a very wide row passes 2^31
    if (x >= s.W) return;
    const int n = s.W - x < VEC ? (int)(s.W - x) : VEC;
    const bool fx = s.op & SN_GEO_FLIP_X, fy = s.op & SN_GEO_FLIP_Y, rt = s.op & SN_GEO_REVERSE_T;
    const long long xq = fx ? s.W - n - x : x;                                 // the plain row's chunk: elements xq .. xq + n - 1, mirrored under FLIP_X
    const size_t planes = (size_t)s.T * s.C;
    for (size_t z = blockIdx.z; z < planes; z += gridDim.z) {
        const size_t tp = z / s.C, c = z % s.C, zq = (rt ? s.T - 1 - tp : tp) * s.C + c;
        for (int y = blockIdx.y * GEO_ROWS + threadIdx.y; y < s.H; y += gridDim.y * GEO_ROWS) {
            E* p = P + (z * s.H + y) * s.W + x;
            E* q = Q + (zq * s.H + (fy ? s.H - 1 - y : y)) * s.W + xq;
            if (n == VEC && (((uintptr_t)p | (uintptr_t)q) & 15) == 0) {
                fn.wide(p, q, fx);
            } else {
                for (int k = 0; k < n; ++k) {
                    E* qk = q + (fx ? n - 1 - k : k);
                    fn.one(p + k, qk, fn.load(p + k, qk));
                }
            }
        }
    }
}

// P is [T][C][W][H] here: the sample (y, x) of a plain plane pairs with (y', x') = (FLIP_Y ? W - 1 - x : x, FLIP_X ? H - 1 - y : y) of a transformed one
// (the index map solved for y', x' with H' = W, W' = H).  TO_P: phase 1 reads the plain tensor and phase 2 writes the transformed one (transform);
// otherwise phase 1 reads the transformed tensor and phase 2 writes the plain one (accumulate).
template <typename E, typename F, bool TO_P>
__global__ __launch_bounds__(256) void tiles_kernel(E* __restrict__ P, E* __restrict__ Q, geo_shape s, F fn) {
    __shared__ uint32_t lds[GEO_TILE * GEO_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool fx = s.op & SN_GEO_FLIP_X, fy = s.op & SN_GEO_FLIP_Y, rt = s.op & SN_GEO_REVERSE_T;
    const long long x0 = (long long)blockIdx.x * GEO_TILE;
    const size_t planes = (size_t)s.T * s.C, plane = (size_t)s.H * s.W;
    const int tiles_y = (s.H - 1) / GEO_TILE + 1;
    for (size_t z = blockIdx.z; z < planes; z += gridDim.z) {
        const size_t tp = z / s.C, c = z % s.C, zq = (rt ? s.T - 1 - tp : tp) * s.C + c;
        E* pz = P + z * plane;
        E* qz = Q + zq * plane;
        for (int ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {
            const long long y0 = (long long)ty * GEO_TILE;
            // phase 1: rows of the tensor read -> lds[r][lane].  TO_P: r is the plain row, lane the plain column; otherwise r is the plain column
            // (a transformed row) and lane the plain row (along that transformed row)
            for (int r = wave; r < GEO_TILE; r += 4) {
                const long long y = y0 + (TO_P ? r : lane), x = x0 + (TO_P ? lane : r);
                if (y < s.H && x < s.W) {
                    E* q = qz + (size_t)y * s.W + x;
                    E* p = pz + (size_t)(fy ? s.W - 1 - x : x) * s.H + (fx ? s.H - 1 - y : y);
                    const E e = fn.load(p, q);
                    uint32_t word = 0;
                    __builtin_memcpy(&word, &e, sizeof(E));
                    lds[r * GEO_PITCH + lane] = word;
                }
            }
            __syncthreads();
            // phase 2: lds[lane][r] -> rows of the tensor written.  TO_P: lane is the plain row (along a transformed row), r the plain column;
            // otherwise lane is the plain column and r the plain row
            for (int r = wave; r < GEO_TILE; r += 4) {
                const long long y = y0 + (TO_P ? lane : r), x = x0 + (TO_P ? r : lane);
                if (y < s.H && x < s.W) {
                    E* q = qz + (size_t)y * s.W + x;
                    E* p = pz + (size_t)(fy ? s.W - 1 - x : x) * s.H + (fx ? s.H - 1 - y : y);
                    const uint32_t word = lds[lane * GEO_PITCH + r];
                    E e;
                    __builtin_memcpy(&e, &word, sizeof(E));
                    fn.one(p, q, e);
                }
            }
            __syncthreads();      // the next tile's phase 1 overwrites what this phase read
        }
    }
}

// the arguments both entry points refuse: sizes, op, the element count, alignment, overlap.  *bytes: the size of either tensor
int geo_check(const void* a, const void* b, int esz, int op, int T, int C, int H, int W) {
    if (!a || !b) return SN_EINVAL;
    if (esz != 2 && esz != 4) return SN_EINVAL;
    if (((uintptr_t)a | (uintptr_t)b) & (uintptr_t)(esz - 1)) return SN_EINVAL;
    if (op < 0 || op > 15) return SN_EINVAL;
    if (T < 1 || C < 1 || H < 1 || W < 1) return SN_EINVAL;
    // the kernels index with size_t; the byte count of a tensor must fit ptrdiff_t.  Four factors below 2^31: multiply with a check at every step
    const unsigned long long limit = 0x7fffffffffffffffull / (unsigned)esz;
    unsigned long long n = (unsigned long long)T * (unsigned long long)C;      // < 2^62
    if (n > limit / (unsigned long long)H) return SN_EINVAL;
    n *= (unsigned long long)H;
    if (n > limit / (unsigned long long)W) return SN_EINVAL;
    n *= (unsigned long long)W;
    const unsigned long long bytes = n * (unsigned)esz;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    if (pa > UINTPTR_MAX - bytes || pb > UINTPTR_MAX - bytes) return SN_EINVAL;
    if (pa < pb + bytes && pb < pa + bytes) return SN_EINVAL;                   // the two ranges overlap
    return SN_OK;
}

template <typename E, typename F, bool TO_P>
int geo_launch(E* P, E* Q, const geo_shape& s, const F& fn, void* stream) {
    const size_t planes = (size_t)s.T * s.C;
    const unsigned gz = planes < (size_t)GEO_GRID_MAX ? (unsigned)planes : (unsigned)GEO_GRID_MAX;
    if (s.op & SN_GEO_TRANSPOSE) {
        const int ty = (s.H - 1) / GEO_TILE + 1;
        const dim3 block(256), grid((s.W - 1) / GEO_TILE + 1, ty < GEO_GRID_MAX ? ty : GEO_GRID_MAX, gz);
        hipLaunchKernelGGL((tiles_kernel<E, F, TO_P>), grid, block, 0, (hipStream_t)stream, P, Q, s, fn);
    } else {
        const int per_wg = 64 * (16 / (int)sizeof(E));
        const int rows = (s.H - 1) / GEO_ROWS + 1;
        const dim3 block(64, GEO_ROWS), grid((s.W - 1) / per_wg + 1, rows < GEO_GRID_MAX ? rows : GEO_GRID_MAX, gz);
        hipLaunchKernelGGL((rows_kernel<E, F>), grid, block, 0, (hipStream_t)stream, P, Q, s, fn);
    }
    return sn_check_launch();
}

}  // namespace

extern "C" int sn_geo_transform(const void* src, void* dst, int esz, int op, int T, int C, int H, int W, void* stream) {
    sn_clear_error();
    if (geo_check(src, dst, esz, op, T, C, H, W) != SN_OK) return SN_EINVAL;
    const geo_shape s{op, T, C, H, W};
    if (esz == 2) return geo_launch<uint16_t, geo_move, true>((uint16_t*)dst, (uint16_t*)const_cast<void*>(src), s, geo_move{}, stream);
    return geo_launch<uint32_t, geo_move, true>((uint32_t*)dst, (uint32_t*)const_cast<void*>(src), s, geo_move{}, stream);
}

extern "C" int sn_geo_accumulate(const float* member, float* canvas, int op, int init, float scale, int T, int C, int H, int W, void* stream) {
    sn_clear_error();
    if (geo_check(member, canvas, 4, op, T, C, H, W) != SN_OK) return SN_EINVAL;
    if (!(scale - scale == 0.f)) return SN_EINVAL;                              // inf and nan: neither is finite
    const geo_shape s{op, T, C, H, W};
    return geo_launch<float, geo_add, false>(const_cast<float*>(member), canvas, s, geo_add{init != 0, scale}, stream);
}
