// Dirt and blotches taken out on the device (gfx950), for `restore_video --despot`: planar Y'CbCr payloads in, payloads of the same format out.
// No float frame is made and no colour conversion runs.  The rule is the spike detection index of the film-restoration literature along the integer
// block vectors of sn_yuv_block_motion; include/shiftnet_hip.h states it and tests/despot_ref.py restates it, byte for byte.
//
//   sn_yuv_despot : S payloads + the vectors of every frame into its previous and into its next frame -> n payloads (frames f0 .. f0 + n - 1 repaired
//                   from the ORIGINAL frames f - 1, f, f + 1) and [n][2] uint32 counts (the core seeds, the luma samples replaced).
//
// One launch.  A workgroup of 16 x 16 threads owns a 128 x 32 luma tile of one frame -- 8 x 2 whole vector blocks -- and its chroma; a thread owns 8 x 2
// luma samples (they lie in ONE vector block) and their chroma: 8 x 2 samples at 4:4:4, 4 x 1 at 4:2:0, which are exactly the chroma samples its own
// luma samples decide.
//   1. The seeds of the tile plus a halo of 1 + grow samples go into an LDS byte mask.  A thread makes the seeds of its own samples from rows it reads
//      with the wide ldn (a vector is constant per block, so the displaced samples of a row of a block are contiguous; where the displaced row crosses
//      the picture's edge, and so is clamped, sample by sample) and keeps the source codes and the repaired ones in registers; the ring of the halo is
//      made sample by sample, every sample looking up the vector of its own block.  Samples outside the picture are not seeds.
//   2. The core seeds (a seed with at least `support` seeds among its eight neighbours) of the tile plus a halo of `grow` go into a second LDS mask.
//   3. A thread ORs the core mask over the (2 grow + 1)^2 square around each of its samples: M.  It stores its luma with the wide stn (source or repair),
//      reads the chroma at the displaced places only where it has a sample in M, and stores its chroma.  The two counts are summed in LDS and leave
//      with two global atomics per workgroup at most.  Integer sums commute: the bytes and counts depend on neither the geometry nor the schedule.
// Every displaced coordinate is clamped to its plane and every block index to the grid: ANY int8 vector keeps every read inside the payloads.
#include "sn_yuv_color.h"

namespace {

constexpr int DS_TW = 128, DS_TH = 32;                                    // a workgroup's tile in luma samples: 8 x 2 vector blocks
constexpr int DS_MAXG = 2, DS_MAXHALO = 1 + DS_MAXG;
constexpr int DS_SP = DS_TW + 2 * DS_MAXHALO, DS_SR = DS_TH + 2 * DS_MAXHALO;      // the seed mask: pitch and rows
constexpr int DS_CP = DS_TW + 2 * DS_MAXG, DS_CR = DS_TH + 2 * DS_MAXG;            // the core mask

struct DespotArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int8_t* mv_prev;
    const int8_t* mv_next;
    uint32_t* counts;
    int f0, nby, nbx;                                                      // nby * nbx == 0: a picture without a vector block, no seeds
    int threshold, support, grow, chroma;
};

// the vector (dy, dx) of luma sample (y, x) in a frame's grid: that of block (min(y / 16, nby - 1), min(x / 16, nbx - 1))
__device__ __forceinline__ void vec_at(const int8_t* mv, int nby, int nbx, int y, int x, int* dy, int* dx) {
    const int8_t* v = mv + 2 * ((size_t)imin(y >> 4, nby - 1) * nbx + imin(x >> 4, nbx - 1));
    *dy = v[0];
    *dx = v[1];
}

__device__ __forceinline__ int clampi(int v, int hi) { return imin(imax(v, 0), hi); }

__device__ __forceinline__ bool is_seed(int c, int p, int n, int threshold) {
    const int a = c - p, b = c - n;
    const int d = ((a > 0 && b > 0) || (a < 0 && b < 0)) ? imin(abs(a), abs(b)) : 0;
    return d > threshold + abs(p - n);
}

// 8 samples of row y (clamped to the plane of h x w samples, pitch w) from column x on, each column clamped: wide where none is
template <int ESZ> __device__ __forceinline__ void row8_clamped(const uint8_t* plane, int h, int w, int y, int x, int* v) {
    const size_t row = (size_t)clampi(y, h - 1) * w;
    if (x >= 0 && x + 8 <= w) ldn<ESZ, 8>(plane, row + x, v);
    else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = ld1<ESZ>(plane, row + clampi(x + k, w - 1));
    }
}

template <int ESZ, int CH>
__global__ __launch_bounds__(256) void yuv_despot_kernel(const DespotArgs A, const YuvGeo G) {
    constexpr bool SUB = CH != SN_YUV_444;
    constexpr int CNX = SUB ? 4 : 8, CNY = SUB ? 1 : 2;                    // a thread's chroma samples
    __shared__ uint8_t seed[DS_SR * DS_SP];
    __shared__ uint8_t core[DS_CR * DS_CP];
    __shared__ uint32_t cnt[2];
    const int tid = threadIdx.y * 16 + threadIdx.x;
    const int H = G.h, W = G.w;
    const int cw = SUB ? (W + 1) >> 1 : W, ch = SUB ? (H + 1) >> 1 : H;
    const int i = blockIdx.z, f = A.f0 + i;
    const int halo = 1 + A.grow, grow = A.grow;
    const bool vectors = A.nby > 0 && A.nbx > 0;
    const uint8_t* fc = A.src + (size_t)f * G.frame_bytes;                // the frame, the one before, the one after: originals all three
    const uint8_t* fp = fc - G.frame_bytes;
    const uint8_t* fn = fc + G.frame_bytes;
    uint8_t* out = A.dst + (size_t)i * G.frame_bytes;
    const size_t grid_bytes = (size_t)A.nby * A.nbx * 2;
    const int8_t* mvp = A.mv_prev + (size_t)(f - 1) * grid_bytes;          // frame f's blocks into frame f - 1
    const int8_t* mvn = A.mv_next + (size_t)f * grid_bytes;                // ... and into frame f + 1
    const int ty0 = blockIdx.y * DS_TH, tx0 = blockIdx.x * DS_TW;
    const int y0 = ty0 + threadIdx.y * 2, x0 = tx0 + threadIdx.x * 8;
    const bool active = y0 < H && x0 < W;
    const int nx = imin(8, W - x0);                                       // the thread's samples that exist in a row
    if (tid < 2) cnt[tid] = 0;

    // ---- 1. the seeds: the thread's own samples, source and repair kept
    int Yc[2][8], Yr[2][8];
    int dyp = 0, dxp = 0, dyn = 0, dxn = 0;
    if (active) {
        if (vectors) {
            vec_at(mvp, A.nby, A.nbx, y0, x0, &dyp, &dxp);                // y0 .. y0 + 1 and x0 .. x0 + 7 lie in one block
            vec_at(mvn, A.nby, A.nbx, y0, x0, &dyn, &dxn);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = y0 + r;
            uint8_t* srow = seed + (y - ty0 + halo) * DS_SP + (x0 - tx0 + halo);
            if (y >= H) {                                                 // the loop below writes the mask outside the picture
#pragma unroll
                for (int k = 0; k < 8; ++k) { Yc[r][k] = 0; Yr[r][k] = 0; }
                continue;
            }
            int P[8], N[8];
            row8_clamped<ESZ>(fc + G.oy, H, W, y, x0, Yc[r]);
            if (vectors) {
                row8_clamped<ESZ>(fp + G.oy, H, W, y + dyp, x0 + dxp, P);
                row8_clamped<ESZ>(fn + G.oy, H, W, y + dyn, x0 + dxn, N);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!vectors) { P[k] = Yc[r][k]; N[k] = Yc[r][k]; }
                Yr[r][k] = (P[k] + N[k] + 1) >> 1;
                if (k < nx) srow[k] = is_seed(Yc[r][k], P[k], N[k], A.threshold) ? 1 : 0;
            }
        }
    }
    // ---- ... and the ring of the halo, sample by sample; also the tile's samples no thread is active for (outside the picture: no seeds)
    {
        const int rw = DS_TW + 2 * halo, rh = DS_TH + 2 * halo;
        for (int e = tid; e < rw * rh; e += 256) {
            const int ry = e / rw, rx = e - ry * rw;
            const int y = ty0 - halo + ry, x = tx0 - halo + rx;
            const bool inside_tile = ry >= halo && ry < halo + DS_TH && rx >= halo && rx < halo + DS_TW;
            const bool in_picture = y >= 0 && y < H && x >= 0 && x < W;
            if (inside_tile && in_picture) continue;                      // its thread has written it, and nobody else does
            uint8_t s = 0;
            if (in_picture && vectors) {
                int ay, ax, by, bx;
                vec_at(mvp, A.nby, A.nbx, y, x, &ay, &ax);
                vec_at(mvn, A.nby, A.nbx, y, x, &by, &bx);
                const int c = ld1<ESZ>(fc + G.oy, (size_t)y * W + x);
                const int p = ld1<ESZ>(fp + G.oy, (size_t)clampi(y + ay, H - 1) * W + clampi(x + ax, W - 1));
                const int n = ld1<ESZ>(fn + G.oy, (size_t)clampi(y + by, H - 1) * W + clampi(x + bx, W - 1));
                s = is_seed(c, p, n, A.threshold) ? 1 : 0;
            }
            seed[ry * DS_SP + rx] = s;
        }
    }
    __syncthreads();

    // ---- 2. the core seeds of the tile plus a halo of `grow`
    {
        const int rw = DS_TW + 2 * grow, rh = DS_TH + 2 * grow;
        for (int e = tid; e < rw * rh; e += 256) {
            const int ry = e / rw, rx = e - ry * rw;
            const uint8_t* s = seed + (ry + 1) * DS_SP + (rx + 1);         // the seed mask's halo is one wider
            int around = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx)
                    if (dy || dx) around += s[dy * DS_SP + dx];
            core[ry * DS_CP + rx] = (s[0] && around >= A.support) ? 1 : 0;
        }
    }
    __syncthreads();

    // ---- 3. M, the stores and the counts
    if (active) {
        bool M[2][8];
        int ncore = 0, nm = 0;
        bool any = false;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                M[r][k] = false;
                if (y0 + r >= H || k >= nx) continue;
                const uint8_t* c = core + (y0 + r - ty0 + grow) * DS_CP + (x0 + k - tx0 + grow);
                int m = 0;
                for (int dy = -grow; dy <= grow; ++dy)
                    for (int dx = -grow; dx <= grow; ++dx) m |= c[dy * DS_CP + dx];
                ncore += c[0];
                nm += m;
                M[r][k] = m != 0;
            }
        }
        if (ncore) atomicAdd(&cnt[0], (uint32_t)ncore);
        if (nm) atomicAdd(&cnt[1], (uint32_t)nm);
        any = nm != 0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (y0 + r >= H) break;
            int v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = M[r][k] ? Yr[r][k] : Yc[r][k];
            const size_t o = (size_t)(y0 + r) * G.py + x0;
            if (nx == 8) stn<ESZ, 8>(out + G.oy, o, v); else for (int k = 0; k < nx; ++k) st1<ESZ>(out + G.oy, o + k, v[k]);
        }
        // ---- chroma: the source's, or the mean of the two neighbours at the displaced place where the luma says so
        const int cy0 = SUB ? y0 >> 1 : y0, cx0 = SUB ? x0 >> 1 : x0;
        const int ncx = imin(CNX, cw - cx0);
        const bool follow = A.chroma != 0 && any;
        const int cdyp = SUB ? dyp >> 1 : dyp, cdxp = SUB ? dxp >> 1 : dxp, cdyn = SUB ? dyn >> 1 : dyn, cdxn = SUB ? dxn >> 1 : dxn;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const size_t op = pl ? G.ov : G.ou;
#pragma unroll
            for (int r = 0; r < CNY; ++r) {
                const int cy = cy0 + r;
                if (cy >= ch) break;
                int v[CNX];
                const size_t o = (size_t)cy * G.pc + cx0;
                if (ncx == CNX) ldn<ESZ, CNX>(fc + op, o, v);
                else {
#pragma unroll
                    for (int k = 0; k < CNX; ++k) v[k] = k < ncx ? ld1<ESZ>(fc + op, o + k) : 0;
                }
                if (follow) {
#pragma unroll
                    for (int k = 0; k < CNX; ++k) {
                        const bool m = SUB ? (M[0][2 * k] || M[0][2 * k + 1] || M[1][2 * k] || M[1][2 * k + 1]) : M[r][k];
                        if (k < ncx && m) {
                            const int pu = ld1<ESZ>(fp + op, (size_t)clampi(cy + cdyp, ch - 1) * G.pc + clampi(cx0 + k + cdxp, cw - 1));
                            const int nu = ld1<ESZ>(fn + op, (size_t)clampi(cy + cdyn, ch - 1) * G.pc + clampi(cx0 + k + cdxn, cw - 1));
                            v[k] = (pu + nu + 1) >> 1;
                        }
                    }
                }
                if (ncx == CNX) stn<ESZ, CNX>(out + op, o, v); else for (int k = 0; k < ncx; ++k) st1<ESZ>(out + op, o + k, v[k]);
            }
        }
    }
    __syncthreads();
    if (tid < 2 && cnt[tid]) atomicAdd(&A.counts[2 * i + tid], cnt[tid]);
}

}  // namespace

extern "C" {

int sn_yuv_despot(const uint8_t* src, const sn_yuv_fmt* fmt, const int8_t* mv_prev, const int8_t* mv_next, uint8_t* dst, uint32_t* counts,
                  int S, int f0, int n, int threshold, int support, int grow, int chroma, int H, int W, void* stream) {
    sn_clear_error();
    YuvK K;
    YuvGeo G;
    if (!valid_payloads(src, fmt, S, H, W) || !dst || !aligned_payload(fmt, dst) || !make_consts(fmt, &K)) return SN_EINVAL;
    if (!mv_prev || !mv_next || !counts || ((uintptr_t)counts & 3) || !make_geo(fmt, H, W, nullptr, &G)) return SN_EINVAL;
    if (f0 < 1 || n < 1 || (long long)f0 + n > (long long)S - 1) return SN_EINVAL;     // a frame's two neighbours are payloads of src
    if (threshold < 0 || support < 0 || support > 8 || grow < 0 || grow > DS_MAXG || chroma < 0 || chroma > 1) return SN_EINVAL;
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
    if (a < b + (size_t)n * G.frame_bytes && b < a + (size_t)S * G.frame_bytes) return SN_EINVAL;      // a frame's neighbours read its original
    const dim3 block(16, 16), grid((W + DS_TW - 1) / DS_TW, (H + DS_TH - 1) / DS_TH, n);
    if (grid.y > 65535) return SN_EINVAL;
    const int hb = H / 2, wb = W / 2;
    DespotArgs A;
    A.src = src; A.dst = dst; A.mv_prev = mv_prev; A.mv_next = mv_next; A.counts = counts;
    A.f0 = f0;
    A.nby = hb > 0 && wb > 0 ? (hb + 7) / 8 : 0;
    A.nbx = hb > 0 && wb > 0 ? (wb + 7) / 8 : 0;
    A.threshold = threshold; A.support = support; A.grow = grow; A.chroma = chroma;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)n * 2 * sizeof(uint32_t), s) != hipSuccess) return sn_check_launch();      // counts is overwritten, not added to
    with_esz_chroma(fmt, [&](auto esz, auto ch) { hipLaunchKernelGGL((yuv_despot_kernel<esz(), ch()>), grid, block, 0, s, A, G); });
    return sn_check_launch();
}

}  // extern "C"
