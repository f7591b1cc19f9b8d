// Statistics of the luma plane of planar Y'CbCr payloads, for the decisions the video restorer makes on the host (gfx950).  The payloads are those
// of csrc/sn_yuv.hip; all but sn_yuv_diff_stats leave the chroma planes unread, and of the format only the bit depth decides anything there.
//
//   sn_yuv_thumb  : T payloads -> [T][ceil(H/8)][ceil(W/8)] uint16 sums of the luma codes of every 8 x 8 block (the scene-cut measure of
//                   shiftnet_amd/scenes.py is computed from these on the host);
//   sn_yuv_noise_hist : T payloads -> [T][2 (2^bits - 1) + 1] uint32 histograms of |a - b - c + d| over the 2 x 2 luma blocks whose four codes lie
//                   strictly between lo and hi (the blind noise estimate of shiftnet_amd/noise.py is computed from these on the host);
//                   sn_yuv_noise_hist_rect: the same kernel on a picture rectangle of the stream (YuvGeo, sn_yuv.h);
//   sn_yuv_noise_hist_bands : the same statistic split into 16 bands of the block's brightness, v saturated to NBV = 128 / 512 bins: [T][16][NBV]
//                   uint32 (the noise-level function of shiftnet_amd/noise.py is estimated from these on the host); rect or the whole frame;
//   sn_yuv_noise_hist_pairs, sn_yuv_noise_hist_pairs_bands : the same two statistics of the DIFFERENCE of consecutive payloads, T - 1 pairs:
//                   [T - 1][4 (2^bits - 1) + 1] and [T - 1][16][NBV] uint32 (the temporal noise estimate of shiftnet_amd/noise.py); rect or the whole frame;
//   sn_yuv_block_motion : T payloads -> [T - 1][nby][nbx][2] int8 vectors and [T - 1][nby][nbx] uint32 SADs: per 16 x 16 luma block of every pair the
//                   integer translation within +-7 samples with the smallest sum of absolute differences over HALF of the block's 2 x 2 blocks;
//                   sn_yuv_noise_hist_pairs_mv, sn_yuv_noise_hist_pairs_bands_mv: the two pair statistics over the OTHER half, the second payload's block
//                   taken where the vector points (the motion-compensated temporal estimate of shiftnet_amd/noise.py); rect or the whole frame;
//   sn_noise_map_level : T payloads and the 16 knots of a noise-level function -> [T][1][Hp][Wp] of the module dtype or float32: the function at the
//                   low-passed luma of every pixel (bilinear between the means of the 8 x 8 blocks): the denoisers' noise plane; rect or the whole frame;
//   sn_yuv_rowcol_sums : T payloads -> [T][H] and [T][W] uint32 sums of the luma codes of every row and every column (the letterbox rule of
//                   shiftnet_amd/picture.py is evaluated on these on the host);
//   sn_yuv_diff_stats : two sets of T payloads, what came in and what was written -> [T][16] int64 sums of their difference in all three planes: its
//                   moments, its products with the right, lower and next-frame neighbour, its energy on the edges of the written picture (the method-noise
//                   report of shiftnet_amd/report.py is computed from these on the host); rect or the whole frame;
//   sn_yuv_diff_stats_mv : the same two sets of T payloads and the vectors of sn_yuv_block_motion -> [T - 1][8] int64 sums over the measuring blocks of
//                   every pair: the moments of the luma difference in both payloads and their product along the vectors (the report's motion-compensated
//                   temporal correlation); rect or the whole frame.
// The seven sn_yuv_noise_hist* entry points launch the instances of ONE kernel template, yuv_noise_hist_kernel<sample size, kind, bands>, from one
// host function; every other entry point has a kernel of its own.
//
// All but the noise map are integer reductions: sums commute, so the results are the same for every launch geometry and every schedule, and the numpy
// restatements of tests/ equal them exactly.  The noise map is float32 arithmetic with every product and sum rounded separately (contraction is
// off for this file: no FMA), stated in include/shiftnet_hip.h and restated by tests/nlf_ref.py.
#include "sn_yuv.h"
#pragma clang fp contract(off)

namespace {

// The thumbnail, noise-map and row/column kernels below repeat one piece of code on purpose: the 8-sample row load with its tree sum and element-wise
// edge path.  It was moved into one __forceinline__ function (pointer and by-value results) and every formulation changed the instruction stream of
// the kernels that used it, some their register counts too: the helper is simplified on its own before it is inlined, and the scheduler then sees
// another order.  A kernel that changes that piece should change the copies together.  The noise histograms are the other way round: one kernel body
// whose variants are template parameters, held to its results, resources and time per launch rather than to an instruction order.

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

// ---- noise histograms ---------------------------------------------------------------------------------------------------------------
// One kernel for the six noise statistics, at both depths twelve instances.  KIND says what is measured on a non-overlapping 2 x 2 luma block with the
// codes p q / r s and HH = p - q - r + s (twice its Haar HH coefficient):
//   HIST_SPATIAL  : v = |HH| of payload blockIdx.y, counted where the four codes lie strictly between lo and hi;
//   HIST_PAIRS    : v = |HH(payload p + 1) - HH(payload p)| of the same block in both payloads of pair p = blockIdx.y, counted where all EIGHT codes
//                   lie strictly between lo and hi.  Content that does not move cancels and the noise of both frames stays: v has the variance
//                   8 s^2 + 2/3 where the spatial statistic has 4 s^2 + 1/3.  The second payload lies frame_bytes further on, which need not be a
//                   multiple of 16: every load tests its own address and takes the element-wise path on its own;
//   HIST_PAIRS_MV : the pair statistic on the MEASURING blocks, (i + j) odd, with the four codes of payload p + 1 taken at (2 i + dy, 2 j + dx), (dy, dx)
//                   the vector that yuv_block_motion_kernel (below) found on the other half of block (i / 8, j / 8).  The displaced block is at no
//                   particular alignment and is loaded element-wise, after the test that it lies inside the picture: mv is device memory nobody has
//                   validated, and with the test any int8 contents are safe -- a block whose displaced position is not wholly inside the h x w picture
//                   does not count, and nothing outside the picture is read.
// BANDS splits the count by the brightness of the block: band = (4 (S - 4 lo)) / (hi - lo) with S the sum of the four codes, (2 (S - 8 lo)) / (hi - lo)
// with the sum of the eight; every code is > lo and < hi, so 4 <= S - 4 lo <= 4 (hi - lo) - 4 (8 and 8 (hi - lo) - 8) and the band is 0 .. 15.  v is
// then saturated to NBV - 1.
// The walk: a lane owns a unit of four horizontally adjacent blocks (8 x 2 pixels: one 8 B / 16 B load per row where the ADDRESS allows it, element-wise
// otherwise and where fewer than four blocks are left on the right edge); a workgroup walks units gridDim.x * 256 apart of one frame or pair.  A unit's
// four blocks lie in one vector block (4 divides 8) and two of them measure: blocks 1 and 3 in an even block row, 0 and 2 in an odd one.
// The histogram, [NBANDS][NBV] words, lives in LDS: the bins v >= LOW in one plain array, the bins v < LOW -- where nearly all of the mass lies, and
// neighbouring blocks are mostly of one brightness, so of one band -- in COPIES copies, copy (lane & (COPIES - 1)) at word (band * LOW + v) * COPIES +
// copy.  An LDS instruction is served in lane groups 0..31 and 32..63 and a b32 access banks by word mod 32, so with 32 copies the 32 lanes of a group
// hit 32 different banks whatever their bins: a wave's add to the low bins never meets a bank conflict or a second lane on its own address.  With
// fewer copies neighbouring lanes are on different copies and lanes COPIES apart share one.  At the end the copies are summed, each lane starting at
// another copy so that the lanes of a group read different banks, and the non-zero bins are added to dst with one global atomic each.  Integer sums
// commute: the result is the same for every geometry and every schedule.
// The constants.  NBV: every value of v, 2 (2^bits - 1) + 1 and twice as far for pairs; with bands 128 / 512.  LOW covers the same range of noise
// levels at both depths and in every form: 32 / 128 bins flat and 16 / 64 by band for the spatial statistic, and 1.5 times that for pairs, whose v is
// sqrt(2) times as wide at the same noise level.  COPIES is 32, except 8 and 4 for the 10-bit band forms, spatial and pairs, where 32 copies of 16 x
// 64 (96) bins do not fit beside the 32 KB of the plain array -- at 10 bit v spreads over four times as many bins, so lanes meet on a word less often
// to begin with.  (DESIGN.md 3.25 has the LDS, registers and time of every instance.)
enum { HIST_SPATIAL, HIST_PAIRS, HIST_PAIRS_MV };

template <int ESZ, int KIND, bool BANDS> struct HistK {
    static constexpr bool PAIR = KIND != HIST_SPATIAL;
    static constexpr int CODES = ESZ == 1 ? 256 : 1024;
    static constexpr int NBANDS = BANDS ? SN_NLF_BANDS : 1;
    static constexpr int NBV = BANDS ? CODES / 2 : (PAIR ? 4 : 2) * (CODES - 1) + 1;      // 128 / 512; 511 / 2047, pairs 1021 / 4093
    static constexpr int LOW = CODES / (BANDS ? 16 : 8) * (PAIR ? 3 : 2) / 2;            // 16 / 64, pairs 24 / 96; 32 / 128, pairs 48 / 192
    static constexpr int COPIES = BANDS && ESZ == 2 ? (PAIR ? 4 : 8) : 32;
    static constexpr int LOWW = NBANDS * LOW * COPIES, HISTW = NBANDS * NBV;
    static constexpr bool ZERO16 = LOWW % 4 == 0 && HISTW % 4 == 0;                      // the band forms: both arrays are zeroed 16 B at a time
};

// HIST_PAIRS_MV has one argument more, the vectors, their grid and the picture's size; the other kinds have none in its place (the pack is empty),
// so that their argument list is what the kernels before the template had
struct HistMvK { const int8_t* mv; int h, w, nby, nbx; };

template <int ESZ, int KIND, bool BANDS, typename... MVK>
__global__ __launch_bounds__(256) void yuv_noise_hist_kernel(const uint8_t* __restrict__ src, uint32_t* __restrict__ dst, int lo, int hi, int W, int hb,
                                                           int wb, int ux, size_t origin, size_t frame_bytes, const MVK... mvk) {
    using K = HistK<ESZ, KIND, BANDS>;
    constexpr int NBV = K::NBV, LOW = K::LOW, COPIES = K::COPIES, LOWW = K::LOWW, HISTW = K::HISTW;
    constexpr bool PAIRS = KIND == HIST_PAIRS, MV = KIND == HIST_PAIRS_MV;
    static_assert(sizeof...(mvk) == (MV ? 1 : 0));
    [[maybe_unused]] const HistMvK M = [&] { if constexpr (MV) return (mvk, ...); else return HistMvK{}; }();
    __shared__ __attribute__((aligned(K::ZERO16 ? 16 : 4))) uint32_t low[LOWW];
    __shared__ __attribute__((aligned(K::ZERO16 ? 16 : 4))) uint32_t hist[HISTW];
    const int tid = threadIdx.x, t = blockIdx.y, cp = tid & (COPIES - 1);      // t: the frame, or the pair of payloads t and t + 1 <= T - 1
    if constexpr (K::ZERO16) {
        for (int i = tid; i < LOWW / 4; i += 256) ((uint4*)low)[i] = make_uint4(0u, 0u, 0u, 0u);
        for (int i = tid; i < HISTW / 4; i += 256) ((uint4*)hist)[i] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        for (int i = tid; i < LOWW; i += 256) low[i] = 0;
        for (int i = tid; i < HISTW; i += 256) hist[i] = 0;
    }
    __syncthreads();
    const uint8_t* y0 = src + (size_t)t * frame_bytes + origin;           // W: the luma row pitch; origin: the byte offset of block (0, 0)
    const uint8_t* y1 = y0 + frame_bytes;
    const int units = ux * hb;                                            // hb, wb: whole 2 x 2 blocks; ux = ceil(wb / 4) units per block row
    const uint32_t span = (uint32_t)(hi - lo);
    for (int u = blockIdx.x * 256 + tid; u < units; u += gridDim.x * 256) {
        const int by = u / ux, bx0 = (u - by * ux) * 4;
        const int nb = imin(4, wb - bx0);
        const size_t r0 = (size_t)(2 * by) * W + 2 * bx0, r1 = r0 + W;
        [[maybe_unused]] int yd = 0, dx = 0;                              // HIST_PAIRS_MV: the displaced block's first row, and the vector's dx
        if constexpr (MV) {
            const int8_t* v2 = M.mv + (((size_t)t * M.nby + (by >> 3)) * M.nbx + (bx0 >> 3)) * 2;      // by / 8 < nby and bx0 / 8 < nbx: inside mv whatever it holds
            yd = 2 * by + v2[0], dx = v2[1];
        }
        int a0[8], b0[8], a1[8], b1[8];
        if (nb == 4) {
            ldn<ESZ, 8>(y0, r0, a0);
            ldn<ESZ, 8>(y0, r1, b0);
            if constexpr (PAIRS) {
                ldn<ESZ, 8>(y1, r0, a1);
                ldn<ESZ, 8>(y1, r1, b1);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {                                 // pixels 2 bx0 .. 2 (bx0 + nb) - 1 < 2 wb <= W exist; the others are not read
                const bool in = k < 2 * nb;
                a0[k] = in ? ld1<ESZ>(y0, r0 + k) : 0;
                b0[k] = in ? ld1<ESZ>(y0, r1 + k) : 0;
                if constexpr (PAIRS) {
                    a1[k] = in ? ld1<ESZ>(y1, r0 + k) : 0;
                    b1[k] = in ? ld1<ESZ>(y1, r1 + k) : 0;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p0 = a0[2 * k], q0 = a0[2 * k + 1], r0c = b0[2 * k], s0 = b0[2 * k + 1];
            int p1 = 0, q1 = 0, r1c = 0, s1 = 0;                          // the block of payload t + 1
            if constexpr (MV) {
                const int xd = 2 * (bx0 + k) + dx;                        // rows yd, yd + 1 must lie in 0 .. h - 1 and columns xd, xd + 1 in 0 .. w - 1
                if (!(k < nb && ((by + k) & 1) && yd >= 0 && yd + 2 <= M.h && xd >= 0 && xd + 2 <= M.w)) continue;      // bx0 is even: (by + k) is the parity of
                                                                          // (i + j); nothing is loaded for a block that does not count
                const size_t o = (size_t)yd * W + xd;
                p1 = ld1<ESZ>(y1, o), q1 = ld1<ESZ>(y1, o + 1), r1c = ld1<ESZ>(y1, o + W), s1 = ld1<ESZ>(y1, o + W + 1);
            } else if constexpr (PAIRS) {
                p1 = a1[2 * k], q1 = a1[2 * k + 1], r1c = b1[2 * k], s1 = b1[2 * k + 1];
            }
            int mn, mx;
            if constexpr (K::PAIR) {
                mn = imin(imin(imin(p0, q0), imin(r0c, s0)), imin(imin(p1, q1), imin(r1c, s1)));
                mx = imax(imax(imax(p0, q0), imax(r0c, s0)), imax(imax(p1, q1), imax(r1c, s1)));
            } else {
                mn = imin(imin(p0, q0), imin(r0c, s0)), mx = imax(imax(p0, q0), imax(r0c, s0));
            }
            if ((MV || k < nb) && mn > lo && mx < hi) {
                const int d = K::PAIR ? (p1 - q1 - r1c + s1) - (p0 - q0 - r0c + s0) : p0 - q0 - r0c + s0;
                // a code of the format gives v <= NBV - 1.  Where hi admits stored 16-bit words above 2^bits - 1 the flat spatial and pair forms index past
                // hist, as they always did: inside the workgroup's own LDS the count lands on another bin, beyond it the hardware drops the access
                int v = d < 0 ? -d : d;
                if constexpr (BANDS || MV) v = imin(v, NBV - 1);
                int band = 0;
                if constexpr (BANDS) {                                    // 0 .. 15 (above)
                    if constexpr (K::PAIR) band = (int)((uint32_t)(2 * (((p0 + q0) + (r0c + s0)) + ((p1 + q1) + (r1c + s1)) - 8 * lo)) / span);
                    else band = (int)((uint32_t)(4 * ((p0 + q0) + (r0c + s0) - 4 * lo)) / span);
                }
                if (v < LOW) atomicAdd(&low[(band * LOW + v) * COPIES + cp], 1u);
                else atomicAdd(&hist[band * NBV + v], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* out = dst + (size_t)t * HISTW;
    for (int i = tid; i < HISTW; i += 256) {
        uint32_t n = hist[i];
        const int band = BANDS ? i / NBV : 0, v = i - band * NBV;
        if (v < LOW) {
            const uint32_t* c = low + (band * LOW + v) * COPIES;
            const int rot = (i * COPIES) >> 5;                            // consecutive bins start on different copies: the lanes of a group read 32 different banks
#pragma unroll 8
            for (int k = 0; k < COPIES; ++k) n += c[(k + rot) & (COPIES - 1)];
        }
        if (n) atomicAdd(&out[i], n);
    }
}

// ---- block motion of frame pairs ------------------------------------------------------------------------------------------------------------
// The vector of a 16 x 16 luma block (a "vector block": 8 x 8 of the 2 x 2 blocks above) of payload p is the (dy, dx), |dy|, |dx| <= MV_R = 7, for which
// the sum of |Y_p(y, x) - Y_{p+1}(y + dy, x + dx)| over the block's MATCHING 2 x 2 blocks -- (i + j) even, half of them, a checkerboard -- is smallest.
// The histogram kernels below measure on the other half: pixel noise is independent between the two, so the choice cannot fit the noise it is
// measured on (include/shiftnet_hip.h states the arithmetic and the tie order; DESIGN.md 3.23 the reason).
// A workgroup takes MV_RUN = 4 neighbouring vector blocks of one block row of one pair, blockIdx = (run, block row, pair).  It stages their 16 x 64
// samples of payload p and the 30 x 78 samples of payload p + 1 that their candidates reach (neighbouring blocks share 14 of a block's 30 columns)
// in LDS as 16-bit words, element-wise loads, consecutive lanes consecutive samples of a row; what lies outside the picture is not read and stays 0
// in LDS, where no admissible candidate looks.  Then lane c < 225 owns candidate c = (dy + 7) 15 + (dx + 7) for one vector block after the other: 128
// differences from LDS (the reference sample is one address for the whole wave, a broadcast; the window's addresses are consecutive in dx), the
// key SAD * 256 + rank with rank the candidate's place in the tie order, 0xFFFFFFFF where the displaced block would leave the picture, and one unsigned
// minimum over the workgroup: across the wave by cross-lane moves, across the four waves by an LDS atomic.  SAD <= 128 x 65535 < 2^24: the key fits.
// The rank is computed once per lane by counting the candidates that come before its own.  Ragged blocks at the right and lower edge have fewer 2 x 2
// blocks and loops that are shorter by that much.  Integer arithmetic throughout: the result does not depend on the geometry or the schedule.
constexpr int MV_R = 7, MV_D = 2 * MV_R + 1, MV_CAND = MV_D * MV_D, MV_RUN = 4;
constexpr int MV_WW = 16 * MV_RUN + 2 * MV_R, MV_WH = 16 + 2 * MV_R, MV_RW = 16 * MV_RUN;      // 78 x 30 window, 64 x 16 reference

template <int ESZ>
__global__ __launch_bounds__(256) void yuv_block_motion_kernel(const uint8_t* __restrict__ src, int8_t* __restrict__ mv, uint32_t* __restrict__ sad, int h,
                                                             int w, int W, int hb, int wb, int nbx, size_t origin, size_t frame_bytes) {
    __shared__ uint16_t win[MV_WH * MV_WW];
    __shared__ uint16_t ref[16 * MV_RW];
    __shared__ uint32_t best[MV_RUN];
    __shared__ uint8_t cand_of[MV_CAND];                                  // rank -> candidate
    const int tid = threadIdx.x, J0 = blockIdx.x * MV_RUN, I = blockIdx.y, pr = blockIdx.z;
    const int nby = gridDim.y;
    const uint8_t* y0 = src + (size_t)pr * frame_bytes + origin;          // payload pr; W: the luma row pitch; origin: the byte offset of the picture's first sample
    const uint8_t* y1 = y0 + frame_bytes;                                 // payload pr + 1 <= T - 1
    const int Y0 = 16 * I, X0 = 16 * J0;                                  // the run's first sample, < 2 hb and < 2 wb
    for (int i = tid; i < MV_WH * MV_WW; i += 256) {
        const int r = i / MV_WW, c = i - r * MV_WW, y = Y0 - MV_R + r, x = X0 - MV_R + c;
        win[i] = (y >= 0 && y < h && x >= 0 && x < w) ? (uint16_t)ld1<ESZ>(y1, (size_t)y * W + x) : (uint16_t)0;
    }
    for (int i = tid; i < 16 * MV_RW; i += 256) {
        const int r = i / MV_RW, c = i - r * MV_RW, y = Y0 + r, x = X0 + c;
        ref[i] = (y < 2 * hb && x < 2 * wb) ? (uint16_t)ld1<ESZ>(y0, (size_t)y * W + x) : (uint16_t)0;
    }
    if (tid < MV_RUN) best[tid] = 0xFFFFFFFFu;
    const int dy = tid / MV_D - MV_R, dx = tid % MV_D - MV_R;             // lanes 225 .. 255 own no candidate
    const bool own = tid < MV_CAND;
    int rank = 0;
    if (own) {
        const int n = (dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx);
        for (int c = 0; c < MV_CAND; ++c) {                               // the candidates before this one in the order (|dy| + |dx|, dy, dx)
            const int ey = c / MV_D - MV_R, ex = c % MV_D - MV_R, m = (ey < 0 ? -ey : ey) + (ex < 0 ? -ex : ex);
            rank += (m < n || (m == n && (ey < dy || (ey == dy && ex < dx)))) ? 1 : 0;
        }
        cand_of[rank] = (uint8_t)tid;
    }
    __syncthreads();
    const int rows = imin(8, hb - 8 * I);                                 // the 2 x 2 block rows of this block row: 1 .. 8
    const int ye = Y0 + 2 * rows;                                         // the end of its sample extent
    const int runs = imin(MV_RUN, nbx - J0);
    for (int b = 0; b < runs; ++b) {
        const int cols = imin(8, wb - 8 * (J0 + b));                      // 1 .. 8
        const int xs = X0 + 16 * b, xe = xs + 2 * cols;
        uint32_t key = 0xFFFFFFFFu;
        if (own && Y0 + dy >= 0 && ye + dy <= h && xs + dx >= 0 && xe + dx <= w) {
            uint32_t s = 0;
            for (int bi = 0; bi < rows; ++bi) {
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const uint16_t* a = ref + (2 * bi + r) * MV_RW + 16 * b;
                    const uint16_t* q = win + (2 * bi + r + MV_R + dy) * MV_WW + 16 * b + MV_R + dx;
                    for (int bj = bi & 1; bj < cols; bj += 2) {           // (bi + bj) even: 8 I and 8 J are even, the parity is that of (i, j)
                        const int d0 = (int)a[2 * bj] - (int)q[2 * bj], d1 = (int)a[2 * bj + 1] - (int)q[2 * bj + 1];
                        s += (uint32_t)(d0 < 0 ? -d0 : d0) + (uint32_t)(d1 < 0 ? -d1 : d1);
                    }
                }
            }
            key = (s << 8) | (uint32_t)rank;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)key, m, 64);
            key = o < key ? o : key;
        }
        if ((tid & 63) == 0) atomicMin(&best[b], key);
    }
    __syncthreads();
    if (tid < runs) {                                                     // (0, 0) is always admissible: best holds a candidate's key
        const uint32_t k = best[tid];
        const int c = cand_of[k & 255u];
        const size_t o = ((size_t)pr * nby + I) * nbx + J0 + tid;
        mv[2 * o] = (int8_t)(c / MV_D - MV_R);
        mv[2 * o + 1] = (int8_t)(c % MV_D - MV_R);
        sad[o] = k >> 8;
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
// ---- method noise: sums of the difference of two sets of payloads ---------------------------------------------------------------------------
// d = b - a of the luma and of both chroma planes, and the sums include/shiftnet_hip.h lists (sn_yuv_diff_stats): of d, of d^2, of the products of d with its
// right, lower and next-frame neighbour, and of d^2 over the pixels that b calls an edge.  blockIdx.y is the payload; payload t + 1 is read by the
// workgroups of t (for the temporal product) and by its own.  A lane owns a unit of 8 x DS_STRIP luma samples: per row one 8 B / 16 B load of a and of
// b where the ADDRESS allows it, element-wise otherwise and on the right edge, plus the one sample right of the unit; it walks down the strip and keeps
// the row below in registers, so that a row is loaded once per unit (and the first row of the next strip twice).  Neighbouring lanes own neighbouring
// units of a strip; a workgroup walks units gridDim.x * 256 apart.  The chroma planes follow in units of the same shape, U and V together.  Every lane
// accumulates in 64 bit -- one product reaches 65535^2 when a 10-bit payload holds arbitrary words, so a 32-bit partial sum is wrong after two
// pixels -- then the 11 sums are added across the wave (cross-lane moves, no LDS), across the four waves through 4 x 16 words of LDS, and the
// workgroup adds each non-zero sum to dst with ONE 64-bit vector atomic.  The first workgroup of a payload adds the four counts the same way.  Integer
// sums commute (a negative sum is added modulo 2^64): the result is the same for every geometry and every schedule.
constexpr int DS_STRIP = 8;

__device__ __forceinline__ long long wave_sum_ll(long long x) {             // the sum over the 64 lanes, in every lane
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// n (1..8) samples of one row of a and of b from element o on: d[k] = b - a and bb[k] = b, both 0 for k >= n; right: the sample at o + 8 exists, then
// dR and bR are its difference and its b, otherwise 0
template <int ESZ>
__device__ __forceinline__ void diff_row(const uint8_t* ap, const uint8_t* bp, size_t o, int n, bool right, int* d, int* bb, int& dR, int& bR) {
    int av[8];
    if (n == 8) {
        ldn<ESZ, 8>(ap, o, av);
        ldn<ESZ, 8>(bp, o, bb);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {                                     // samples o .. o + n - 1 exist; the others are not read
            const bool in = k < n;
            av[k] = in ? ld1<ESZ>(ap, o + k) : 0;
            bb[k] = in ? ld1<ESZ>(bp, o + k) : 0;
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = bb[k] - av[k];
    bR = right ? ld1<ESZ>(bp, o + 8) : 0;
    dR = right ? bR - ld1<ESZ>(ap, o + 8) : 0;
}

template <int ESZ>
__global__ __launch_bounds__(256) void yuv_diff_stats_kernel(const uint8_t* a, const uint8_t* b, unsigned long long* dst, const YuvGeo G, int ch, int cw,
                                                           int edge, int T) {
    __shared__ long long part[4][SN_DIFF_STATS];
    const int tid = threadIdx.x, t = blockIdx.y;
    const int h = G.h, w = G.w;
    const uint8_t* af = a + (size_t)t * G.frame_bytes;
    const uint8_t* bf = b + (size_t)t * G.frame_bytes;
    const bool next = t + 1 < T;                                          // payload t + 1 exists: only then is anything beyond payload t read
    long long s1 = 0, s2 = 0, sx = 0, sy = 0, st = 0, ne = 0, s2e = 0, su = 0, su2 = 0, sv = 0, sv2 = 0;
    {
        const uint8_t* ay = af + G.oy;
        const uint8_t* by = bf + G.oy;
        const int ux = (w + 7) >> 3, units = ux * ((h + DS_STRIP - 1) / DS_STRIP);
        for (int u = blockIdx.x * 256 + tid; u < units; u += gridDim.x * 256) {
            const int sr = u / ux, x0 = (u - sr * ux) * 8, y0 = sr * DS_STRIP, y1 = imin(y0 + DS_STRIP, h);
            const int n = imin(8, w - x0);                                // >= 1
            const bool right = x0 + 8 < w;                                // n < 8 is the picture's right edge: no sample right of the unit
            int d[8], bb[8], dR, bR;
            diff_row<ESZ>(ay, by, (size_t)y0 * G.py + x0, n, right, d, bb, dR, bR);
#pragma unroll 1
            for (int y = y0; y < y1; ++y) {
                const size_t o = (size_t)y * G.py + x0;
                int dn[8], bn[8], dRn = 0, bRn = 0, dt[8];
                if (y + 1 < h) {
                    diff_row<ESZ>(ay, by, o + G.py, n, right, dn, bn, dRn, bRn);
                } else {                                                  // the last row: no product, and the row below is the row itself
#pragma unroll
                    for (int k = 0; k < 8; ++k) { dn[k] = 0; bn[k] = bb[k]; }
                }
                if (next) {
                    int bt[8], dRt, bRt;
                    diff_row<ESZ>(ay + G.frame_bytes, by + G.frame_bytes, o, n, false, dt, bt, dRt, bRt);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) dt[k] = 0;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int dk = d[k];                                  // 0 beyond the picture, and so is every product with it
                    const int dr = k < 7 ? d[k + 1] : dR;
                    const int br = k < 7 ? (k + 1 < n ? bb[k + 1] : bb[k]) : (right ? bR : bb[k]);       // min(x + 1, w - 1)
                    const int eh = br - bb[k], ev = bn[k] - bb[k];
                    const int e = (eh < 0 ? -eh : eh) + (ev < 0 ? -ev : ev);
                    const long long q = (long long)dk * dk;
                    s1 += dk;
                    s2 += q;
                    sx += (long long)dk * dr;
                    sy += (long long)dk * dn[k];
                    st += (long long)dk * dt[k];
                    if (k < n && e >= edge) { ne += 1; s2e += q; }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) { d[k] = dn[k]; bb[k] = bn[k]; }
                dR = dRn; bR = bRn;
            }
        }
    }
    {
        const uint8_t* au = af + G.ou;
        const uint8_t* bu = bf + G.ou;
        const uint8_t* av = af + G.ov;
        const uint8_t* bv = bf + G.ov;
        const int ux = (cw + 7) >> 3, units = ux * ((ch + DS_STRIP - 1) / DS_STRIP);
        for (int u = blockIdx.x * 256 + tid; u < units; u += gridDim.x * 256) {
            const int sr = u / ux, x0 = (u - sr * ux) * 8, y0 = sr * DS_STRIP, y1 = imin(y0 + DS_STRIP, ch);
            const int n = imin(8, cw - x0);
#pragma unroll 1
            for (int y = y0; y < y1; ++y) {
                const size_t o = (size_t)y * G.pc + x0;
                int du[8], dv[8], x[8], dR, bR;
                diff_row<ESZ>(au, bu, o, n, false, du, x, dR, bR);
                diff_row<ESZ>(av, bv, o, n, false, dv, x, dR, bR);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    su += du[k];
                    su2 += (long long)du[k] * du[k];
                    sv += dv[k];
                    sv2 += (long long)dv[k] * dv[k];
                }
            }
        }
    }
    // the words of dst[t] in their order; the counts are not sums of the lanes
    long long v[SN_DIFF_STATS] = {0, s1, s2, 0, sx, 0, sy, st, ne, s2e, 0, su, su2, sv, sv2, 0};
#pragma unroll
    for (int i = 0; i < SN_DIFF_STATS; ++i) {
        if (i == 0 || i == 3 || i == 5 || i == 10 || i == 15) continue;
        v[i] = wave_sum_ll(v[i]);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < SN_DIFF_STATS; ++i) part[tid >> 6][i] = v[i];
    }
    __syncthreads();
    if (tid < SN_DIFF_STATS) {
        long long tot = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
        if (blockIdx.x == 0) {
            if (tid == 0) tot = (long long)h * w;
            if (tid == 3) tot = (long long)h * (w - 1);
            if (tid == 5) tot = (long long)(h - 1) * w;
            if (tid == 10) tot = (long long)ch * cw;
        }
        if (tot) atomicAdd(&dst[(size_t)t * SN_DIFF_STATS + tid], (unsigned long long)tot);
    }
}

// ---- method noise along block motion vectors ------------------------------------------------------------------------------------------------
// The temporal product of yuv_diff_stats_kernel compares d = b - a of a payload with the next payload's d at the same place: removed detail that moves
// with the picture reads as uncorrelated.  Here the next payload's samples are taken where the vector of yuv_block_motion_kernel points, on the
// MEASURING 2 x 2 blocks, (i + j) odd -- the vector was chosen on the other half, so the choice cannot fit what is measured -- and the eight sums
// include/shiftnet_hip.h lists (sn_yuv_diff_stats_mv) are made of d0 = d_p(y, x), d1 = d_{p+1}(y + dy, x + dx) and g = b_{p+1}(y + dy, x + dx) - b_p(y, x).
// blockIdx.y is the pair.  A lane owns a unit of 8 x 8 luma samples anchored at multiples of 8: 4 x 4 blocks of one vector block (4 divides 8), so one
// vector per unit, and two blocks of every block row measure: 1 and 3 in an even block row, 0 and 2 in an odd one.  Per sample row one 8 B / 16 B load
// of a and of b of payload p where the ADDRESS allows it, element-wise otherwise and where fewer than four blocks are left on the right edge.  The
// displaced row of payload p + 1 is at no particular alignment: where all of its 8 samples lie inside the picture and both addresses allow it (a zero
// vector in an aligned stream: static footage) it is one wide load per plane, otherwise the 4 samples of the two measuring blocks are loaded
// element-wise, each block after the test that its displaced position lies wholly inside the picture.  mv is device memory nobody has validated: with
// that test any int8 contents are safe, a block that fails it does not count and nothing outside the picture is read.  Neighbouring lanes own
// neighbouring units of a unit row; a workgroup walks units gridDim.x * 256 apart.  Accumulators, reduction and the one 64-bit vector atomic per
// workgroup and non-zero word are those of yuv_diff_stats_kernel; here the two counts are sums of the lanes too.  Integer sums commute: the result is
// the same for every geometry and every schedule.
template <int ESZ>
__global__ __launch_bounds__(256) void yuv_diff_stats_mv_kernel(const uint8_t* a, const uint8_t* b, const int8_t* __restrict__ mv, unsigned long long* dst,
                                                              const YuvGeo G, int hb, int wb, int nby, int nbx) {
    __shared__ long long part[4][SN_DIFF_STATS_MV];
    const int tid = threadIdx.x, p = blockIdx.y;                          // pair p: payloads p and p + 1 <= T - 1
    const int h = G.h, w = G.w;
    const uint8_t* a0 = a + (size_t)p * G.frame_bytes + G.oy;
    const uint8_t* b0 = b + (size_t)p * G.frame_bytes + G.oy;
    const uint8_t* a1 = a0 + G.frame_bytes;
    const uint8_t* b1 = b0 + G.frame_bytes;
    const int ux = (wb + 3) >> 2, units = ux * ((hb + 3) >> 2);           // hb, wb: whole 2 x 2 blocks; a unit is 4 x 4 of them
    int nm = 0, nv = 0;
    long long s0 = 0, s00 = 0, s1 = 0, s11 = 0, s01 = 0, sgg = 0;
    for (int u = blockIdx.x * 256 + tid; u < units; u += gridDim.x * 256) {
        const int uy = u / ux, uxi = u - uy * ux, x0 = uxi * 8, y0 = uy * 8;
        const int nb = imin(4, wb - 4 * uxi), rows = 2 * imin(4, hb - 4 * uy);      // blocks per block row 1 .. 4, sample rows 2 .. 8
        const int8_t* v2 = mv + (((size_t)p * nby + (uy >> 1)) * nbx + (uxi >> 1)) * 2;      // uy / 2 < nby and uxi / 2 < nbx: inside mv whatever it holds
        const int dy = v2[0], dx = v2[1];
        const int moved = (dy | dx) != 0 ? 1 : 0;
        const int xd0 = x0 + dx;                                          // the displaced unit's first column
        const bool xin = nb == 4 && xd0 >= 0 && xd0 + 8 <= w;             // all 8 samples of a displaced row lie in the picture's columns
#pragma unroll 1
        for (int r = 0; r < rows; ++r) {
            const int odd = (r >> 1) & 1;                                 // 4 uy and 4 uxi are even: the measuring blocks of this row are bj = 1 - odd, 3 - odd
            const int yd = y0 + (r & ~1) + dy;                            // the displaced block row's first sample row: rows yd, yd + 1 must lie in 0 .. h - 1
            if (yd < 0 || yd + 2 > h) continue;                           // no block of this row counts: nothing is loaded
            const size_t o = (size_t)(y0 + r) * G.py + x0;
            int av[8], bv[8];
            if (nb == 4) {
                ldn<ESZ, 8>(a0, o, av);
                ldn<ESZ, 8>(b0, o, bv);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {                             // samples x0 .. x0 + 2 nb - 1 < 2 wb <= w exist; the others are not read
                    const bool in = k < 2 * nb;
                    av[k] = in ? ld1<ESZ>(a0, o + k) : 0;
                    bv[k] = in ? ld1<ESZ>(b0, o + k) : 0;
                }
            }
            const long long od = (long long)(yd + (r & 1)) * G.py + xd0;   // element offset of the displaced row's first sample; xd0 may be negative
            const bool wide = xin && ((((uintptr_t)a1 + (uintptr_t)(od * ESZ)) | ((uintptr_t)b1 + (uintptr_t)(od * ESZ))) & (8 * ESZ - 1)) == 0;
            int aw[8], bw[8];
            if (wide) {
                ldn<ESZ, 8>(a1, (size_t)od, aw);
                ldn<ESZ, 8>(b1, (size_t)od, bw);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int bj = 1 - odd + 2 * m, xd = xd0 + 2 * bj;        // columns xd, xd + 1 must lie in 0 .. w - 1
                if (!(bj < nb && xd >= 0 && xd + 2 <= w)) continue;
                nm += 2;
                nv += 2 * moved;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int ap = odd ? av[4 * m + s] : av[4 * m + 2 + s], bp = odd ? bv[4 * m + s] : bv[4 * m + 2 + s];
                    int an, bn;
                    if (wide) {
                        an = odd ? aw[4 * m + s] : aw[4 * m + 2 + s];
                        bn = odd ? bw[4 * m + s] : bw[4 * m + 2 + s];
                    } else {
                        an = ld1<ESZ>(a1, (size_t)(od + 2 * bj + s));
                        bn = ld1<ESZ>(b1, (size_t)(od + 2 * bj + s));
                    }
                    const int d0 = bp - ap, d1 = bn - an, g = bn - bp;
                    s0 += d0;
                    s00 += (long long)d0 * d0;
                    s1 += d1;
                    s11 += (long long)d1 * d1;
                    s01 += (long long)d0 * d1;
                    sgg += (long long)g * g;
                }
            }
        }
    }
    long long v[SN_DIFF_STATS_MV] = {nm, s0, s00, s1, s11, s01, sgg, nv};   // the words of dst[p] in their order
#pragma unroll
    for (int i = 0; i < SN_DIFF_STATS_MV; ++i) v[i] = wave_sum_ll(v[i]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < SN_DIFF_STATS_MV; ++i) part[tid >> 6][i] = v[i];
    }
    __syncthreads();
    if (tid < SN_DIFF_STATS_MV) {
        const long long tot = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
        if (tot) atomicAdd(&dst[(size_t)p * SN_DIFF_STATS_MV + tid], (unsigned long long)tot);
    }
}
}  // namespace

// The seven histogram entry points: one kernel instance each way.  T payloads are T frames or T - 1 pairs; mv is looked at by the vector forms alone
template <int KIND, bool BANDS>
static int noise_hist(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const int8_t* mv, uint32_t* dst, int lo, int hi, int T, int H, int W,
                      void* stream) {
    constexpr bool PAIR = KIND != HIST_SPATIAL, MV = KIND == HIST_PAIRS_MV;
    sn_clear_error();
    if (!valid_payloads(src, fmt, T, H, W) || !dst || ((uintptr_t)dst & 3) || lo > hi) return SN_EINVAL;
    if ((PAIR && T < 2) || (MV && !mv)) return SN_EINVAL;                  // T - 1 <= 65534 pairs: a grid dimension
    if ((BANDS || PAIR) && (lo < -(1 << 24) || hi > (1 << 24))) return SN_EINVAL;      // the band is 32-bit arithmetic: 4 (S - 4 lo), 2 (S - 8 lo) must fit
    YuvGeo G;
    if (!make_geo(fmt, H, W, rect, &G)) return SN_EINVAL;
    const int n = PAIR ? T - 1 : T;
    int words = 0;
    with_esz(fmt, [&](auto esz) { words = HistK<esz(), KIND, BANDS>::HISTW; });
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(dst, 0, (size_t)n * words * sizeof(uint32_t), s) != hipSuccess) return sn_check_launch();      // dst is overwritten, not added to
    const int hb = G.h / 2, wb = G.w / 2, ux = (wb + 3) / 4;               // the block grid is anchored at the picture's first sample
    if (hb < 1 || wb < 1) return sn_check_launch();                        // no whole block: all-zero histograms
    const long long units = (long long)ux * hb;
    if (units > 0x7fffffffLL - 1024 * 256) return SN_EINVAL;
    // 8 units (32 blocks) per lane, with bands 16: the zeroing, the sum of the copies and the flush (bands: of 40 to 64 KB of LDS) are paid once per
    // 8192 / 16384 blocks, and a 720p frame is 29 / 15 workgroups
    const long long per = BANDS ? 4096 : 2048, wgs = (units + per - 1) / per;
    const dim3 block(256), grid(wgs < 1024 ? (int)wgs : 1024, n);
    with_esz(fmt, [&](auto esz) {
        if constexpr (MV) {
            const HistMvK M = {mv, G.h, G.w, (hb + 7) / 8, (wb + 7) / 8};      // the vector blocks: 8 x 8 of the 2 x 2 blocks
            hipLaunchKernelGGL((yuv_noise_hist_kernel<esz(), KIND, BANDS, HistMvK>), grid, block, 0, s, src, dst, lo, hi, W, hb, wb, ux, G.oy, G.frame_bytes, M);
        } else {
            hipLaunchKernelGGL((yuv_noise_hist_kernel<esz(), KIND, BANDS>), grid, block, 0, s, src, dst, lo, hi, W, hb, wb, ux, G.oy, G.frame_bytes);
        }
    });
    return sn_check_launch();
}

extern "C" {

int sn_yuv_thumb(const uint8_t* src, const sn_yuv_fmt* fmt, uint16_t* dst, int T, int H, int W, void* stream) {
    sn_clear_error();
    if (!valid_payloads(src, fmt, T, H, W) || !dst || ((uintptr_t)dst & 1)) return SN_EINVAL;
    const size_t fb = frame_bytes_of(fmt, H, W);
    const int hb = (H + 7) / 8, wb = (W + 7) / 8;
    const dim3 block(32, 8), grid((wb + 31) / 32, (hb + 7) / 8, T);
    if (grid.y > 65535) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    with_esz(fmt, [&](auto esz) { hipLaunchKernelGGL((yuv_thumb_kernel<esz()>), grid, block, 0, s, src, dst, H, W, hb, wb, fb); });
    return sn_check_launch();
}

int sn_yuv_noise_hist(const uint8_t* src, const sn_yuv_fmt* fmt, uint32_t* dst, int lo, int hi, int T, int H, int W, void* stream) {
    return noise_hist<HIST_SPATIAL, false>(src, fmt, nullptr, nullptr, dst, lo, hi, T, H, W, stream);
}

int sn_yuv_noise_hist_rect(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, uint32_t* dst, int lo, int hi, int T, int H, int W,
                           void* stream) {
    if (!rect) { sn_clear_error(); return SN_EINVAL; }
    return noise_hist<HIST_SPATIAL, false>(src, fmt, rect, nullptr, dst, lo, hi, T, H, W, stream);
}

int sn_yuv_noise_hist_bands(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, uint32_t* dst, int lo, int hi, int T, int H, int W,
                            void* stream) {
    return noise_hist<HIST_SPATIAL, true>(src, fmt, rect, nullptr, dst, lo, hi, T, H, W, stream);
}

int sn_yuv_noise_hist_pairs(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, uint32_t* dst, int lo, int hi, int T, int H, int W,
                            void* stream) {
    return noise_hist<HIST_PAIRS, false>(src, fmt, rect, nullptr, dst, lo, hi, T, H, W, stream);
}

int sn_yuv_noise_hist_pairs_bands(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, uint32_t* dst, int lo, int hi, int T, int H, int W,
                                  void* stream) {
    return noise_hist<HIST_PAIRS, true>(src, fmt, rect, nullptr, dst, lo, hi, T, H, W, stream);
}

int sn_yuv_noise_hist_pairs_mv(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const int8_t* mv, uint32_t* dst, int lo, int hi, int T,
                               int H, int W, void* stream) {
    return noise_hist<HIST_PAIRS_MV, false>(src, fmt, rect, mv, dst, lo, hi, T, H, W, stream);
}

int sn_yuv_noise_hist_pairs_bands_mv(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const int8_t* mv, uint32_t* dst, int lo, int hi,
                                     int T, int H, int W, void* stream) {
    return noise_hist<HIST_PAIRS_MV, true>(src, fmt, rect, mv, dst, lo, hi, T, H, W, stream);
}

// The vectors of the 16 x 16 blocks of every pair: nothing to zero, every word of mv and sad is written by the one workgroup that owns it
int sn_yuv_block_motion(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, int8_t* mv, uint32_t* sad, int T, int H, int W, void* stream) {
    sn_clear_error();
    if (!valid_payloads(src, fmt, T, H, W) || T < 2 || !mv || !sad || ((uintptr_t)sad & 3)) return SN_EINVAL;
    YuvGeo G;
    if (!make_geo(fmt, H, W, rect, &G)) return SN_EINVAL;
    const int hb = G.h / 2, wb = G.w / 2, nby = (hb + 7) / 8, nbx = (wb + 7) / 8;      // the block grid is anchored at the picture's first sample
    if (nby > 65535) return SN_EINVAL;                                     // a grid dimension
    if (hb < 1 || wb < 1) return sn_check_launch();                        // no whole block: no vector block, nothing is written
    const dim3 block(256), grid((nbx + MV_RUN - 1) / MV_RUN, nby, T - 1);
    hipStream_t s = (hipStream_t)stream;
    with_esz(fmt, [&](auto esz) {
        hipLaunchKernelGGL((yuv_block_motion_kernel<esz()>), grid, block, 0, s, src, mv, sad, G.h, G.w, W, hb, wb, nbx, G.oy, G.frame_bytes);
    });
    return sn_check_launch();
}

int sn_noise_map_level(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const float* knots, int lo, int hi, void* dst, int dst_dtype,
                       int T, int H, int W, int Hp, int Wp, void* stream) {
    sn_clear_error();
    if (!valid_payloads(src, fmt, T, H, W) || !dst || !knots || dst_dtype < 0 || dst_dtype > 2 || lo >= hi) return SN_EINVAL;
    if (lo < -(1 << 24) || hi > (1 << 24)) return SN_EINVAL;               // float(lo) is exact
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
    with_esz(fmt, [&](auto esz) { hipLaunchKernelGGL((noise_map_level_kernel<esz()>), grid, block, 0, s, src, dst, dst_dtype, K, G, Hp, Wp, dst_vec); });
    return sn_check_launch();
}

int sn_yuv_rowcol_sums(const uint8_t* src, const sn_yuv_fmt* fmt, uint32_t* rows, uint32_t* cols, int T, int H, int W, void* stream) {
    sn_clear_error();
    if (!valid_payloads(src, fmt, T, H, W) || !rows || !cols || H > 65535 || W > 65535 || ((uintptr_t)rows & 3) || ((uintptr_t)cols & 3)) return SN_EINVAL;
    const size_t fb = frame_bytes_of(fmt, H, W);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(rows, 0, (size_t)T * H * sizeof(uint32_t), s) != hipSuccess) return sn_check_launch();       // both are overwritten, not added to
    if (hipMemsetAsync(cols, 0, (size_t)T * W * sizeof(uint32_t), s) != hipSuccess) return sn_check_launch();
    const dim3 block(64, 4), grid((W + 511) / 512, (H + 4 * ROWCOL_STRIP - 1) / (4 * ROWCOL_STRIP), T);
    with_esz(fmt, [&](auto esz) { hipLaunchKernelGGL((yuv_rowcol_kernel<esz()>), grid, block, 0, s, src, rows, cols, H, W, fb); });
    return sn_check_launch();
}

int sn_yuv_diff_stats(const uint8_t* a, const uint8_t* b, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, int edge, int64_t* dst, int T, int H, int W,
                      void* stream) {
    sn_clear_error();
    if (!valid_payloads(a, fmt, T, H, W) || !b || !aligned_payload(fmt, b) || !dst || ((uintptr_t)dst & 7) || edge < 0) return SN_EINVAL;
    YuvGeo G;
    if (!make_geo(fmt, H, W, rect, &G)) return SN_EINVAL;
    const bool sub = fmt->chroma != SN_YUV_444;
    const int ch = sub ? (G.h + 1) / 2 : G.h, cw = sub ? (G.w + 1) / 2 : G.w;      // the picture's chroma planes (a legal rectangle shares no chroma sample)
    const long long units = (long long)((G.w + 7) / 8) * ((G.h + DS_STRIP - 1) / DS_STRIP);      // the chroma planes have no more
    if (units > 0x7fffffffLL - 1024 * 256) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(dst, 0, (size_t)T * SN_DIFF_STATS * sizeof(int64_t), s) != hipSuccess) return sn_check_launch();      // dst is overwritten, not added to
    const long long wgs = (units + 255) / 256;                             // one unit (64 pixels) per lane: a 720p frame is 57 workgroups
    const dim3 block(256), grid(wgs < 1024 ? (int)wgs : 1024, T);
    with_esz(fmt, [&](auto esz) {
        hipLaunchKernelGGL((yuv_diff_stats_kernel<esz()>), grid, block, 0, s, a, b, (unsigned long long*)dst, G, ch, cw, edge, T);
    });
    return sn_check_launch();
}

int sn_yuv_diff_stats_mv(const uint8_t* a, const uint8_t* b, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, const int8_t* mv, int64_t* dst, int T, int H, int W,
                         void* stream) {
    sn_clear_error();
    if (!valid_payloads(a, fmt, T, H, W) || !b || !aligned_payload(fmt, b) || !dst || ((uintptr_t)dst & 7) || T < 2 || !mv) return SN_EINVAL;
    YuvGeo G;
    if (!make_geo(fmt, H, W, rect, &G)) return SN_EINVAL;
    const long long bound = (long long)((G.w + 7) / 8) * ((G.h + DS_STRIP - 1) / DS_STRIP);      // the bound of sn_yuv_diff_stats; the units here are no more
    if (bound > 0x7fffffffLL - 1024 * 256) return SN_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(dst, 0, (size_t)(T - 1) * SN_DIFF_STATS_MV * sizeof(int64_t), s) != hipSuccess) return sn_check_launch();      // dst is overwritten, not added to
    const int hb = G.h / 2, wb = G.w / 2;                                  // the block grid is anchored at the picture's first sample
    if (hb < 1 || wb < 1) return sn_check_launch();                        // no whole block: all zeros
    const long long units = (long long)((wb + 3) / 4) * ((hb + 3) / 4);
    const long long wgs = (units + 255) / 256;                             // one unit (64 pixels) per lane: a 720p frame is 57 workgroups
    const dim3 block(256), grid(wgs < 1024 ? (int)wgs : 1024, T - 1);
    with_esz(fmt, [&](auto esz) {
        hipLaunchKernelGGL((yuv_diff_stats_mv_kernel<esz()>), grid, block, 0, s, a, b, mv, (unsigned long long*)dst, G, hb, wb, (hb + 7) / 8, (wb + 7) / 8);
    });
    return sn_check_launch();
}

}  // extern "C"
