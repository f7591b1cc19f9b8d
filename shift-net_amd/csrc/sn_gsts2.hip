// Second-generation GSTS kernels (gfx950): fewer passes over HBM, stencils fed from LDS.
//
//   sn_ln_gemm_gate   (K12): g1 = SimpleGate(RepConv2(body[0](norm(u))))  -- LayerNorm + 1x1 (MFMA) + depthwise 3x3 +
//                      gate in ONE kernel; the 2C-channel tensor `a` (the widest tensor of the block) never reaches HBM.
//                      One workgroup owns an 8x32 output tile; LN+GEMM run on the tile plus a 1-pixel ring (340 px,
//                      1.33x recompute); `a` goes to LDS 32 channels at a time (gate-paired chunks), the normalised
//                      operands stay in registers as MFMA B fragments for the whole chunk loop.
//   sn_grp5_gemm_gate (K3g): the grouped RepConv of the "+" variants as a block-diagonal MFMA GEMM + 1x1 + SimpleGate2 (below).
#include "sn_common.h"
#include "../../include/shiftnet_hip.h"

namespace {

struct UnitK2 {
    const bf16_t* x; const bf16_t* halo;
    int T, h, w, C, mode, wrap, t0, clip;      // clip: frames per clip, T for one clip (sn_clip_len)
};

// ------------------------------------------------------------------------------------------------------------
#define SN_K12_TH 8
#define SN_K12_NWV 8
template <int C, bool WITH_HW>
__global__ __launch_bounds__(SN_K12_NWV * 64) void ln_gemm_gate_kernel(const UnitK2 U, const XcdTiles G, const bf16_t* __restrict__ hwb, const uint4* __restrict__ wfrag,
                                                         const float* __restrict__ bias, const uint32_t* __restrict__ wdw,
                                                         bf16_t* g1, float* pool, const int blocked) {
    constexpr int CH = C / 2, K = WITH_HW ? C + CH : C, KS = (K + 31) / 32, MT = C / 8, NCHK = MT / 2;
    constexpr int TH = SN_K12_TH, TW = 32, RH = TH + 2, RW = TW + 2, NPX = RH * RW;  // tile + 1-pixel ring (8x32: 340 px, 16x32: 612 px)
    constexpr int NWV = SN_K12_NWV;                                                // waves per workgroup
    constexpr int NTILES = (NPX + 15) / 16, NTW = (NTILES + NWV - 1) / NWV;        // 22 N-tiles, <= 3 per wave
    constexpr int PSA = 80;                                                        // LDS bytes per pixel of an a-chunk (64 + 16 pad)
    __shared__ __attribute__((aligned(16))) char lds_a2[2][NPX * PSA];           // double-buffered a-chunk: one barrier per chunk
    __shared__ __attribute__((aligned(16))) uint16_t lds_tr[NWV][8][64];          // per-wave transpose scratch of the planar epilogue
    const int lane = threadIdx.x & 63, wv = wave_id(), g = lane >> 4, p = lane & 15;
    int t, tyi, txi;
    if (!sn_xcd_tile(G, t, tyi, txi)) return;     // XCD-aware walk (sn_common.h): ring rows / columns of neighbouring tiles meet in one L2
    t += U.t0;
    const int oy0 = tyi * TH, ox0 = txi * TW;
    const int hw = U.h * U.w;
    const SnSlabs<bf16_t> sl = sn_unit_slabs<bf16_t>(U.x, U.halo, U.T, hw, C, U.mode, U.wrap, U.clip, t);

    // weight fragments and bias of one chunk, fetched one chunk AHEAD (they come from L2: ~1 us when loaded at the point of use)
    bf16x8_t Wf[2][KS];
    float4 Wb[2];
    auto load_w = [&](int q) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            Wf[0][s] = as_frag(wfrag[((2 * q) * KS + s) * 64 + lane]);
            Wf[1][s] = as_frag(wfrag[((2 * q + 1) * KS + s) * 64 + lane]);
        }
        Wb[0] = *(const float4*)(bias + g * 4 * MT + (2 * q) * 4);
        Wb[1] = *(const float4*)(bias + g * 4 * MT + (2 * q + 1) * 4);
    };
    load_w(0);

    // ---- LayerNorm of every pixel of the ring-extended tile; results stay in registers as MFMA B fragments ----
    // Lane group g reads k-slots [s*32 + g*8, +8) of its pixel: which slab that is (first / second half of x, or hw) depends on
    // (s, g) only, so ONE 64-bit slab pointer and pixel stride per k-step are chosen up front and a load costs a 32-bit multiply
    // and one 64-bit add (the former per-load pointer selects were ~100 VALU instructions of this VALU-bound kernel).
    const bf16_t* slab[KS];
    int sstride[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int kk0 = s * 32 + g * 8;
        const bf16_t* b0 = sl.p0 + (kk0 < CH ? kk0 : 0);
        const bf16_t* b1 = sl.p1 + (kk0 >= CH && kk0 < C ? kk0 - CH : 0);
        slab[s] = kk0 < CH ? b0 : b1;                   // padding slots (kk0 >= K) re-read x and are zeroed below
        sstride[s] = kk0 < CH ? sl.s0 : sl.s1;          // C, or C/2 for the halo half-frame of a temporally split window
        if (WITH_HW) {
            const bf16_t* b2 = hwb + (size_t)t * hw * CH + (kk0 >= C && kk0 < K ? kk0 - C : 0);
            const bool ishw = kk0 >= C && kk0 < K;
            slab[s] = ishw ? b2 : slab[s];
            sstride[s] = ishw ? CH : sstride[s];
        }
    }
    bf16x8_t B[NTW][KS];
    bool inimg[NTW];
#pragma unroll
    for (int n = 0; n < NTW; ++n) {
        const int tile = wv + NWV * n;
        const int rp = tile * 16 + p;                         // pixel index inside the region
        const int ry = rp / RW, rx = rp - ry * RW;
        const int gy = oy0 - 1 + ry, gx = ox0 - 1 + rx;
        const bool in = (tile < NTILES) && (rp < NPX) && gy >= 0 && gy < U.h && gx >= 0 && gx < U.w;
        inimg[n] = in;
        const int ii = in ? gy * U.w + gx : 0;
        // branch-free: ALWAYS load (a load inside a divergent branch is waited for on the spot, one memory round trip per slab)
        uint4 raw[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) raw[s] = *(const uint4*)(slab[s] + ii * sstride[s]);
        f32x2_t xv[KS][4];
        f32x2_t sum2 = {0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            uint4 q = raw[s];
            if ((KS - 1) * 32 + 24 >= K && s == KS - 1) {     // only the last k-step of the 80-channel variants has padding slots
                const bool has = s * 32 + g * 8 < K;
                q.x = has ? q.x : 0u; q.y = has ? q.y : 0u; q.z = has ? q.z : 0u; q.w = has ? q.w : 0u;
            }
            xv[s][0] = (f32x2_t){bf_lo(q.x), bf_hi(q.x)}; xv[s][1] = (f32x2_t){bf_lo(q.y), bf_hi(q.y)};
            xv[s][2] = (f32x2_t){bf_lo(q.z), bf_hi(q.z)}; xv[s][3] = (f32x2_t){bf_lo(q.w), bf_hi(q.w)};
#pragma unroll
            for (int j = 0; j < 4; ++j) sum2 += xv[s][j];    // packed fp32 (v_pk_add_f32): two partial sums per lane
        }
        const float mean = sum_rows4(sum2[0] + sum2[1]) * (1.0f / K);
        const f32x2_t mean2 = {mean, mean};
        f32x2_t sq2 = {0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const bool pad = (KS - 1) * 32 + 24 >= K && s == KS - 1 && !(s * 32 + g * 8 < K);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x2_t d = xv[s][j] - mean2;
                if ((KS - 1) * 32 + 24 >= K && s == KS - 1) d = pad ? (f32x2_t){0.f, 0.f} : d;
                xv[s][j] = d;
                sq2 = __builtin_elementwise_fma(d, d, sq2);   // v_pk_fma_f32
            }
        }
        const float sq = sum_rows4(sq2[0] + sq2[1]);
        const float rstd = 1.0f / sqrtf(sq * (1.0f / K) + 1e-6f);
        const f32x2_t rstd2 = {rstd, rstd};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            uint4 o;
            f32x2_t a = xv[s][0] * rstd2, b = xv[s][1] * rstd2, c = xv[s][2] * rstd2, d = xv[s][3] * rstd2;
            o.x = pack_bf2(a[0], a[1]); o.y = pack_bf2(b[0], b[1]); o.z = pack_bf2(c[0], c[1]); o.w = pack_bf2(d[0], d[1]);
            B[n][s] = as_frag(o);
        }
    }

    // GEMM chunk q: rows 2q (first-half channels) and 2q+1 (their gate partners) -> LDS buffer q&1, zero outside the image
    auto gemm_chunk = [&](int q) {
        char* lds_a = lds_a2[q & 1];
        f32x4_t acc0[NTW], acc1[NTW];
        const float4 b0 = Wb[0], b1 = Wb[1];
#pragma unroll
        for (int n = 0; n < NTW; ++n) { acc0[n] = (f32x4_t){b0.x, b0.y, b0.z, b0.w}; acc1[n] = (f32x4_t){b1.x, b1.y, b1.z, b1.w}; }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int n = 0; n < NTW; ++n) { acc0[n] = mfma16(Wf[0][s], B[n][s], acc0[n]); acc1[n] = mfma16(Wf[1][s], B[n][s], acc1[n]); }
        }
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
            const int rp = (wv + NWV * n) * 16 + p;
            if (rp < NPX && (wv + NWV * n) < NTILES) {
                uint4 o = make_uint4(0, 0, 0, 0);
                if (inimg[n]) {       // `a` lives in LDS as fp16 (round to nearest): operand of the packed-fp16 stencil below
                    o.x = pack_h2(acc0[n][0], acc0[n][1]); o.y = pack_h2(acc0[n][2], acc0[n][3]);
                    o.z = pack_h2(acc1[n][0], acc1[n][1]); o.w = pack_h2(acc1[n][2], acc1[n][3]);
                }
                *(uint4*)(lds_a + rp * PSA + g * 16) = o;
            }
        }
    };
    gemm_chunk(0);
    load_w(1);
#pragma unroll 1
    for (int q = 0; q < NCHK; ++q) {
        // one barrier per chunk: chunk q is complete in buffer q&1, and every wave is done reading buffer (q+1)&1 (chunk q-1)
        __syncthreads();
        if (q + 1 < NCHK) gemm_chunk(q + 1);            // MFMA work of the next chunk overlaps this chunk's stencil
        load_w(q + 2 < NCHK ? q + 2 : NCHK - 1);        // unconditional (clamped): consumed one iteration later
        const char* lds_a = lds_a2[q & 1];
        // ---- depthwise 3x3 (+identity) and gate.  Wave = (64-pixel group pg, lane-group-slot pair gp): it handles slots
        //      2gp and 2gp+1 one after the other (the slot's weights are wave-uniform scalar loads), lanes are pixels, so a
        //      lane ends up with 8 consecutive g1 channels of the chunk block = ONE 16-byte store per pixel and chunk.
        {
            static_assert(NWV == 2 * ((TH * TW) / 64), "K12 stencil mapping: two waves per 64-pixel group");
            const int pg = wv % ((TH * TW) / 64), gp = wv / ((TH * TW) / 64);
            const int op = pg * 64 + lane, oy = op / TW, ox = op - oy * TW;
            const int gy = oy0 + oy, gx = ox0 + ox;
            const bool inside = gy < U.h && gx < U.w;
            uint32_t ow[4];
#pragma unroll
            for (int gi = 0; gi < 2; ++gi) {
                const int gs = gp * 2 + gi;
                // Depthwise 3x3 (+identity) as PACKED fp16 FMAs: a dword of the chunk image holds positions (2k, 2k+1) of one pixel,
                // the weight word the two matching fp16 taps, so one v_pk_fma_f16 (full-rate VALU) does two MACs -- the former
                // one-hot v_dot2c_f32_bf16 did one MAC in 4.8 cycles and this loop was 35 % of the kernel (VALU-bound).
                // |a| is O(10) after the LayerNorm'd 1x1, nine fp16 products accumulate with 2^-11 relative steps: tighter than the
                // bf16 rounding of the old operands (the folded identity tap 1 + w is exact to 2^-11 instead of 2^-8).
                h2_t wt[9][4];                // fp16 weights of positions (2k, 2k+1), k = 0..3, per tap (wave-uniform: scalar loads)
#pragma unroll
                for (int tp = 0; tp < 9; ++tp)
#pragma unroll
                    for (int k = 0; k < 4; ++k) wt[tp][k] = __builtin_bit_cast(h2_t, wdw[tp * C + gs * 2 * MT + q * 4 + k]);
                h2_t o2[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) o2[k] = (h2_t){(_Float16)0.f, (_Float16)0.f};
                {
#pragma unroll
                    for (int ty = 0; ty < 3; ++ty)
#pragma unroll
                        for (int tx = 0; tx < 3; ++tx) {
                            const uint4 v = *(const uint4*)(lds_a + ((oy + ty) * RW + ox + tx) * PSA + gs * 16);
                            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                            for (int k = 0; k < 4; ++k) o2[k] = __builtin_elementwise_fma(__builtin_bit_cast(h2_t, d[k]), wt[ty * 3 + tx][k], o2[k]);
                        }
                }
                float o[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) { o[2 * k] = (float)o2[k][0]; o[2 * k + 1] = (float)o2[k][1]; }
                const float r0 = o[0] * o[4], r1 = o[1] * o[5], r2 = o[2] * o[6], r3 = o[3] * o[7];
                ow[2 * gi] = pack_bf2(r0, r1); ow[2 * gi + 1] = pack_bf2(r2, r3);
                if (pool) {                   // denoise CALayer2 on g1: per-wave channel sums (4 channels of slot gs)
                    float ps[4] = {inside ? r0 : 0.f, inside ? r1 : 0.f, inside ? r2 : 0.f, inside ? r3 : 0.f};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float sm = ps[j];
                        sm = row_sum16(sm);
                        sm += __shfl_xor(sm, 16); sm += __shfl_xor(sm, 32);
                        if (lane == 0) {
                            constexpr int NPG = (TH * TW) / 64;
                            const int nblk = NPG * G.ntx * G.nty, blk = NPG * (tyi * G.ntx + txi) + pg;
                            pool[((size_t)t * nblk + blk) * C + gs * 2 * MT + q * 4 + j] = sm;
                        }
                    }
                }
            }
            if (blocked == 2) {
                // channel-planar g1 [T][h][C][wr] for the matrix-core stencil (sn_gsts3.hip): the wave's 64 pixels x 8 channels
                // go through a wave-private LDS transpose (LDS operations of one wave execute in order: no barrier), then every
                // lane stores 8 consecutive columns of one channel (16 B).  Pixels outside the image are written as zeros
                // (pad columns w .. wr-1 must read as zero downstream).
                uint16_t (*tr)[64] = lds_tr[wv];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t v = inside ? ow[k] : 0u;
                    tr[2 * k][lane] = (uint16_t)(v & 0xffffu);
                    tr[2 * k + 1][lane] = (uint16_t)(v >> 16);
                }
                const int ci = lane >> 3, xc = lane & 7;                              // channel index 0..7 of this wave's set, 8-pixel piece
                const uint4 v = *(const uint4*)(&tr[ci][xc * 8]);
                const int ch = (gp * 2 + (ci >> 2)) * 2 * MT + q * 4 + (ci & 3);      // slot gs = 2gp + (ci>>2), r = ci & 3
                const int py = oy0 + pg * (64 / TW) + (xc >> 2), pxx = ox0 + (xc & 3) * 8;
                const int wr = (U.w + 7) & ~7;
                if (py < U.h && pxx < wr) *(uint4*)(g1 + (((size_t)t * U.h + py) * C + ch) * wr + pxx) = v;
            } else if (inside) {
                const size_t pix = (size_t)gy * U.w + gx;
                bf16_t* dst = g1 + ((size_t)t * hw + pix) * C + q * 4;          // natural NHWC
                *(uint2*)(dst + (gp * 2) * 2 * MT) = make_uint2(ow[0], ow[1]);
                *(uint2*)(dst + (gp * 2 + 1) * 2 * MT) = make_uint2(ow[2], ow[3]);
            }
        }
    }
}


// ------------------------------------------------------------------------------------------------------------
// K3g ("+" variants, RepConv with groups = C/8): grouped 5x5 (+3x3 +identity folded) as a block-diagonal MFMA GEMM
// (one M-tile = two groups of 8 output channels, K = 25 taps x their 16 input channels, half of each A fragment is zero),
// then the 1x1 C -> 2C, SimpleGate2 and the channel sums.  Tile 32 x 4 pixels, g1 region (+2 ring, all C channels) in LDS.
//
// Second generation.  The first one (one workgroup per tile, every wave walking ALL M-tiles of its 32 pixels) re-read
// every weight fragment from L1/L2 for every 32 pixels: 125 KB of A operands per wave-tile against 5 KB of activations,
// ~60 clk per pixel and CU on the vector-memory path alone (1120 us at the level-1 size of config 2 vs 381 us for the
// depthwise kernel).  Here the WEIGHTS STAY IN REGISTERS: a persistent workgroup of 10 waves, wave (m, nh) owns M-tile m of
// the grouped conv (13 fragments) and gate pair m of the 1x1 (6 fragments) for the four N-tiles of half nh of every tile it
// walks, so the only operand traffic inside the tile loop is LDS reads of activations:
//   stage (HBM -> registers one tile AHEAD -> LDS, optional CALayer2 scale) | grouped MFMAs -> r tile in LDS | 1x1 MFMAs,
//   gate -> output tile in LDS (over the dead g1 region) | coalesced 16-byte NHWC stores + channel sums.
// NH = pixel halves per tile = waves per M-tile: NH = 1 -> 5 waves (320 threads) per workgroup and TWO independent workgroups per
// CU (one computes while the other waits for its loads); NH = 2 -> one 10-wave workgroup per CU.
template <int C, int NH>
__global__ __launch_bounds__(64 * NH * (C / 16), 3) void grp5p_gemm_gate_kernel(const bf16_t* __restrict__ g1, const float* __restrict__ ca_in,
                                                            const uint4* __restrict__ wgrp, const uint4* __restrict__ wfrag,
                                                            bf16_t* g2, float* pool, int T, int h, int w) {
    // PS = LDS bytes per pixel = 10 slots of 16 B, NO padding: ds_read_b128 is serviced in the lane groups {0-3,12-15,20-27}, ...
    // (MI355X_MICROARCH.md), i.e. half a group reads chunk g&1 = 0 of 8 pixels and the other half chunk 1 of 8 OTHER pixels; with
    // slot = 10 p + (g&1) the 16 lanes of every group hit 16 distinct slots, while the "odd number of slots" padding (11) that suits
    // 16 consecutive lanes collides on 3 of 16 (measured: the grouped-MFMA phase was LDS-bound).
    constexpr int TY = 4, TXW = 32, RH = TY + 4, RW = TXW + 4, PS = C * 2, MTG = C / 16, KSG = 13;
    constexpr int KS = (C + 31) / 32, NPC = C / 8, NTL = (TY * TXW) / 16, NTWV = NTL / NH, NTHR = 64 * NH * MTG;
    constexpr int NITEM = RH * RW * NPC, NIT = (NITEM + NTHR - 1) / NTHR;
    static_assert(C == 80 && (NH == 1 || NH == 2), "wave roles are laid out for C = 80 (5 group pairs x NH pixel halves)");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* lds_g = smem;                                  // [RH*RW][PS] staged g1 region; reused as the [TY*TXW][PS] output tile
    char* lds_r = smem + RH * RW * PS;                   // [TY*TXW][PS] RepConv output
    float* red = (float*)(lds_r + TY * TXW * PS);        // [NH][C]
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), g = lane >> 4, p = lane & 15;
    const int m = wv % MTG, nh = wv / MTG;
    const int tiles_x = (w + TXW - 1) / TXW, tiles_y = (h + TY - 1) / TY, tpf = tiles_x * tiles_y, ntiles = T * tpf;

    // resident weights: the 13 grouped-conv fragments of M-tile m (52 VGPRs).  The 6 fragments of gate pair m (rows 2m, 2m+1 of
    // the gate-paired order) are re-fetched once per tile: keeping them resident too pushes the kernel over the 168 registers
    // that 10 waves per CU allow (scratch spills).
    bf16x8_t A1[KSG];
#pragma unroll
    for (int s = 0; s < KSG; ++s) A1[s] = as_frag(wgrp[(m * KSG + s) * 64 + lane]);
    // staging plan (the same region items for every tile): item idx -> (region pixel, 16-byte piece), recomputed where needed
    // (divisions by constants) instead of kept live
    uint4 stg[NIT];
    bool sin[NIT];
    auto item = [&](int k, int& pix, int& pc) {
        int idx = tid + k * NTHR;
        asm volatile("" : "+v"(idx));                      // opaque: keeps LICM from hoisting (and then spilling) the results
        pix = idx / NPC; pc = idx - pix * NPC;
        return idx < NITEM;
    };
    auto issue_loads = [&](int tile) {                   // branch-free (clamped) loads; masks are applied at the LDS write
        const int t = tile / tpf, rem = tile - t * tpf, ty = rem / tiles_x, tx = rem - ty * tiles_x;
        const bf16_t* gt = g1 + (size_t)t * h * w * C;
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            int pix, pc;
            const bool live = item(k, pix, pc);
            const int ry = pix / RW, rx = pix - ry * RW, gy = ty * TY - 2 + ry, gx = tx * TXW - 2 + rx;
            sin[k] = live && gy >= 0 && gy < h && gx >= 0 && gx < w;
            stg[k] = *(const uint4*)(gt + (sin[k] ? (gy * w + gx) * C + pc * 8 : 0));
        }
    };

    // persistent, XCD-aware walk (workgroup b runs on XCD b % 8): each XCD takes a contiguous eighth of the tile list
    const int nxcd = (gridDim.x % 8 == 0) ? 8 : 1, wpx = gridDim.x / nxcd, seg = (ntiles + nxcd - 1) / nxcd;
    const int seg0 = (blockIdx.x % nxcd) * seg, seg1 = seg0 + seg < ntiles ? seg0 + seg : ntiles;
    int tile = seg0 + blockIdx.x / nxcd;
    if (tile < seg1) issue_loads(tile);
    for (; tile < seg1; tile += wpx) {
        const int t = tile / tpf, rem = tile - t * tpf, tyi = rem / tiles_x, txi = rem - tyi * tiles_x;
        const int y0 = tyi * TY, x0 = txi * TXW;
        // ---- registers -> LDS (optional CALayer2 scale of the denoise variants), then prefetch the next tile ----
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            int pix, pc;
            if (!item(k, pix, pc)) continue;
            uint4 q = sin[k] ? stg[k] : make_uint4(0, 0, 0, 0);
            if (ca_in && sin[k]) {
                float f[8];
                unpack8(q, f);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] *= ca_in[(size_t)t * C + pc * 8 + j];
                q = pack8(f);
            }
            *(uint4*)(lds_g + pix * PS + pc * 16) = q;
        }
        __syncthreads();
        // gate-pair fragments of this tile (L1/L2 hits) FIRST, then the next tile's staging loads: vmcnt retires in order, so
        // waiting for the fragments before phase 2 must not also wait for the HBM loads issued behind them
        bf16x8_t A2[2][KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            A2[0][s] = as_frag(wfrag[((2 * m) * KS + s) * 64 + lane]);
            A2[1][s] = as_frag(wfrag[((2 * m + 1) * KS + s) * 64 + lane]);
        }
        {
            const int ntile = tile + wpx < seg1 ? tile + wpx : tile;      // past the end: re-read this tile (harmless)
            issue_loads(ntile);
        }
        // ---- grouped 5x5: k-step s covers taps 2s, 2s+1; lane group g -> tap 2s + (g>>1), input channels 16m + (g&1)*8 .. ----
        // (four N-tiles at a time: 16 accumulator registers live next to the 52 of the resident fragments)
#pragma unroll 1
        for (int n0 = 0; n0 < NTWV; n0 += 4) {
            f32x4_t acc[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
            int pb[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int nt = NTWV * nh + n0 + n, row = nt >> 1, xb = nt & 1;
                pb[n] = (row * RW + xb * 16 + p) * PS + (g & 1) * 16 + m * 32;
            }
            // B fragments one k-step AHEAD (explicit double buffer): left to itself hipcc waits for every ds_read right before
            // the MFMA that consumes it (s_waitcnt lgkmcnt(0) x 52: the LDS latency, ~100 cycles, exposed per MFMA)
            auto toff_of = [&](int s) {
                int tap = 2 * s + (g >> 1);
                tap = tap < 25 ? tap : 0;                  // the 26th slot has zero weights: any valid address will do
                const int dy = tap / 5, dx = tap - dy * 5;
                return (dy * RW + dx) * PS;
            };
            uint4 Bq[2][4];
            {
                const int t0 = toff_of(0);
#pragma unroll
                for (int n = 0; n < 4; ++n) Bq[0][n] = *(const uint4*)(lds_g + pb[n] + t0);
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);          // prologue reads of step 0 (see the loop)
#pragma unroll
            for (int s = 0; s < KSG; ++s) {
                if (s + 1 < KSG) {
                    const int t1 = toff_of(s + 1);
#pragma unroll
                    for (int n = 0; n < 4; ++n) Bq[(s + 1) & 1][n] = *(const uint4*)(lds_g + pb[n] + t1);
                }
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[n] = mfma16(A1[s], as_frag(Bq[s & 1][n]), acc[n]);
                // pin the issue order: the 4 ds_reads of step s+1, THEN the 4 MFMAs of step s (the scheduler otherwise sinks each
                // read next to its consumer and the wave waits out one LDS latency per MFMA)
                if (s + 1 < KSG) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                uint2 o; o.x = pack_bf2(acc[n][0], acc[n][1]); o.y = pack_bf2(acc[n][2], acc[n][3]);
                *(uint2*)(lds_r + ((NTWV * nh + n0 + n) * 16 + p) * PS + (m * 16 + g * 4) * 2) = o;
            }
        }
        __syncthreads();                                   // r complete; every wave is done reading the g1 region
        // ---- 1x1 C -> 2C, gate pair m: channels 2*MT*g + 4m + rr of the gate-paired order (MT = C/8), SimpleGate2 ----
        float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int n0 = 0; n0 < NTWV; n0 += 2) {             // two N-tiles at a time: all six B reads first, then the twelve MFMAs
            uint4 Bf[2][KS];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const int kk0 = s * 32 + g * 8, tpj = (NTWV * nh + n0 + j) * 16 + p;
                    Bf[j][s] = kk0 < C ? *(const uint4*)(lds_r + tpj * PS + kk0 * 2) : make_uint4(0, 0, 0, 0);
                }
            f32x4_t a0[2], a1[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) { a0[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; a1[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int s = 0; s < KS; ++s)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    a0[j] = mfma16(A2[0][s], as_frag(Bf[j][s]), a0[j]);
                    a1[j] = mfma16(A2[1][s], as_frag(Bf[j][s]), a1[j]);
                }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int tp = (NTWV * nh + n0 + j) * 16 + p;
                float v[4];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) v[rr] = a0[j][rr] * sigmoidf_(a1[j][rr]);
                const int oyv = y0 + (tp >> 5), oxv = x0 + (tp & 31);
                if (oyv < h && oxv < w) {
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) ps[rr] += v[rr];
                }
                uint2 o; o.x = pack_bf2(v[0], v[1]); o.y = pack_bf2(v[2], v[3]);
                *(uint2*)(lds_g + tp * PS + (g * (C / 4) + 4 * m) * 2) = o;      // output tile over the dead g1 region
            }
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const float sm = row_sum16(ps[rr]);
            if (p == 0) red[nh * C + g * (C / 4) + 4 * m + rr] = sm;
        }
        __syncthreads();                                   // output tile and red complete
        // ---- coalesced NHWC stores: 16-byte pieces, consecutive lanes = consecutive addresses of a pixel's C channels ----
        for (int it = tid; it < TY * TXW * NPC; it += NTHR) {
            const int px = it / NPC, pc = it - px * NPC;
            const int oy = y0 + (px >> 5), ox = x0 + (px & 31);
            if (oy < h && ox < w) *(uint4*)(g2 + (((size_t)t * h + oy) * w + ox) * C + pc * 8) = *(const uint4*)(lds_g + px * PS + pc * 16);
        }
        if (pool && tid < C) pool[((size_t)t * tpf + rem) * C + tid] = NH == 2 ? red[tid] + red[C + tid] : red[tid];
        __syncthreads();                                   // the output tile (g1 region) and red are rewritten by the next tile
    }
}

}  // namespace

extern "C" {

int sn_lngate_blocks(int h, int w) { return (SN_K12_TH * 32 / 64) * ((h + SN_K12_TH - 1) / SN_K12_TH) * ((w + 31) / 32); }

int sn_ln_gemm_gate(const sn_unit_src* s, const void* hw, const void* wfrag, const float* bias, const uint32_t* wdw,
                    void* g1, float* pool, int g1_blocked, void* stream) {
    sn_clear_error();
    if (!s || !s->x || (s->C != 64 && s->C != 80) || s->T < 1 || s->h < 1 || s->w < 1 || s->mode < 0 || s->mode > 2 || !wfrag || !bias || !wdw || !g1 ||
        (s->mode != 0 && !hw) || (g1_blocked && s->C != 64) || (g1_blocked != 0 && g1_blocked != 2) || (s->wrap == 2 && s->mode != 0 && !s->halo))
        return SN_EINVAL;
    UnitK2 u; u.x = (const bf16_t*)s->x; u.halo = (const bf16_t*)s->halo; u.T = s->T; u.h = s->h; u.w = s->w; u.C = s->C; u.mode = s->mode; u.wrap = s->wrap; u.clip = sn_clip_len(s->T, s->clip);
    SN_FRAME_RANGE(s, t0, nt);
    u.t0 = t0;
    const XcdTiles G = sn_xcd_tiles((s->w + 31) / 32, (s->h + SN_K12_TH - 1) / SN_K12_TH, nt);
    const dim3 grid = sn_xcd_grid(G);
    hipStream_t st = (hipStream_t)stream;
#define SN_LAUNCH_K12(CC, HW_) hipLaunchKernelGGL((ln_gemm_gate_kernel<CC, HW_>), grid, dim3(SN_K12_NWV * 64), 0, st, u, G, (const bf16_t*)hw, \
        (const uint4*)wfrag, bias, wdw, (bf16_t*)g1, pool, g1_blocked)
    if (s->C == 64) { if (s->mode) SN_LAUNCH_K12(64, true); else SN_LAUNCH_K12(64, false); }
    else { if (s->mode) SN_LAUNCH_K12(80, true); else SN_LAUNCH_K12(80, false); }
#undef SN_LAUNCH_K12
    return sn_check_launch();
}


int sn_grp5_blocks(int h, int w) { return ((h + 3) / 4) * ((w + 31) / 32); }

int sn_grp5_gemm_gate(const void* g1, const float* ca_in, const void* wgrp, const void* wfrag, void* g2, float* pool,
                      int T, int h, int w, int C, void* stream) {
    sn_clear_error();
    if (!g1 || !wgrp || !wfrag || !g2 || C != 80 || T < 1 || h < 1 || w < 1) return SN_EINVAL;
    const size_t lds = (size_t)(8 * 36 + 4 * 32) * (C * 2) + 2 * C * sizeof(float);             // 67200 B
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1)
        return SN_ELAUNCH;
    constexpr int NH = 2;      /* measured on config 3: NH = 2 (one 10-wave workgroup per CU) 123.6 ms, NH = 1 (two 5-wave workgroups) 180.1 ms */
    if (hipFuncSetAttribute((const void*)grp5p_gemm_gate_kernel<80, NH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return SN_ELAUNCH;
    const int ntiles = T * ((h + 3) / 4) * ((w + 31) / 32);
    const int maxwg = (NH == 1 ? 2 : 1) * ncu, nwg = ntiles < maxwg ? ntiles : maxwg;            // persistent, all workgroups resident
    sn_clear_error();
    hipLaunchKernelGGL((grp5p_gemm_gate_kernel<80, NH>), nwg, dim3(64 * NH * 5), lds, (hipStream_t)stream, (const bf16_t*)g1, ca_in,
                       (const uint4*)wgrp, (const uint4*)wfrag, (bf16_t*)g2, pool, T, h, w);
    return sn_check_launch();
}

}  // extern "C"
