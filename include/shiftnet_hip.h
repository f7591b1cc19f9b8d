/* shiftnet_hip.h -- C ABI of libshiftnet_hip.so: the MI355X (gfx950) kernels behind GShiftNet.forward.
 *
 * The reference has no native code and no FFI: its "operators" are the ATen calls made by
 * basicsr/models/archs/gshift_{deblur,denoise}{1,2}.py.  This header is the boundary a maintainer binds instead
 * (ctypes stub: INTEGRATION.md).  Each entry point names the reference expression it replaces.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless said otherwise; the caller owns every buffer (outputs and workspaces
 *     included), the library never allocates or frees, reads no environment variable and keeps no global mutable
 *     state (thread compatible).  Kernels launch on the calling thread's CURRENT HIP device: make the device that owns
 *     `stream` and the buffers current first (the Python engine wraps every forward in torch.cuda.device(dev));
 *   - work is enqueued on `stream` (a hipStream_t passed as void*) and returns immediately;
 *   - return 0 on success, negative errno-style code otherwise (-22 bad argument, -5 launch failure); nothing throws;
 *   - activations: NHWC bf16 [T][H][W][Cs], Cs a multiple of 8, pad channels must be (and are kept) zero;
 *   - "wfrag" arguments are weights prepacked by the host into MFMA A-fragment order (shiftnet_amd/prep.py):
 *     bf16 [MT][KS][64 lanes][8], see csrc/sn_common.h for the lane/slot convention.
 */
#ifndef SHIFTNET_HIP_H
#define SHIFTNET_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SN_ABI_VERSION 20    /* bump on ANY change of a struct, signature or operand encoding (shiftnet_amd/lib.py checks it) */

/* element types of NCHW tensors exchanged with the PyTorch side */
#define SN_F32 0
#define SN_F16 1
#define SN_BF16 2

int sn_abi_version(void);

/* MFMA lane-layout self test: D = A.B on one 16x16x32 tile with asymmetric operands written in the slot
 * convention of sn_common.h.  a:[16][32] f32, b:[32][16] f32 row major, d:[16][16] f32 out (all device). */
int sn_selftest_mfma(const float* a, const float* b, float* d, void* stream);

/* x = x[0]; torch.cat((x, noise_map), 1) and the implicit NCHW->kernel layout change
 * (gshift_deblur1.py:784-787, gshift_denoise1.py:828-831).  src:[T][C][H][W] of `src_dtype`, noise:[T][1][H][W]
 * or NULL, dst:[T][H][W][8] bf16 (channels C(+1)..7 zeroed). */
int sn_ingest(const void* src, int src_dtype, const void* noise, void* dst, int T, int C, int H, int W, void* stream);

/* One dense nn.Conv2d (+ what the reference applies around it), as an implicit GEMM on MFMA. */
typedef struct sn_conv_desc {
    const void* in[3];   /* 1..3 NHWC inputs of equal shape, concatenated along channels (torch.cat(...,1)):
                            rconcat gshift_deblur1.py:772, conv_hr0 :640 */
    int n_in;
    int cs_in;           /* storage channels of each input */
    int T, h_in, w_in;   /* spatial size the convolution sees */
    int in_mode;         /* 0: as is; 1: inputs are [T][h_in/2][w_in/2] and are bilinearly upsampled x2,
                            align_corners=False, while staging (SkipUpSample.up[0], gshift_deblur1.py:344) */
    int k, stride, pad;  /* k in {1,2,3,5}; Conv2d zero padding */
    int h_out, w_out;
    const void* wfrag;   /* [MT][KS][64][8] bf16 */
    int mt, ks;
    const float* bias;   /* [16*mt] natural channel order, zero padded; NULL = no bias */
    int act;             /* 0 none, 1 PReLU with the single shared slope `prelu` (nn.PReLU(), :551,576) */
    float prelu;
    const void* res;     /* NHWC [T][h_out][w_out][cs_out] added after the activation, or NULL
                            ("x = self.up(x); x = x + y" :348-349, "+ self.skip_conv(shortcut)" gshift_deblur2.py:611) */
    void* out;
    int cs_out;
    int out_mode;        /* 0: NHWC; 1: F.pixel_shuffle(.,2) store -> [T][2h][2w][cs_out] (PixelShufflePack :277) -- the weight ROWS (and bias) of such
                            a conv are ordered [sub-pixel 2 i + j][output channel c < cs_out] (reference row 4 c + 2 i + j; zero rows for the storage
                            padding), cs_out = 4 mt, so lane group g of the accumulator layout holds every channel of sub-pixel g (ABI 16; prep.pack_conv);
                            2: NCHW [T][c_out][h][w] of `nchw_dtype` plus the NCHW shortcut `sc`
                               ("return output_features + shortcut[...]" :791) */
    int c_out;           /* logical out channels (mode 2 only) */
    int nchw_dtype;      /* SN_F32 with a half-precision module = the restored frame straight from the fp32 accumulators: what the CLIs'
                            metrics and PNG writer consume (inference/test_deblur.py:137-143 calls .float() on the module output) */
    const void* sc;      /* mode 2: NCHW tensor of `sc_dtype`, same shape as out */
    int sc_dtype;
    float* pool;         /* NULL or [T][gridDim.y*gridDim.x][16*mt] f32 per-workgroup channel sums of the output
                            (first half of AdaptiveAvgPool2d(1), CALayer :69); rows per frame = sn_conv_pool_blocks(d) */
    const float* oscale; /* NULL or [T][oscale_stride] f32: out = conv * oscale[t][c] (+ res) -- the CALayer scale of a CAB
                            applied in the epilogue of its second conv ("res = self.CA(res); res += x", :155-157) */
    int oscale_stride;
    const void* res2;    /* NULL or a second NHWC residual of the same shape as `res`, added after it: the "+ shortcut" that
                            follows the last TFR_UNet of a stage (gshift_deblur1.py:769,779) rides on that UNet's last conv */
    int flags;           /* SN_CONV_TILE_KERNEL: run single-input 3x3 stride-1 convs on the one-workgroup-per-tile kernel instead of the
                            persistent streaming kernel (csrc/sn_conv3p.hip) -- A/B measurements; results are bit-identical.
                            Bits 4..7: persistent workgroups per CU of the streaming kernel, 0 = the library's choice; bit 8: the streaming kernel also
                            where the library prefers the tile kernel; bit 9: its residual operand through registers instead of LDS; bits 10..11:
                            prefetch depth code (1 / 2: three / four tiles ahead at 16 channels; 3: the streaming fused CAB with two region buffers);
                            bits 12..14: MEASUREMENTS ONLY, WRONG RESULTS -- the streaming conv without its DMA (1), B reads / MFMAs (2), stores (4);
                            on conv2 of sn_cab_fused(rows = 0) bit 12 means "both weight sets in LDS" (results unchanged); bit 15: stride-2 convs on
                            4 x 16 tiles whatever their width (measurements; results unchanged).  Which instance a descriptor runs on, with these
                            bits and without: sn_conv2d_route (below) */
    int clip_n, clip_T, clip_lo; /* per-clip frame remap (ABI 19; all 0 = off): output frame j reads frame (j / clip_n) * clip_T + clip_lo + j % clip_n
                            of every in[] -- the kept frames [clip_lo, clip_lo + clip_n) of each clip of a batch, read in place (rconcat of
                            Engine.forward_clips).  out, res, res2, pool and oscale stay indexed by j.  T % clip_n == 0, clip_lo + clip_n <= clip_T.
                            Implemented by the generic MFMA kernel (n_in > 1, or any conv the specialised 3x3 / streaming kernels do not take);
                            on any other route, and in sn_cab_stats / sn_cab_fused, nonzero fields are SN_EINVAL */
} sn_conv_desc;
#define SN_CONV_TILE_KERNEL 1
int sn_conv2d(const sn_conv_desc* d, void* stream);   /* d is a HOST pointer, read during the call */
/* number of workgroups per frame sn_conv2d launches for this descriptor (= rows of `pool` per frame); host only */
int sn_conv_pool_blocks(const sn_conv_desc* d);
/* The kernel instance sn_conv2d (lines_len = 0) or sn_cab_stats(d, lines_len) (lines_len > 0) launches for d, or SN_EINVAL where that entry point
 * refuses d (ABI 20).  Both entry points launch exactly what this returns.  Host only: the pointers are tested for NULL, never read.
 * ncu: compute units the streaming kernel plans for; 0 = the current device (none: the tile kernel, as the entry points do), < 0 = no device.
 * plan: NULL, or int[8] that receives the streaming kernel's work plan {ntx, nty, S, nseg, nsg, qs, grid, pool_rows} (streaming routes only):
 * tile columns / rows of 8 x 32 pixels, tiles per segment of a column (the last one shorter when S does not divide nty), segments per column,
 * segments in all, segments per workgroup, workgroups launched (a multiple of 8; the last ones may be idle), pool rows per frame.
 * The route does not depend on ncu, on the plan bits 4..7 or on the measurement bits 12..14 of flags.
 * SN_CONV_ROUTE(kernel, mt, a, d, mode, rl) names one template instance: */
#define SN_CONV_K_GENERIC 1   /* conv_mfma_kernel<MT = mt, TH = a, TW = 4 a>: a = 8 (8 x 32 tiles) or 4 (4 x 16: stride 2 over more than 24 input channels,
                               * or bit 15 of flags); d = mode = rl = 0 */
#define SN_CONV_K_FAST    2   /* conv3_fast_kernel<MT = mt, CS = a, 8>: (mt, a) in {(1, 16), (2, 24), (3, 40), (3, 48), (4, 64), (5, 80)} */
#define SN_CONV_K_STATS   3   /* conv3_fast_kernel<MT = mt, CS = a, 8, STATS>: sn_cab_stats on the tile kernel, (mt, a) in {(1, 16), (2, 24)} */
#define SN_CONV_K_STREAM  4   /* conv3p_kernel<MT = mt, CS = a, 8, D = d, MODE = mode, RL = rl> (csrc/sn_conv3p.hip): (mt, a) in {(1, 16), (2, 24),
                               * (3, 40), (3, 48), (4, 64)}, mode 0 bias, 1 PReLU + pool, 2 oscale + res, 3 sn_cab_stats; d: tiles of prefetch */
#define SN_CONV_ROUTE(kernel, mt, a, d, mode, rl) (((kernel) << 24) | ((mt) << 20) | ((a) << 12) | ((d) << 8) | ((mode) << 4) | (rl))
int sn_conv2d_route(const sn_conv_desc* d, int lines_len, int ncu, int* plan);

/* SkipUpSample's tail (gshift_deblur1.py:341-350: x = up(x); x = x + y with up = bilinear x2 -> 1x1 conv).  The 1x1 is linear and the interpolation
 * weights sum to one, so conv(up(x)) = up(conv(x)): the caller runs the 1x1 at LOW resolution with sn_conv2d (in_mode 0) and this pass computes
 *   out[T][2 hs][2 ws][cs] = bilinear_x2(lo[T][hs][ws][cs]) + res[T][2 hs][2 ws][cs]      (bf16 NHWC, fp32 arithmetic, cs a multiple of 8;
 * nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False)).  sn_conv2d's in_mode 1 (interpolation in the conv's loader) stays available. */
int sn_upsample2_add(const void* lo, const void* res, void* out, int T, int hs, int ws, int cs, void* stream);

/* CALayer / CALayer2 squeeze-excite: mean -> 1x1 -> ReLU -> 1x1 -> sigmoid (gshift_deblur1.py:61-70,84-87).
 * partial:[T][nblk][cpad] f32 sums, wa:[cr][c], wb:[c][cr] f32, ca:[T][cpad] f32 out (pad entries 0).
 * bad: NULL, or one u32 that is set to 1 when a channel sum is not finite -- the range guard of the half-precision intermediates of the
 * producer (an overflowed fp16 value upstream turns its channel sum into inf / NaN); the caller zeroes it and reads it back when it likes. */
int sn_ca_mlp(const float* partial, int nblk, int cpad, int c, int cr, float inv_hw,
              const float* wa, const float* wb, float* ca, int T, unsigned* bad, void* stream);

/* CALayer of a CAB computed BEFORE its second conv runs: the pooled mean of res = conv2(mid) is linear in mid,
 *   sum_p res[co](p) = sum_ci sum_tap W2[co][ci][tap] * S_tap[ci],   S_tap = sum of mid over the pixels the tap can reach
 *   (total - excluded border row / column + corner), so it follows from the channel sums of mid (partial, from conv1's
 * epilogue) and the first/last rows and columns of mid.  Then the usual 1x1 -> ReLU -> 1x1 -> sigmoid (:61-70).
 * mid:[T][h][w][cs] bf16, w2:[cin=c][9][cpad] f32 (bias-free 3x3, zero beyond c), ca:[T][cpad] out.  Lets sn_conv2d apply the scale and the
 * residual in conv2's epilogue (no separate pass over res).
 * scratch: sn_cab_ca_scratch_floats(T) floats of workspace (partial sums of the split reduction). */
int sn_cab_ca_scratch_floats(int T);
int sn_cab_ca(const float* partial, int nblk, int cpad, const void* mid, int cs, int c, int cr, int h, int w,
              const float* w2, const float* wa, const float* wb, float* scratch, float* ca, int T, void* stream);
/* ---- fused dense CAB (csrc/sn_cabf.hip): CAB.forward, gshift_deblur1.py:141-156, in three tensor passes instead of five ----
 *   res = body(x) = conv3x3(PReLU(conv3x3(x)));  res = CA(res);  res += x
 * The two-launch form (sn_conv2d with `pool`, sn_cab_ca, sn_conv2d with oscale / res) writes `mid` = PReLU(conv1(x)) to memory and reads it
 * back.  The fused form never stores it:
 *   1. sn_cab_stats(conv1, lines_len): conv1 exactly as sn_conv2d would run it -- same tiles, same per-workgroup channel sums into conv1->pool --
 *      but conv1->out is the LINE buffer [T][4][lines_len][cs] bf16 (lines_len >= max(h, w)): row 0, row h-1, column 0, column w-1 of mid;
 *   2. sn_cab_ca_lines: sn_cab_ca reading those lines instead of the tensor;
 *   3. sn_cab_fused(conv1, conv2, tile_rows): per (tile_rows x 32)-pixel tile conv1 + PReLU on the tile's 1-pixel ring into LDS, conv2 from there,
 *      * conv2->oscale, + x (conv2->res must be conv1->in[0]), + conv2->res2, stored to conv2->out.  tile_rows: 8 or 16 = one workgroup per
 *      tile (csrc/sn_cabf.hip); 0 = the STREAMING form (csrc/sn_conv3p.hip: cabp_kernel -- persistent workgroups, a loader wave that moves the next
 *      (8 + 4) x 36 pixel regions HBM -> LDS with LDS-DMA, four compute waves: conv1 on the ring -> mid in LDS -> conv2 -> scale + x -> store;
 *      no res2; its statistics pass is sn_cab_stats on a descriptor WITHOUT SN_CONV_TILE_KERNEL, i.e. the streaming conv's own pool rows).
 *      The streaming form also needs conv1->act == 1 with 0 <= conv1->prelu <= 1 (its PReLU is max(v, a v)): for any other slope
 *      tile_rows = 0 returns SN_EINVAL -- after the caller has already run passes 1 and 2 -- while the tile forms (8 / 16) take every slope.
 * Both descriptors are those of the two-launch form (3x3, stride 1, pad 1, one input, cs_in == cs_out, NHWC); conv1->pool / conv1->out are only
 * read by sn_cab_stats.  Results are bit-identical to the two-launch form.  sn_cab_fused_supported: 1 when an instance for the pair's GEOMETRY
 * exists (16- and 24-channel storage), else 0 -- the caller then uses the two-launch form.  It does not look at the slope: a caller of the
 * streaming form checks 0 <= conv1->prelu <= 1 itself before pass 1 (shiftnet_amd/engine.py: Engine._cab_fused). */
int sn_cab_fused_supported(const sn_conv_desc* conv1, const sn_conv_desc* conv2);
int sn_cab_stats(const sn_conv_desc* conv1, int lines_len, void* stream);
int sn_cab_ca_lines(const float* partial, int nblk, int cpad, const void* lines, int lines_len, int cs, int c, int cr, int h, int w,
                    const float* w2, const float* wa, const float* wb, float* scratch, float* ca, int T, void* stream);
int sn_cab_fused(const sn_conv_desc* conv1, const sn_conv_desc* conv2, int tile_rows, void* stream);

/* the same for the fp32 engine: mid [T][h][w][c] float32 (pixel stride c), partial = sn32_chan_sum(mid), w2 [c][9][cpad] f32: the CAB's scale and
 * residual then ride on the second sn32_conv2d (oscale / res) instead of a pass of their own (sn32_scale_residual). */
int sn32_cab_ca(const float* partial, int nblk, int cpad, const float* mid, int c, int cr, int h, int w,
                const float* w2, const float* wa, const float* wb, float* scratch, float* ca, int T, void* stream);

/* ---- grouped spatial-temporal shift unit: channel_shift -> CAB2 -> CAB1 (gshift_deblur1.py:504-547) ---- */
typedef struct sn_unit_src {
    const void* x;       /* [T][h][w][C] the unit's input */
    int T, h, w, C;      /* C in {64, 80} */
    int mode;            /* 0: CAB1 (no shift, u = x[t]); 1: CAB2 of a forward unit; 2: CAB2 of a reverse unit */
    int wrap;            /* 0: boundary frame kept (gshift_deblur1.py:513,517); 1: circular temporal roll (gshift_deblur2.py:504-505);
                            2: x is a frame range of a temporally split window and the neighbour of its boundary frame (frame -1 for a
                            forward unit, T for a reverse unit) belongs to the adjacent rank: only the half the unit borrows exists
                            here, in `halo` */
    const void* halo;    /* wrap == 2, mode 1 / 2: the neighbour frame's borrowed half-channels, CONTIGUOUS [h][w][C/2] (same element type
                            as x): forward units the upper half of the previous rank's last frame, reverse units the lower half of the
                            next rank's first frame -- the receive buffer of the halo exchange itself, no copy into a strided slot */
    int t0, nt;          /* frames [t0, t0 + nt) of x are processed (nt == 0: all T).  Outputs, pool rows and the neighbour rule are indexed
                            by the absolute frame, so a unit can be launched in pieces: the frames that need no halo while the exchange is
                            in flight, the boundary frame after it */
    int clip;            /* frames per clip (ABI 19): x holds T / clip independent clips end to end and the neighbour rule applies inside each --
                            a forward unit's first frame of a clip is kept (wrap 0) or borrows from the last frame of the SAME clip (wrap 1), a
                            reverse unit mirrors it.  0 (or T): one clip.  T % clip != 0, or clip > 0 with wrap 2, is SN_EINVAL.  t0 / nt stay
                            absolute frame indices */
} sn_unit_src;

/* validation op: materialise u = cat(y, spatial_shift2(hw)) : [T][h][w][3C/2] exactly as channel_shift returns it
 * (gshift_deblur1.py:504-528).  offs: int8 [C/2][2] (dy,dx) of the source pixel.  Pure index work: bit exact. */
int sn_gsts_gather(const sn_unit_src* s, const int8_t* offs, void* u, void* stream);

/* y = channel_shift(x) of Shift_CAB (gshift_denoise1.py:167-179): the temporal half-channel roll alone, materialised
 * (the 24-/80-channel Shift_CAB encoders feed a dense 3x3 CAB, which reads y as an ordinary tensor).
 * C any even channel count whose halves are whole elements; mode 1 forward / 2 reverse. */
int sn_temporal_roll(const sn_unit_src* s, void* y, void* stream);

/* hw = CAB2.conv1(spatial_shift2(borrowed half)) (gshift_deblur1.py:470-503,223,251): depthwise 3x3 of the
 * zero-padded displaced neighbour-frame channels, never materialising the shifted tensor.
 * w1:[C/2][9] u32 words: the bf16 weight in the LOW half, high half zero (operand of v_dot2c_f32_bf16). */
int sn_gsts_shiftconv(const sn_unit_src* s, const int8_t* offs, const uint32_t* w1, void* hw, void* stream);
/* The same operator on the matrix cores (round 6), same operands: per channel and 16 x 16 output tile the depthwise 3x3 is the banded GEMM
 *   out[n][m] = sum_{ty, j} A[m][(ty, j)] * W[n + ty + 8 + dy_k][j + 8 + dx_k],   A[m][(ty, j)] = w[ty][j - m] for 0 <= j - m <= 2,
 * over a CHANNEL-PLANAR 34 x 34 LDS window (the loader transposes; hw and x stay NHWC): three 16-byte LDS reads + three MFMAs per channel and tile
 * instead of 9 two-byte reads + 9 v_dot2c per pixel and channel; the A fragments are built in registers from the nine weights (one v_perm_b32 per
 * word).  Every displacement in offs must be a multiple of 4 pixels (spec.shift_table: they are).  Same products, another accumulation order:
 * within rounding of sn_gsts_shiftconv, not bit-identical to it. */
int sn_gsts_shiftconv_mfma(const sn_unit_src* s, const int8_t* offs, const uint32_t* w1, void* hw, void* stream);
/* The kernel has two forms with bit-identical results: SN_K0_TILE, one 34 x 34 window per 16 x 16 tile (persistent workgroups walk an XCD's tile
 * list), and SN_K0_WALK, a workgroup takes a segment of S vertically adjacent tiles and keeps the window as a ring of 34 rows (16 new rows per
 * tile after a segment's first).  sn_gsts_shiftconv_mfma_plan tells which one a launch of s takes on a device with ncu compute units (host only,
 * nothing is launched, no device access; the launch calls the same function with the device's own count): plan[SN_K0_PLAN_LEN] =
 *   {form, S, nseg, wgs, per_x, per_tile, ntx, nty, nt, grid}
 * form: SN_K0_TILE / SN_K0_WALK; S, nseg: segment length in tiles and segments per tile column (tile form: the candidate that was too short to
 * walk); wgs: workgroups per XCD (grid = 8 wgs); per_x: rows of the item list per XCD -- (frame, segment) rows for the walking form, (frame, tile
 * row) rows for the tile form, XCD k owns rows [k per_x, (k + 1) per_x) and a workgroup takes every wgs-th (row, tile column) item of them;
 * per_tile: the tile form with one workgroup per tile; ntx, nty: tiles per row / column; nt: frames.  SN_EINVAL: what the launch refuses, ncu < 8.
 * sn_gsts_shiftconv_mfma_opt: the same launch with the form named (tests and measurements; results do not depend on it).  form 0: the plan's;
 * seg: segment length 1..8 of SN_K0_WALK (clipped to nty), 0: the plan's; wgs: workgroups per XCD, clipped to the XCD's items, 0: the plan's.
 * Anything else -- a seg without form SN_K0_WALK included -- is SN_EINVAL and launches nothing.  opt == NULL: sn_gsts_shiftconv_mfma.
 * sn_gsts_shiftconv_mfma_plan_opt: the plan of that launch (opt == NULL: sn_gsts_shiftconv_mfma_plan).
 * (Three new symbols and one new struct, no existing struct or signature changes: SN_ABI_VERSION stays 20.) */
#define SN_K0_TILE 1
#define SN_K0_WALK 2
#define SN_K0_PLAN_LEN 10
typedef struct sn_k0_opts {
    int form;
    int seg;
    int wgs;
} sn_k0_opts;
int sn_gsts_shiftconv_mfma_plan(const sn_unit_src* s, int ncu, int* plan);
int sn_gsts_shiftconv_mfma_plan_opt(const sn_unit_src* s, int ncu, const sn_k0_opts* opt, int* plan);
int sn_gsts_shiftconv_mfma_opt(const sn_unit_src* s, const int8_t* offs, const uint32_t* w1, void* hw, const sn_k0_opts* opt, void* stream);

/* g1 = SimpleGate(RepConv2(body[0](norm(cat(shortcut, hw))))): LayerNorm2d over 3C/2 (CAB2) or C (CAB1) channels (eps 1e-6,
 * affine folded into the 1x1 weights), the 1x1 conv to 2C on MFMA, depthwise 3x3 + identity and the gate, with the 2C-channel
 * intermediate kept in LDS (gshift_deblur1.py:19-28,190-198,225-233).  wfrag / bias: prep.pack_ln_gemm (gate-paired rows).
 * hw may be NULL for mode 0.
 * wdw: [9][C] u32: word k of a tap row holds the fp16 weights of positions (2k, 2k+1) of a's storage order (v_pk_fma_f16
 * operand, prep.pk_f16_words of the [9][2C] table with the identity folded into the centre tap).
 * g1_blocked = 0: g1 natural NHWC [T][h][w][C] (sn_grp5_gemm_gate);
 * g1_blocked = 2 (C = 64 only): channel-planar [T][h][C][sn_planar_pitch(w)], zeros in the pad columns (sn_dw5m_gemm_gate).
 * pool: NULL or [T][sn_lngate_blocks][C].  T, h or w below 1 is SN_EINVAL like every other bad operand: nothing is launched. */
int sn_ln_gemm_gate(const sn_unit_src* s, const void* hw, const void* wfrag, const float* bias, const uint32_t* wdw,
                    void* g1, float* pool, int g1_blocked, void* stream);
int sn_lngate_blocks(int h, int w);

/* "+" variants: RepConv with groups = C/8 (gshift_deblur1.py:157-165) as a block-diagonal MFMA GEMM, then body[4]
 * (1x1 C->2C), SimpleGate2 and the channel sums.  g1:[T][h][w][C] natural NHWC, wgrp: prep.pack_grouped_frag
 * [C/16][13][64][8] bf16 (3x3 and identity folded), C = 80.  pool: [T][sn_grp5_blocks][C]. */
int sn_grp5_gemm_gate(const void* g1, const float* ca_in, const void* wgrp, const void* wfrag, void* g2, float* pool,
                      int T, int h, int w, int C, void* stream);
int sn_grp5_blocks(int h, int w);

/* ---- matrix-core stencils (csrc/sn_gsts3.hip) ------------------------------------------------------------------
 * A depthwise k x k conv is a GEMM over the x axis: 16 outputs x 32 input columns of ONE channel per MFMA (banded
 * Toeplitz A operand), N = 16 places of that channel.  Its input is channel-planar: [T][h][C][wr] bf16,
 * wr = sn_planar_pitch(w) (w rounded up to 8), columns >= w are ZERO. */
int sn_planar_pitch(int w);
int sn_nhwc_to_planar(const void* x, void* xp, int T, int h, int w, int C, void* stream);   /* x:[T][h][w][C] -> xp planar */

/* g2 = SimpleGate2(body[4](RepConv(g1))) for the depthwise variants (gshift_deblur2.py:159-168,182-185,201): 5x5 + 3x3 +
 * identity folded into one 5x5 and run as Toeplitz MFMAs on the channel-planar g1p, the 1x1 C -> 2C on MFMA, x1 * sigmoid(x2),
 * per-workgroup channel sums for the CALayer2 that follows.  ca_in: NULL or [T][C] f32 scale applied first (denoise).  C = 64.
 * ttab: bf16 [C][5][2][20] padded bands (prep.pack_toeplitz), wfrag: body 1x1 fragments, gate-paired rows, natural K.
 * pool: [T][sn_dw5m_blocks(h,w)][C] partial sums of g2. */
int sn_dw5m_blocks(int h, int w);
int sn_dw5m_gemm_gate(const void* g1p, const float* ca_in, const void* ttab, const void* wfrag, void* g2, float* pool,
                      int T, int h, int w, int C, void* stream);

/* ---- the two phases of a GSTS unit's blocks (sn_gsts_cab2_phase1 / phase2, sn_cab1_phase1 / phase2) --------------------
 * The global average pool of CALayer2 (gshift_deblur1.py:76-87) is the one grid-wide dependency inside CAB2 / CAB1, so a block is two
 * passes over the frame: phase 1 up to g2 and its channel sums, [sn_ca_mlp on the sums], phase 2 from g2 to the block's output.
 *
 * PHASE 1, fused, every variant (csrc/sn_phase1r.hip):
 *   g2 = SimpleGate2(body[4](RepConv(SimpleGate(RepConv2(body[0](norm(u)))))))   (gshift_deblur1.py:183-211 CAB1, :212-255 CAB2; gshift_deblur2.py:186-258)
 * in ONE kernel: u is read once, g2 written once; `a`, g1 and r never reach HBM.  (The denoisers, whose inner CALayer2 needs the global pool of g1,
 * run it twice: sn_phase1_opts.  sn_ln_gemm_gate + sn_dw5m_gemm_gate / sn_grp5_gemm_gate above are the same phase 1 in two kernels with g1 in bf16 in HBM:
 * the engine's fallback for a checkpoint whose activations leave the fp16 range of `a`, g1 and r inside the fused kernel.)
 * The fused kernel RELIES ON UN-FLUSHED fp16 SUBNORMALS in every fp16 stage (v_cvt_pk_f16_f32 of `a`, the packed fp16 FMAs of RepConv2, the gate product,
 * the A / B operands of the fp16 MFMAs): the gate's rescaling symmetry (tests/gauge.py) lets a checkpoint hold body[0] rows 2^k times smaller against a
 * second 1x1 4^k times larger -- the same network -- and g1 = a1 a2 2^-4 is then 4^k of what the synthetic checkpoint gives.  No source sets a denormal
 * mode; the compiler's default for gfx950 keeps them.  Measured on MI355X (tests/test_gpu_phase1_gauge.py): down to k = -6, where 98 % of g1 is below 2^-14, every
 * g2 element stays inside a float64 interval that assumes gradual underflow and the error against the exact function stays within 10 % of the base
 * gauge's; a kernel that flushed would lose one decimal digit at k = -4 and everything at k = -6.  At k = -7 wfrag2 (body[4] times 16) passes 65504:
 * Plan.add_naf notices at pack time and the engine starts the module on the two-kernel chain, whose second 1x1 is bf16.
 * sn_gsts_cab2_phase1: s->mode 1 / 2, hw = sn_gsts_shiftconv's output; sn_cab1_phase1: s->mode 0.  C = 64 or 80, RepConv depthwise or grouped 8 -> 8 ON THE
 * MATRIX CORES; weights prep.pack_phase1r --
 *     wfrag1  bf16 [C/8][KS1][64][8]: body[0] with the LayerNorm scale folded, wave-paired rows (M-tiles 2q, 2q+1 = channels 16q.. and their gate
 *             partners), the folded bias as bf16 hi + lo in the columns of k-slots K, K+1 (the kernel feeds the normalised input and a constant 1);
 *     w3      uint32 [C/16][4][9][4] packed-fp16 taps of RepConv2 (+identity) per (wave, lane group, tap, packed register);
 *     wgrp    fp16 [C/16][2][8][64][8]: RepConv (5x5 + 3x3 + identity) of every group as an x-pair Toeplitz GEMM (row = output channel + 8 * pixel of a
 *             pair; k = kernel row, input column 0..5 relative to the pair, input channel);
 *     wfrag2  fp16 [C/8][KS2][64][8]: body[4], wave-paired rows, sigmoid rows times -log2 e.
 * g2: [T][h][w][C] NHWC bf16.  pool: NULL or [T][sn_phase1_pool_blocks(T,h,w)][C] f32 partial channel sums of g2 (CALayer2, finished by sn_ca_mlp or by
 * the sn_se_fold tail): one row per (column strip, block of 8 image rows) -- a property of the image, not of the launch, so the sums and every
 * reduction over them are bit-identical whatever frame range (s->t0, s->nt), team size or device the launch runs with. */
typedef struct sn_phase1_weights {
    const void* wfrag1;
    const uint32_t* w3;
    const void* wgrp;
    const void* wfrag2;
} sn_phase1_weights;
/* Optional fold of CALayer2's squeeze-excite MLP (gshift_deblur1.py:76-87) into phase 1: the LAST workgroup of a frame to finish reduces
 * the frame's partial sums in a fixed order (bit-reproducible whichever workgroup that is) and writes ca[t][C] = sigmoid(wb relu(wa mean)),
 * so no sn_ca_mlp launch sits between the phases.  wa:[cr][c], wb:[c][cr] f32 (conv_du.0 / conv_du.2), c == C.
 * ticket: [>= T] u32 counters, ZERO before the first use; every launch leaves them zero again.  NULL: partial sums only. */
typedef struct sn_se_fold {
    const float* wa;
    const float* wb;
    int c, cr;
    unsigned* ticket;
    float* ca;
    unsigned* bad;       /* NULL, or the range guard of sn_ca_mlp: set to 1 when a channel sum of the frame is not finite */
} sn_se_fold;
/* The denoisers' inner CALayer2 on g1 = SimpleGate(...) (gshift_denoise1.py:224,257; gshift_denoise2.py:194,227).  Its global average
 * pool sits INSIDE phase 1, so phase 1 runs twice over the input and g1 still never reaches HBM:
 *   pass 1, g1_sums = 1: LayerNorm -> 1x1 -> dw3x3 -> gate only; pool receives the partial channel sums of g1 (finish them with sn_ca_mlp, or pass
 *           the inner CALayer2's weights as `se`: se->ca is then that layer's scale); g2 is not touched (may be NULL);
 *   pass 2, g1_scale = that scale [T][C] f32: the whole phase 1 with g1 multiplied by it before the RepConv.
 *   g1_store (optional, both passes): a scratch buffer of the size sn_phase1_g1_store_bytes gives for (T, h, w, C).  Pass 1 then also writes every g1 row it
 *           computes (fp16, unscaled, in the kernel's own strip / ring order: opaque), and pass 2 reads those rows back, scales them and runs only the
 *           RepConv -> 1x1 -> gate half: the stagers' LayerNorm and the first 1x1 + 3x3 run once per block instead of twice.  Bit-identical to the
 *           two passes without a store.  Both passes must see the same buffer, frame range and geometry.
 * NULL / zeros: the deblur models (no inner CALayer2).
 * team: 0 = the library chooses how many workgroups walk consecutive frames of the same rows in lock step (1, 2, 4 or 8: csrc/sn_phase1r.hip,
 * P1RPlan); a fixed value is for measurements only.  Results do not depend on it beyond the summation order of the pool rows. */
typedef struct sn_phase1_opts {
    const float* g1_scale;
    int g1_sums;
    int team;
    void* g1_store;
} sn_phase1_opts;
int sn_phase1_pool_blocks(int T, int h, int w);
int sn_phase1_g1_store_bytes(int T, int h, int w, int C, long long* bytes);
int sn_gsts_cab2_phase1(const sn_unit_src* s, const void* hw, const sn_phase1_weights* wt, void* g2, float* pool, const sn_se_fold* se,
                        const sn_phase1_opts* opt, void* stream);
int sn_cab1_phase1(const sn_unit_src* s, const sn_phase1_weights* wt, void* g2, float* pool, const sn_se_fold* se, const sn_phase1_opts* opt, void* stream);
/* The work decomposition of a phase-1 launch over nfr frames of h x w on a device with ncu compute units (host only, no device access): out7 =
 * {strips, slack / strip, slack remainder, team size F, frame blocks, rows per team chunk, teams}; sn_p1r_strip_begin: first own column of strip s
 * (s == strips: w).  Exposed for the host-logic tests and for tools that size measurements; the launch uses exactly this plan. */
int sn_p1r_plan(int nfr, int h, int w, int ncu, int team, int* out7);
int sn_p1r_strip_begin(const int* plan7, int s, int w);

/* PHASE 2, all variants (C = 64 / 80): y = shortcut + beta * body[7](ca * g2) (gshift_deblur1.py:201,210,254): beta and the optional bias
 * are folded into wfrag / bias; the shortcut is the ROLLED tensor for CAB2 (s->mode 1 / 2: sn_gsts_cab2_phase2) and x itself for CAB1
 * (s->mode 0: sn_cab1_phase2).  ca: [T][C] f32 from sn_ca_mlp. */
int sn_gsts_cab2_phase2(const sn_unit_src* s, const void* g2, const float* ca, const void* wfrag, const float* bias, void* y, void* stream);
int sn_cab1_phase2(const sn_unit_src* s, const void* g2, const float* ca, const void* wfrag, const float* bias, void* y, void* stream);

/* sn_gsts_cab2_phase2 of a unit's CAB2 and sn_cab1_phase1 of its CAB1 in ONE launch (csrc/sn_phase1r.hip, the FK4 instance): the stager waves of
 * phase 1 form y = shortcut + W3' . (ca * g2_in) + bias' for the rows they stage -- the operations of phase 2 in its order, y is bit-identical --
 * store it once (the CAB1's phase 2 reads it as its shortcut) and feed the LayerNorm from the values they just rounded; g2 / pool / se as
 * sn_cab1_phase1, also bit-identical.  s is the CAB2's source (mode 1 / 2), g2_in / ca / wfrag / bias / y the operands of sn_gsts_cab2_phase2, wt
 * the CAB1's phase-1 weights; opt: NULL or the team size only.  g2_in, y, g2 and s->x are four distinct tensors.
 * sn_cab2_phase2_cab1_phase1_supported: 1 where the fused launch exists -- C = 64, the whole tensor (nt = 0), wrap 0 / 1, one clip -- else 0, and the
 * entry point returns SN_EINVAL (never a wrong result): the caller keeps the two launches. */
int sn_cab2_phase2_cab1_phase1_supported(const sn_unit_src* s);
int sn_cab2_phase2_cab1_phase1(const sn_unit_src* s, const void* g2_in, const float* ca, const void* wfrag, const float* bias, void* y,
                               const sn_phase1_weights* wt, void* g2, float* pool, const sn_se_fold* se, const sn_phase1_opts* opt, void* stream);


/* ---- fp32-storage path (csrc/sn_f32.hip) -----------------------------------------------------------------------
 * The arithmetic type upstream runs the "+" denoiser in (inference/test_denoise.py:83-85: the .half() is commented out)
 * and the validation build of the engine: activations fp32 NHWC [T][H][W][C] with an explicit pixel stride `cs`
 * (elements) so that channel slices of a wider tensor can be read / written in place, weights = the checkpoint's fp32
 * values re-ordered to [k][k][cin/groups][cout].  Direct fp32 FMA kernels (no MFMA): correctness first. */
typedef struct sn32_conv_desc {
    const float* in[3];  /* 1..3 inputs concatenated along channels (groups == 1), pre-offset to their first channel */
    int c_in[3];         /* logical channels taken from each input */
    int cs_in[3];        /* pixel stride of each input, elements */
    int n_in;
    int T, h_in, w_in;   /* spatial size the convolution sees */
    int in_mode;         /* 0 as is; 1 inputs are [T][h_in/2][w_in/2] upsampled x2 bilinearly while reading (gshift_deblur1.py:344) */
    int k, stride, pad, groups;   /* nn.Conv2d(.., groups): 1, C/8 (RepConv "+", :160-161) or C (depthwise) */
    int h_out, w_out, c_out;
    const float* w;      /* [k][k][cin_total/groups][c_out] */
    const float* bias;   /* [c_out] or NULL */
    int act; float prelu;                      /* as sn_conv_desc */
    const float* oscale; int oscale_stride;    /* NULL or [T][oscale_stride] (stride 0: one row for all frames): out = (conv+bias) * oscale (+ res) */
    const float* res; int cs_res;              /* NULL or NHWC tensor added last */
    void* out; int cs_out;
    int out_mode;        /* 0 NHWC fp32; 1 pixel_shuffle(2) NHWC fp32; 2 NCHW of nchw_dtype + shortcut sc (as sn_conv_desc) */
    int nchw_dtype; const void* sc;
    const void* wsplit;  /* NULL: exact fp32 products (v_mfma_f32_16x16x4_f32).  Else the weights as bf16 hi / lo A fragments
                          * (prep.pack_conv32_split): every product is wh xh + wh xl + wl xh on the bf16 matrix cores with fp32 accumulation
                          * (~2^-16 relative per product), taken for single-input stride-1 dense k = 1 / 3 and grouped-by-8 k = 3 / 5 convs */
    const float* iscale; int iscale_stride;   /* NULL or [T][iscale_stride] f32: the input is multiplied by iscale[t][ci] while it is loaded (the
                          * CALayer scale of the producer, gshift_deblur1.py:69-70, without a pass of its own); single-input dense / grouped-by-8 convs */
    const float* rscale; int rscale_stride;   /* NULL or [T][rscale_stride] f32: res is multiplied by rscale[t][co] before it is added (RepConv of the
                          * denoisers: conv(g1 ca1) + g1 ca1 with iscale = rscale = ca1, gshift_denoise1.py RepConv after CALayer2); grouped-by-8 convs */
    const float* ln_w; const float* ln_b;     /* NULL or [cin]: LayerNorm2d (gshift_deblur1.py:19-28, eps 1e-6) over the cin channels of every input pixel while
                          * it is loaded; the split-precision 1x1 path only (wsplit, k 1, cin <= 128, h_out w_out >= 64), SN_EINVAL otherwise */
    float* csum; int csum_cpad;               /* NULL or [T][sn32_conv_csum_tiles(h_out, w_out)][csum_cpad] f32: channel sums of the stored output per workgroup
                          * (AdaptiveAvgPool2d(1) of the CALayer behind a conv, finished by sn_ca_mlp / sn32_cab_ca); split-precision dense 3x3 only */
    int clip_n, clip_T, clip_lo;              /* per-clip frame remap of the inputs as in sn_conv_desc (ABI 19; all 0 = off): the split dense tiles
                          * (SN32_K_SPLIT) and the exact kernels (SN32_K_EXACT) without iscale / rscale / ln_w / csum; SN_EINVAL on any other route */
} sn32_conv_desc;
int sn32_conv_csum_tiles(int h_out, int w_out);
int sn32_conv2d(const sn32_conv_desc* d, void* stream);
/* The kernel instance sn32_conv2d launches for d (host only, no device access: the pointers' alignment takes part, nothing is read), or SN_EINVAL
 * where sn32_conv2d refuses d.  sn32_conv2d launches exactly what this returns.  SN32_ROUTE(kernel, a, b), a / b its template arguments: */
#define SN32_K_1X1      1    /* conv32s_1x1_kernel<NCB = a, LOAD = b>: split 1x1 over the flat pixel list; a = ceil(cin / 32) in 1..4,
                              * b 0 plain (iscale), 1 LayerNorm on load, 2 bilinear x2 on load (in_mode 1) */
#define SN32_K_SPLIT    2    /* conv32s_kernel<MTC = a, KSZ = b, dense>: split tiles, a in {1, 3, 4}, b in {1, 3} */
#define SN32_K_SPLIT_G8 3    /* conv32s_kernel<MTC = a, KSZ = b, grouped by 8>: split tiles, a in {3, 4}, b in {3, 5} */
#define SN32_K_EXACT    4    /* conv32m_kernel<MTC = a, TH = b, TW = 4 b>: exact fp32 MFMA, (a, b) in {(1, 8), (3, 8), (5, 8)} stride 1, {(2, 4), (5, 4)} stride 2 */
#define SN32_K_DW       5    /* dw32_kernel: depthwise, four channels per thread (a = b = 0) */
#define SN32_K_DIRECT   6    /* conv32_kernel<NCO = a>: direct fp32 FMA, a in {1, 4} (b = 0) */
#define SN32_ROUTE(kernel, a, b) (((kernel) << 16) | ((a) << 8) | (b))
int sn32_conv2d_route(const sn32_conv_desc* d);
/* channel_shift (gshift_deblur1.py:504-528) materialised in fp32: offs != NULL: u [T][h][w][3C/2] = cat(roll(x), shift(borrowed));
 * offs == NULL: the temporal roll alone, [T][h][w][C] (Shift_CAB, gshift_denoise1.py:167-179).  s->x is a float tensor.
 * u2: NULL, or (offs != NULL) a second [T][h][w][3C/2] tensor whose first C channels receive roll(x) too (CAB2's LayerNorm input is built in it). */
int sn32_gsts_gather(const sn_unit_src* s, const int8_t* offs, float* u, float* u2, void* stream);
/* channel_shift (gshift_deblur1.py:504-528) written where CAB2 consumes it: vin:[T][h][w][3C/2] receives roll(x) in its first C channels
 * (LayerNorm input and shortcut -- one copy, not the two of sn32_gsts_gather), and
 *   w == NULL, u != NULL: u:[T][h][w][C/2] = shift(borrowed half) for a separate conv1 (sn32_conv2d depthwise into vin[:, C:]);
 *   w != NULL, u == NULL: conv1 (depthwise 3x3, no bias, :206-212; w:[9][C/2] tap-major) is applied here, vin[:, C:] = conv1(shift(borrowed))
 *                         (bit-identical, slower: scattered 4-byte taps).
 * C % 8 == 0.  Frame range as sn32_gsts_gather. */
int sn32_gsts_shiftconv(const sn_unit_src* s, const int8_t* offs, const float* w, float* vin, float* u, void* stream);
/* LayerNorm2d (gshift_deblur1.py:19-28,44-53) over K channels per pixel. */
int sn32_layernorm(const float* x, int cs_x, int K, const float* w, const float* b, float* out, int cs_out, long long npix, void* stream);
/* SimpleGate (mode 0, :175-178) / SimpleGate2 (mode 1, :179-182): a:[npix][2C] -> out:[npix][C]. */
int sn32_gate(const float* a, int C, int mode, float* out, long long npix, void* stream);
/* SimpleGate / SimpleGate2 plus the channel sums of the result in one pass (the CALayer2 after it): out:[T][hw][C], partial as
 * sn32_chan_sum would compute from out. */
int sn32_gate_sum(const float* a, int C, int cpad, int mode, float* out, int T, int hw, int nblk, float* partial, void* stream);
/* The second 1x1 of phase 1 (C -> 2C, no bias) + SimpleGate2 (gshift_deblur1.py:179-182, x1 * sigmoid(x2)) + the channel sums of the result for
 * CALayer2, split-precision arithmetic (wsplit as in sn32_conv_desc): x:[T][hw][cs_x >= cin], out:[T][hw][C], partial:[T][hw / 64][cpad]
 * (finished by sn_ca_mlp with nblk = hw / 64).  hw % 64 == 0, C % 16 == 0, cin % 4 == 0, cin <= 128. */
int sn32_conv1x1_gate2(const float* x, int cs_x, int cin, const void* wsplit, int C, int cpad, float* out, int T, int hw, float* partial, void* stream);
/* RepConv2 (depthwise 3x3 + identity, gshift_deblur1.py:143-157) and SimpleGate (:175-178) in one pass: a:[T][h][w][cs_a >= 2C] f32,
 * w:[9][2C] (the depthwise weight, tap-major), out:[T][h][w][C] = a'[c] * a'[C + c]; partial NULL, or [T][nblk][cpad] channel sums of out
 * (what sn32_gate_sum returns) for the CALayer2 of the denoisers.  Bit-identical to sn32_conv2d(depthwise, res = a) + sn32_gate. */
int sn32_dw_gate(const float* a, int cs_a, const float* w, int C, int cpad, float* out, int T, int h, int wd, int nblk, float* partial, void* stream);
/* AdaptiveAvgPool2d(1) first half: partial:[T][nblk][cpad] sums (cpad >= C, <= 256), finished by sn_ca_mlp. */
int sn32_chan_sum(const float* x, int cs, int C, int cpad, int T, int hw, int nblk, float* partial, void* stream);
/* out = r * ca[t][c] (+ x if x != NULL). */
int sn32_scale_residual(const float* r, const float* x, const float* ca, int ca_stride, float* out, int T, int hw, int C, void* stream);
/* NCHW (src_dtype) [+ noise map] -> NHWC fp32 [T][H][W][C(+1)]. */
int sn32_ingest(const void* src, int src_dtype, const void* noise, float* dst, int T, int C, int H, int W, void* stream);


/* ---- I/O edges of the CLIs (csrc/sn_io.hip) ---------------------------------------------------------------------
 * numpy2tensor + .to(device) + .half() (inference/test_deblur.py:191-200,128,134) with the uint8 frames crossing PCIe:
 * src:[T][H][W][3] u8 (device) -> dst:[T][3][H][W] of dst_dtype, value = round(float(v) * (1/255)). */
int sn_ingest_u8(const uint8_t* src, void* dst, int dst_dtype, int T, int H, int W, void* stream);
/* clamp(0,1) * 255 of the network output (test_deblur.py:140-141): img:[T][H][W][3] u8 rounded to nearest even (what
 * cv2.imwrite stores, :152) or NULL; gt:[T][H][W][3] u8 or NULL; sse:[T][sn_egress_blocks()] f32 partial sums of the
 * squared error of the UNROUNDED value vs gt (skimage PSNR, data_range 255, :142). */
int sn_egress_blocks(void);
int sn_egress_u8(const void* out, int out_dtype, const uint8_t* gt, uint8_t* img, float* sse, int T, int H, int W, void* stream);
/* The CLIs' own SSIM (inference/test_deblur.py:25-49: Gaussian statistics, sd 1.5, over the (C,H,W) volume of clamp(out,0,1) and
 * gt / 255, scipy 'reflect' boundaries on all three axes): scratch:[T][15][H][W] f32 workspace, partial:[T][sn_ssim_blocks()]
 * f32 sums of the SSIM map; SSIM of frame t = sum(partial[t]) / (3 H W).
 * Arithmetic: scipy's and numpy's, rounding for rounding -- the five statistics a, b, a a, b b, a b in float32; the filter one axis after the
 * other in scipy's order C, H, W, each a float64 sum of float64 taps rounded once to float32 (scratch holds the planes after C and H); the map
 * in float32 with every operation rounded on its own (no FMA); the map summed in float64 per workgroup and rounded once into partial.  Only the
 * order of the sums inside float64 and of the final mean differs from the CLI's ssim_calculate: within 2e-5 of it on any content, near-flat
 * frames far from mid-grey included (measured: 2e-7).  Every word of partial is written; nothing outside scratch and partial is. */
int sn_ssim_blocks(void);
int sn_ssim_u8(const void* out, int out_dtype, const uint8_t* gt, float* scratch, float* partial, int T, int H, int W, void* stream);

/* ---- Y'CbCr edges of the video restorer (csrc/sn_yuv.hip, csrc/sn_yuv_stats.hip) -----------------------------------------
 * Added without an ABI bump: SN_ABI_VERSION stays 20, because these are new symbols and a new struct; no existing struct,
 * signature or operand encoding changes, so a caller built against the earlier header keeps working.
 *
 * A frame payload is Y4M's: the Y plane [H][W], then the U and the V plane, each [H][W] (4:4:4) or [ceil(H/2)][ceil(W/2)] (4:2:0);
 * one byte per sample at 8 bit, one 16-bit little-endian word with the value in the low 10 bits at 10 bit.  T payloads lie end to end.
 *
 * Constants (each a float64 expression rounded ONCE to float32).  Kr, Kb = 0.299, 0.114 (BT.601) or 0.2126, 0.0722 (BT.709),
 * Kg = (1 - Kr) - Kb; s = 2^(bits - 8); limited range: yo = 16 s, ys = 219 s, cs = 224 s, legal codes Y 16 s..235 s, C 16 s..240 s;
 * full range: yo = 0, ys = cs = 2^bits - 1, legal codes 0..2^bits - 1; co = 128 s in both.
 *   ky = 1 / ys, crv = 2 (1 - Kr) / cs, cbu = 2 (1 - Kb) / cs, cgu = -2 Kb (1 - Kb) / Kg / cs, cgv = -2 Kr (1 - Kr) / Kg / cs,
 *   cu = 1 / (2 (1 - Kb)), cv = 1 / (2 (1 - Kr)).
 *
 * sn_ingest_yuv, per pixel, every product and sum rounded separately to float32 (no FMA):
 *   yd = float(Y - yo); ud = float(Un - D co) / D, vd = float(Vn - D co) / D with Un / D the upsampled chroma code (below; exact);
 *   yy = ky * yd;  R = yy + crv * vd;  G = (yy + cgu * ud) + cgv * vd;  B = yy + cbu * ud;  each clamped to [0,1] and then rounded
 *   to dst_dtype (nearest even).  dst:[T][3][Hp][Wp]; pixel (y, x) with y >= H or x >= W is pixel (min(y, H-1), min(x, W-1)).
 *   Chroma upsampling, bilinear on the integer codes, (j, i) = (y >> 1, x >> 1), neighbours clamped to the chroma plane:
 *     4:2:0 centre-sited (D = 16): jn = j + 1 for odd y, j - 1 for even y, in likewise from x:
 *                                  Un = 3 (3 C[j][i] + C[jn][i]) + (3 C[j][in] + C[jn][in])                 (weights 9/3/3/1)
 *     4:2:0 left-sited   (D = 8):  v(c) = 3 C[j][c] + C[jn][c];  even x: Un = 2 v(i);  odd x: Un = v(i) + v(i + 1)
 *     4:4:4              (D = 1):  Un = C[y][x].
 *
 * sn_egress_yuv, out:[T][3][Hp][Wp] of out_dtype, the H x W top-left crop is written:
 *   R, G, B clamped to [0,1];  Y' = (Kr R + Kg G) + Kb B;  Cb = (B - Y') * cu;  Cr = (R - Y') * cv   (float32, no FMA);
 *   4:2:0 chroma of block (j, i), pixel coordinates clamped to the H x W frame:
 *     centre-sited: 0.25 * ((c[2j][2i] + c[2j][2i+1]) + (c[2j+1][2i] + c[2j+1][2i+1]))
 *     left-sited:   h(y) = (c[y][2i-1] + 2 c[y][2i]) + c[y][2i+1];  0.125 * (h(2j) + h(2j+1))
 *   code = clamp(rint(yo + ys * Y'), legal Y codes), clamp(rint(co + cs * C), legal C codes), rint = nearest even.
 *   Only the T payloads are written.  10-bit payloads must be 2-byte aligned. */
#define SN_YUV_444 0
#define SN_YUV_420_CENTER 1     /* Y4M C420jpeg */
#define SN_YUV_420_LEFT 2       /* Y4M C420mpeg2, C420 (and C420paldv, whose vertical siting is not modelled) */
#define SN_YUV_BT601 0
#define SN_YUV_BT709 1
#define SN_YUV_LIMITED 0
#define SN_YUV_FULL 1
typedef struct sn_yuv_fmt {
    int bits;      /* 8 | 10 */
    int chroma;    /* SN_YUV_444 | SN_YUV_420_CENTER | SN_YUV_420_LEFT */
    int matrix;    /* SN_YUV_BT601 | SN_YUV_BT709 */
    int range;     /* SN_YUV_LIMITED | SN_YUV_FULL */
} sn_yuv_fmt;
int sn_ingest_yuv(const uint8_t* src, const sn_yuv_fmt* fmt, void* dst, int dst_dtype, int T, int H, int W, int Hp, int Wp, void* stream);
int sn_egress_yuv(const void* out, int out_dtype, const sn_yuv_fmt* fmt, uint8_t* dst, int T, int H, int W, int Hp, int Wp, void* stream);

/* sn_yuv_thumb (added like the two above: a new symbol, SN_ABI_VERSION stays 20): luma thumbnails for the scene-cut detector of the video
 * restorer (shiftnet_amd/scenes.py).  src: T payloads as sn_ingest_yuv takes them (frame_bytes(fmt, H, W) apart, luma plane first); only the
 * luma plane is read, fmt->matrix and fmt->range are not looked at.  dst:[T][ceil(H/8)][ceil(W/8)] uint16,
 *   dst[t][by][bx] = sum of the luma codes Y[y][x] of frame t over 8 by <= y < min(8 by + 8, H), 8 bx <= x < min(8 bx + 8, W):
 * the integer sum of the 8 x 8 block; pixels outside H x W contribute nothing (edge blocks are partial sums, not replicated).
 * 64 x 1023 = 65 472 fits uint16.  Integer arithmetic, no atomics: exact, and the same for every launch geometry.  Only dst is written.
 * SN_EINVAL before anything is launched: null pointers, bits not 8 / 10, unknown chroma code, T, H or W < 1, dst at an odd address, src at
 * an odd address at 10 bit. */
int sn_yuv_thumb(const uint8_t* src, const sn_yuv_fmt* fmt, uint16_t* dst, int T, int H, int W, void* stream);

/* sn_yuv_noise_hist (a new symbol, SN_ABI_VERSION stays 20): histograms for the blind noise estimate of the video restorer
 * (shiftnet_amd/noise.py).  src: T payloads as sn_yuv_thumb takes them; only the luma plane is read and of fmt only bits decides anything.
 * For every non-overlapping 2 x 2 block i < H/2, j < W/2 (integer division: a last odd row or column belongs to no block) with
 *   a = Y[2i][2j], b = Y[2i][2j+1], c = Y[2i+1][2j], d = Y[2i+1][2j+1]:
 * the block counts iff all four codes lie strictly between lo and hi, and then adds one to bin v = |a - b - c + d| (twice the Haar HH
 * coefficient, 0 <= v <= 2 (2^bits - 1)).  dst:[T][NB] uint32 with NB = 2 (2^bits - 1) + 1 (511 at 8 bit, 2047 at 10 bit) is OVERWRITTEN
 * with the counts, never added to; nothing outside these T NB words is written.  Integer sums: exact, and the same for every launch
 * geometry and schedule.  H < 2 or W < 2 is legal and gives all-zero histograms.
 * SN_EINVAL before anything is launched: null pointers, bits not 8 / 10, unknown chroma code, T, H or W < 1, lo > hi, dst not 4-byte
 * aligned, src at an odd address at 10 bit. */
int sn_yuv_noise_hist(const uint8_t* src, const sn_yuv_fmt* fmt, uint32_t* dst, int lo, int hi, int T, int H, int W, void* stream);

/* ---- the active picture of a letterboxed / pillarboxed stream (new symbols and one new struct, SN_ABI_VERSION stays 20) ------------------
 * A picture rectangle is (x0, y0, w, h) in luma samples of the H x W stream: 0 <= x0, 1 <= w, x0 + w <= W, and the same for y.  At 4:2:0
 * x0 and y0 are even, w is even unless x0 + w == W and h is even unless y0 + h == H, so that no chroma sample is shared between the inside
 * and the outside; at 4:4:4 any integers are legal.  "The cropped stream" is the video whose planes are the rectangle cut out of every plane:
 * luma rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1; 4:2:0 chroma rows y0/2 .. y0/2 + ceil(h/2) - 1, columns x0/2 .. x0/2 + ceil(w/2) - 1.
 * The three _rect entry points launch the kernels of the entry points above with the rectangle's origin and the stream's row pitches (H, W
 * give the pitches and frame_bytes, payload to payload); SN_EINVAL as theirs, and for a null or illegal rectangle.
 *
 * sn_ingest_yuv_rect: dst:[T][3][Hp][Wp], Hp >= rect.h, Wp >= rect.w, is bit for bit what sn_ingest_yuv writes for the cropped stream (H = rect.h,
 *   W = rect.w): the chroma neighbours clamp to the rectangle's chroma planes, never to the stream's -- no bar sample reaches the picture --
 *   and the padding repeats the rectangle's last row and column.
 * sn_egress_yuv_rect: out:[T][3][Hp][Wp]; the samples of the rectangle, luma and chroma, of the T payloads of the STREAM's size at dst are written
 *   with what sn_egress_yuv writes for the cropped stream (the 4:2:0 filters clamp to the rect.h x rect.w crop of out), and nothing else is.
 * sn_yuv_noise_hist_rect: the histograms of sn_yuv_noise_hist over the rectangle's luma, the 2 x 2 block grid anchored at (x0, y0): block
 *   (i, j), i < rect.h / 2, j < rect.w / 2, is Y[y0 + 2i .. y0 + 2i + 1][x0 + 2j .. x0 + 2j + 1].
 * The wide loads and stores test the address itself: a rectangle with x0 % 16 == 0 in a stream with W % 16 == 0 keeps them, any other takes the
 * element-wise path with the same arithmetic. */
typedef struct sn_yuv_rect { int x0, y0, w, h; } sn_yuv_rect;
int sn_ingest_yuv_rect(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, void* dst, int dst_dtype, int T, int H, int W, int Hp, int Wp,
                       void* stream);
int sn_egress_yuv_rect(const void* out, int out_dtype, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, uint8_t* dst, int T, int H, int W, int Hp, int Wp,
                       void* stream);
int sn_yuv_noise_hist_rect(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect, uint32_t* dst, int lo, int hi, int T, int H, int W,
                           void* stream);

/* sn_yuv_rowcol_sums: what the letterbox rule of the video restorer (shiftnet_amd/picture.py) looks at.  src: T payloads as sn_yuv_thumb takes
 * them; only the luma plane is read and of fmt only bits decides anything.
 *   rows[t][y] = sum over x < W of Y[y][x],  cols[t][x] = sum over y < H of Y[y][x]      (uint32 [T][H] and [T][W])
 * exact integer sums (65535 x 1023 < 2^32).  Both arrays are OVERWRITTEN, never added to, and nothing else is written.  Integer atomics: the
 * result is the same for every launch geometry and schedule.
 * SN_EINVAL before anything is launched: null pointers, bits not 8 / 10, unknown chroma code, T, H or W < 1, H or W > 65535, rows or cols not
 * 4-byte aligned, src at an odd address at 10 bit. */
int sn_yuv_rowcol_sums(const uint8_t* src, const sn_yuv_fmt* fmt, uint32_t* rows, uint32_t* cols, int T, int H, int W, void* stream);

/* ---- dithered egress (a new symbol and one new struct, SN_ABI_VERSION stays 20) ------------------------------------------------------------
 * sn_egress_yuv_dither is sn_egress_yuv (rect == NULL: the whole frame) or sn_egress_yuv_rect (rect != NULL) with one change in the last line
 * of sn_egress_yuv above.  With mode SN_DITHER_TPDF the code of a sample is
 *   clamp(rint((off + scale * v) + d), legal codes)        (off, scale) = (yo, ys) for Y, (co, cs) for C; every float32 sum rounded separately
 * where d is triangular noise of +-1 code (mean 0, variance 1/6), an integer hash of where the sample is:
 *   f = dither->t0 + t                       the frame number: t counts the payloads of the launch
 *   p = 0 (Y), 1 (Cb), 2 (Cr)
 *   (y, x) = the sample's row and column in ITS plane (at 4:2:0 the chroma planes count chroma samples), counted from the picture's first
 *            sample: the rectangle's origin with rect, so that the rectangle still holds what the cropped stream's egress writes
 *   k = (y * 0x9E3779B1) ^ (x * 0x85EBCA77) ^ (f * 0xC2B2AE3D) ^ (p * 0x27D4EB2F) ^ seed                  (uint32, products wrap)
 *   k ^= k >> 16;  k *= 0x85EBCA6B;  k ^= k >> 13;  k *= 0xC2B2AE35;  k ^= k >> 16
 *   d = float((k & 0xFFF) + ((k >> 12) & 0xFFF) - 4095) / 4096                                            (exact in float32, |d| < 1)
 * (tests/dither_ref.py restates it in numpy; the kernel equals it bit for bit.)  A launch of T payloads at t0 therefore equals launches of its
 * parts at their own t0.  With mode SN_DITHER_NONE the launch, the kernel instantiation and the bytes are those of the entry points without
 * _dither, which launch the instantiations without a dither as before.  The per-thread layout is theirs: 8 x 2 pixels, wide stores where the
 * address allows, the element-wise path elsewhere; both paths dither.
 * SN_EINVAL before anything is launched: as sn_egress_yuv / sn_egress_yuv_rect (an illegal rectangle included), and a null dither, a mode
 * that is neither of the two, or t0 < 0. */
#define SN_DITHER_NONE 0
#define SN_DITHER_TPDF 1
typedef struct sn_yuv_dither { int mode; uint32_t seed; int t0; } sn_yuv_dither;
int sn_egress_yuv_dither(const void* out, int out_dtype, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */,
                         const sn_yuv_dither* dither, uint8_t* dst, int T, int H, int W, int Hp, int Wp, void* stream);

/* ---- restoration amount and the view of what was removed (a new symbol and one new struct, SN_ABI_VERSION stays 20) ----------------------------
 * sn_egress_yuv_mix is sn_egress_yuv_dither (dither == NULL is legal here and means no dither; rect == NULL: the whole frame) that also reads the code
 * every sample had on the way in.  in: T payloads of the same fmt, H and W as dst; the sample of `in` that belongs to a sample of dst sits at the same
 * byte offset -- with a rectangle it is the STREAM's sample, not the crop's.  Everything up to the value
 *   v = off + scale * value                  (off, scale) = (yo, ys) for Y, (co, cs) for C
 * is sn_egress_yuv_dither's, unchanged: the clamp of R, G, B, Y', Cb, Cr, the 4:2:0 filters, their clamping to the crop with rect, every float32
 * operation rounded separately (no FMA).  Then, with e = float(code_in), a = mix->ay for Y and mix->ac for Cb and Cr, d the dither of that sample as
 * sn_egress_yuv_dither defines it (0 without one), lo..hi the plane's legal codes, every float32 product, sum and difference rounded separately:
 *   SN_MIX_AMOUNT   a == 0.0f:  code = code_in, whatever the dither is
 *                   otherwise:  m = e + a * (v - e);  code = clamp(rint(m + d), min(lo, code_in), max(hi, code_in))
 *                   The result never leaves the legal range unless the input sample already had; amount 0 is the identity on illegal codes too.
 *                   Amount 1 is e + (v - e) in float32, which may differ from v in the last bit: callers who want sn_egress_yuv's bytes call it.
 *   SN_MIX_REMOVED  m = co + a * (e - v);  code = clamp(rint(m + d), lo, hi)      co = 128 s for all three planes: input minus result around mid-grey,
 *                   a the gain
 * The blend is linear in the code domain: not perceptual, and at 4:2:0 not a blend of the R'G'B' pictures.  (tests/mix_ref.py restates it in numpy; the
 * kernel equals it bit for bit.)  The per-thread layout is sn_egress_yuv's: 8 x 2 pixels; `in` is read with one 8 / 16 B load (chroma at 4:2:0:
 * 4 / 8 B) where dst is stored wide and the address of `in` allows it, element-wise elsewhere; both paths use the same arithmetic.  Only the samples
 * sn_egress_yuv_dither writes are written.  The entry points without _mix launch the instantiations they launched before.
 * SN_EINVAL before anything is launched: everything sn_egress_yuv_dither refuses except a null dither; a null mix or in; a mode that is neither of the
 * two; ay or ac that is not finite, or outside [0, 1] in SN_MIX_AMOUNT; in at an odd address at 10 bit; byte ranges [in, in + T frame_bytes) and
 * [dst, dst + T frame_bytes) that overlap. */
#define SN_MIX_AMOUNT  0
#define SN_MIX_REMOVED 1
typedef struct sn_yuv_mix { int mode; float ay, ac; } sn_yuv_mix;   /* AMOUNT: the amounts of Y and of Cb/Cr; REMOVED: the gains */
int sn_egress_yuv_mix(const void* out, int out_dtype, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */,
                      const sn_yuv_dither* dither /* NULL: none */, const sn_yuv_mix* mix, const uint8_t* in, uint8_t* dst,
                      int T, int H, int W, int Hp, int Wp, void* stream);

/* ---- a noise-level function for the denoisers (new symbols, SN_ABI_VERSION stays 20) -----------------------------------------------------------
 * The curve: the sigma of the noise as a function of the luma code, SN_NLF_BANDS = 16 knots; knot b sits at luma code lo + (b + 0.5) (hi - lo) / 16
 * (shiftnet_amd/noise.py estimates it on the host from the histograms of the first entry point; the second turns it into the network's noise plane).
 *
 * sn_yuv_noise_hist_bands: the statistic of sn_yuv_noise_hist split by brightness.  src, fmt, lo, hi, T, H, W as sn_yuv_noise_hist_rect; rect == NULL is
 * the whole frame, otherwise the block grid is anchored at the rectangle's origin (the cropped stream's histograms).  For every non-overlapping 2 x 2 luma
 * block (a, b / c, d) whose four codes lie strictly between lo and hi, with S = a + b + c + d:
 *   band = (16 (S - 4 lo)) / (4 (hi - lo))      integer division; 4 <= S - 4 lo <= 4 (hi - lo) - 4, so 0 <= band <= 15
 *   v    = min(|a - b - c + d|, NBV - 1)         NBV = 128 at 8 bit, 512 at 10 bit: the last bin means "at least NBV - 1"
 * and one is added to dst[t][band][v].  dst:[T][16][NBV] uint32 is OVERWRITTEN with the counts, never added to; nothing else is written.  Integer
 * arithmetic: exact, and the same for every launch geometry and schedule.  Summed over the bands, bins < NBV - 1 are those of sn_yuv_noise_hist and the
 * last bin is the sum of its bins from NBV - 1 up.  A picture without a whole block is legal and gives zeros.
 * SN_EINVAL before anything is launched: as sn_yuv_noise_hist_rect (rect may be NULL here), and lo < -2^24 or hi > 2^24 (the band is 32-bit arithmetic).
 *
 * sn_noise_map_level: dst:[T][1][Hp][Wp] of dst_dtype, Hp >= h, Wp >= w, with h x w the picture (rect, or H x W for rect == NULL; all coordinates below
 * count from the picture's first sample and nothing outside the picture is read).  knots: 16 finite float32 in HOST memory, read before the call returns:
 * the curve already divided by 255.  lo < hi.  Every float32 product, sum, difference and quotient below is rounded separately (no FMA):
 *   block means   M[j][i] = float(sum of the luma codes of block (j, i)) / float(count), block (j, i) = rows 8j .. min(8j + 8, h) - 1, columns
 *                 8i .. min(8i + 8, w) - 1: partial blocks at the far edges divide by their own count; nby = ceil(h / 8), nbx = ceil(w / 8)
 *   pixel (y, x): ye = min(y, h - 1), xe = min(x, w - 1)      (the padding replicates the edge pixel, as sn_ingest_yuv pads)
 *                 nx = 2 xe - 7;  i0 = floor(nx / 16);  ax = float(nx - 16 i0) * 0.0625      ((xe - 3.5) / 8 = i0 + ax: the block centres lie at 8 i + 3.5; exact)
 *                 ny, j0, ay likewise from ye;  i1 = i0 + 1, j1 = j0 + 1;  all four indices clamped to 0 .. nbx - 1 / 0 .. nby - 1 after that
 *                 top = M[j0][i0] + ax * (M[j0][i1] - M[j0][i0]);  bot = M[j1][i0] + ax * (M[j1][i1] - M[j1][i0]);  m = top + ay * (bot - top)
 *                 u = min(max((m - float(lo)) * s - 0.5, 0), 15)   with s = 16 / (hi - lo), a float64 expression rounded ONCE to float32
 *                 i = min(int(floor(u)), 14);  f = u - float(i);  value = k[i] + f * (k[i + 1] - k[i])
 *   and value is rounded to dst_dtype (nearest even).  A flat curve therefore gives exactly k[0] at every pixel.  (tests/nlf_ref.py restates both entry
 * points in numpy; the kernels equal it bit for bit.)  Only dst is written.
 * SN_EINVAL before anything is launched: null pointers, bits not 8 / 10, unknown chroma code or dtype, T, H or W < 1, an illegal rectangle, Hp or Wp
 * smaller than the picture, lo >= hi, lo < -2^24 or hi > 2^24, a knot that is not finite, src at an odd address at 10 bit. */
#define SN_NLF_BANDS 16
int sn_yuv_noise_hist_bands(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */, uint32_t* dst, int lo, int hi,
                            int T, int H, int W, void* stream);
int sn_noise_map_level(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */, const float* knots, int lo, int hi,
                       void* dst, int dst_dtype, int T, int H, int W, int Hp, int Wp, void* stream);

/* ---- the noise statistics of frame pairs (new symbols, SN_ABI_VERSION stays 20) -----------------------------------------------------------------
 * The temporal noise estimate of the video restorer (shiftnet_amd/noise.py): texture that does not move is the same in the next frame and noise is
 * not, so the Haar HH coefficient of the DIFFERENCE of two consecutive frames keeps the noise and drops the picture.  src, fmt, rect (NULL: the
 * whole frame), lo, hi, H, W exactly as sn_yuv_noise_hist_rect / sn_yuv_noise_hist_bands take them: only the luma plane is read, of fmt only bits
 * decides anything, the 2 x 2 block grid is anchored at the rectangle's origin, a last odd row or column belongs to no block.  T >= 2 payloads are
 * T - 1 pairs; pair p is payloads p and p + 1.  For block (i, j) with the codes a0 b0 / c0 d0 in payload p and a1 b1 / c1 d1 in payload p + 1:
 * the block counts iff all EIGHT codes lie strictly between lo and hi, and then
 *   v = |(a1 - b1 - c1 + d1) - (a0 - b0 - c0 + d0)|          0 <= v <= 4 (2^bits - 1)
 * sn_yuv_noise_hist_pairs: one is added to dst[p][v]; dst:[T - 1][NBP] uint32, NBP = 4 (2^bits - 1) + 1 (1021 at 8 bit, 4093 at 10 bit).
 * sn_yuv_noise_hist_pairs_bands: one is added to dst[p][band][min(v, NBV - 1)]; dst:[T - 1][16][NBV] uint32 with the NBV of sn_yuv_noise_hist_bands and
 *   band = (2 (S - 8 lo)) / (hi - lo)      unsigned integer division, S the sum of the eight codes; 8 <= S - 8 lo <= 8 (hi - lo) - 8, so 0 <= band <= 15
 * Both: dst is OVERWRITTEN with the counts, never added to; nothing outside those words is written.  Integer sums: exact, and the same for every launch
 * geometry and schedule.  A picture without a whole block (h < 2 or w < 2) is legal and gives zeros.
 * SN_EINVAL before anything is launched: everything sn_yuv_noise_hist_bands refuses (an illegal rectangle and lo < -2^24 or hi > 2^24 included, for both
 * entry points), and T < 2 (T - 1 > 65535 is refused with T > 65535). */
int sn_yuv_noise_hist_pairs(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */, uint32_t* dst, int lo, int hi,
                            int T, int H, int W, void* stream);
int sn_yuv_noise_hist_pairs_bands(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */, uint32_t* dst, int lo, int hi,
                                  int T, int H, int W, void* stream);

/* ---- block motion of frame pairs and the pair statistics along it (new symbols, SN_ABI_VERSION stays 20) ------------------------------------------
 * The motion-compensated temporal noise estimate of the video restorer (shiftnet_amd/noise.py): the pair statistics above compare a 2 x 2 block with
 * the block at the same place in the next payload, so content that moves reads as noise.  sn_yuv_block_motion finds one integer translation per
 * 16 x 16 luma block of every pair and the two _mv entry points take the second payload's block where it points.  src, fmt, rect (NULL: the whole
 * frame), lo, hi, T >= 2, H, W and stream exactly as sn_yuv_noise_hist_pairs takes them: only the luma plane is read, of fmt only bits decides
 * anything, samples are taken as stored (a 16-bit word may hold up to 65535), pair p is payloads p and p + 1.  The picture is h x w, the rectangle
 * or the frame; every grid is anchored at its first sample and all coordinates below count from there.
 *   hb = h / 2, wb = w / 2: the whole 2 x 2 blocks (i, j).  Block (i, j) is a MATCHING block if i + j is even and a MEASURING block if it is odd.
 *   Vector block (I, J) holds the 2 x 2 blocks with i / 8 == I and j / 8 == J: 16 x 16 samples, fewer at the right and lower edge.
 *   nby = ceil(hb / 8), nbx = ceil(wb / 8).  hb == 0 or wb == 0: no vector block; sn_yuv_block_motion writes nothing and the histograms are zero.
 *   Candidates: (dy, dx) with |dy| <= 7 and |dx| <= 7, 225 in all.  A candidate is ADMISSIBLE for a vector block iff the block's sample extent --
 *   rows 16 I .. 2 min(8 I + 8, hb) - 1, columns 16 J .. 2 min(8 J + 8, wb) - 1 -- displaced by it lies inside the h x w picture.  Nothing is
 *   clamped and nothing outside the picture is ever read.  (0, 0) is always admissible.
 *   SAD(dy, dx) = the sum of |Y_p(y, x) - Y_{p+1}(y + dy, x + dx)| over the four samples of every matching block of the vector block (at most
 *   128 x 65535: exact in 32 bits).  The vector is the admissible candidate with the smallest SAD; among equal SADs the one with the smallest
 *   (|dy| + |dx|, dy, dx) in lexicographic order.
 * sn_yuv_block_motion: mv:[T - 1][nby][nbx][2] int8 holds (dy, dx), sad:[T - 1][nby][nbx] uint32 the winning SAD.  Both are overwritten; nothing outside
 *   them is written.
 * sn_yuv_noise_hist_pairs_mv, sn_yuv_noise_hist_pairs_bands_mv: dst, v, S, band, NBP and NBV exactly as sn_yuv_noise_hist_pairs and
 *   sn_yuv_noise_hist_pairs_bands define them, except that only measuring blocks count, that the four codes a1 b1 / c1 d1 of payload p + 1 are those
 *   at rows 2 i + dy, 2 i + dy + 1 and columns 2 j + dx, 2 j + dx + 1 with (dy, dx) = mv[p][i / 8][j / 8], and that a block whose displaced position
 *   does not lie wholly inside the picture does not count.  mv is device memory the entry point cannot validate: the test is made per block in the
 *   kernel, ANY int8 contents are memory-safe, and with the vectors of sn_yuv_block_motion it never fails.  The eight codes must lie strictly between
 *   lo and hi, as there; where hi admits stored words above 2^bits - 1, v is saturated to NBP - 1 (the flat histogram) as it is to NBV - 1.  dst is
 *   OVERWRITTEN; integer sums, exact and the same for every launch geometry and schedule.
 * (tests/motion_ref.py restates all three in numpy; the kernels equal it word for word.)
 * SN_EINVAL before anything is launched: everything sn_yuv_noise_hist_pairs_bands refuses (sn_yuv_block_motion takes no lo / hi / dst), a null mv or
 * sad, sad or dst not 4-byte aligned, and a picture of more than 65535 x 16 rows for sn_yuv_block_motion (nby is a grid dimension). */
int sn_yuv_block_motion(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */, int8_t* mv, uint32_t* sad,
                        int T, int H, int W, void* stream);
int sn_yuv_noise_hist_pairs_mv(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */, const int8_t* mv, uint32_t* dst,
                               int lo, int hi, int T, int H, int W, void* stream);
int sn_yuv_noise_hist_pairs_bands_mv(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */, const int8_t* mv,
                                     uint32_t* dst, int lo, int hi, int T, int H, int W, void* stream);

/* ---- method noise: the statistics of what a run changed (a new symbol, SN_ABI_VERSION stays 20) ---------------------------------------------------
 * The report of the video restorer (shiftnet_amd/report.py): if only noise left the picture, input minus output is white in space, independent from
 * frame to frame, no stronger on edges than on flat areas, and as strong as the noise was.  sn_yuv_diff_stats makes the integer sums those four
 * measures are computed from on the host.  a (what came in) and b (what was written): T payloads each, of fmt and H x W, laid out as
 * sn_egress_yuv_mix takes `in` and `dst`; rect == NULL is the whole frame, otherwise the h x w picture of every payload (the rules of
 * sn_ingest_yuv_rect say which rectangles are legal).  Samples are taken as stored, not masked to the legal codes (a 10-bit payload's words may hold
 * anything up to 65535).  On the picture's h x w luma samples d(y, x) = b_Y(y, x) - a_Y(y, x); on its chroma planes -- ceil(h / 2) x ceil(w / 2) at
 * 4:2:0, h x w at 4:4:4 -- du and dv likewise.  A pixel is an EDGE pixel iff e(y, x) >= edge with
 *   e(y, x) = |b_Y(y, min(x + 1, w - 1)) - b_Y(y, x)| + |b_Y(min(y + 1, h - 1), x) - b_Y(y, x)|
 * (the written picture, which is the clean one, classifies).  dst[t] holds SN_DIFF_STATS = 16 signed 64-bit integers:
 *   0, 1, 2     N = h w, sum d, sum d^2
 *   3, 4        Nx = h (w - 1), sum d(y, x) d(y, x + 1) over x < w - 1
 *   5, 6        Ny = (h - 1) w, sum d(y, x) d(y + 1, x) over y < h - 1
 *   7           sum d_t(y, x) d_{t+1}(y, x) with payload t + 1 of the same launch; 0 for the launch's last payload
 *   8, 9        Ne = the number of edge pixels, sum d^2 over them
 *   10          Nc = the samples of one chroma plane
 *   11, 12      sum du, sum du^2
 *   13, 14      sum dv, sum dv^2
 *   15          0
 * dst:[T][16] int64 is OVERWRITTEN, never added to; nothing outside those words is written.  Integer sums accumulated in 64 bit (one product reaches
 * 65535^2): exact, and the same for every launch geometry and schedule.  a == b is legal and gives zeros beside the counts.
 * (tests/diff_stats_ref.py restates it in numpy; the kernel equals it word for word.)
 * SN_EINVAL before anything is launched: a null a, b, dst or fmt; bits not 8 / 10 or an unknown chroma code; a or b at an odd address at 10 bit; dst
 * not 8-byte aligned; an illegal rectangle; edge < 0; T outside 1 .. 65535; H or W < 1. */
#define SN_DIFF_STATS 16
int sn_yuv_diff_stats(const uint8_t* a, const uint8_t* b, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */,
                      int edge, int64_t* dst /* [T][SN_DIFF_STATS] */, int T, int H, int W, void* stream);

/* ---- method noise along block motion vectors (a new symbol, SN_ABI_VERSION stays 20) ---------------------------------------------------------------
 * Word 7 of sn_yuv_diff_stats compares a payload's difference with the next payload's AT THE SAME PLACE: removed detail that moves with the picture
 * reads as uncorrelated, which is what a noise-only removal reads.  sn_yuv_diff_stats_mv takes the next payload's samples where the vectors of
 * sn_yuv_block_motion point.  a, b, fmt, rect (NULL: the whole frame), H, W and stream exactly as sn_yuv_diff_stats takes them, T >= 2; mv:[T - 1][nby][nbx][2]
 * int8 laid out as sn_yuv_block_motion writes it for the same picture (the written payloads b, by the restorer's use).  Only the luma planes are read,
 * samples are taken as stored (a 16-bit word may hold up to 65535), pair p is payloads p and p + 1.  The picture is h x w, the rectangle or the frame;
 * the block grid is anchored at its first sample and the coordinates below count from there.
 *   hb = h / 2, wb = w / 2: the whole 2 x 2 blocks (i, j).  Block (i, j) is a MEASURING block iff i + j is odd (sn_yuv_block_motion chose its vector on
 *   the other half, so the choice cannot fit what is measured here), and its vector is (dy, dx) = mv[p][i / 8][j / 8].
 *   A measuring block COUNTS iff rows 2 i + dy, 2 i + dy + 1 and columns 2 j + dx, 2 j + dx + 1 lie inside the picture: the rule of
 *   sn_yuv_noise_hist_pairs_mv.  mv is device memory the entry point cannot validate: the test is made per block in the kernel, so ANY int8 contents are
 *   memory-safe.  Nothing is clamped and nothing outside the picture is read.
 *   For each of the four samples (y, x) of a counting block:
 *     d0 = b_p(y, x) - a_p(y, x),  d1 = b_{p+1}(y + dy, x + dx) - a_{p+1}(y + dy, x + dx),  g = b_{p+1}(y + dy, x + dx) - b_p(y, x).
 * dst[p] holds SN_DIFF_STATS_MV = 8 signed 64-bit integers:
 *   0           Nm = the samples counted (4 per counting block)
 *   1, 2        sum d0, sum d0^2
 *   3, 4        sum d1, sum d1^2
 *   5           sum d0 d1
 *   6           sum g^2 (how well the vectors fit the written picture)
 *   7           Nv = the counted samples whose vector is not (0, 0)
 * dst:[T - 1][8] int64 is OVERWRITTEN, never added to; nothing outside those words is written.  Integer sums accumulated in 64 bit: exact, and the same
 * for every launch geometry and schedule.  a == b is legal.  hb == 0 or wb == 0: all zeros.
 * (tests/diff_stats_mv_ref.py restates it in numpy; the kernel equals it word for word.)
 * SN_EINVAL before anything is launched: everything sn_yuv_diff_stats refuses (it takes no edge); T < 2; a null mv; dst not 8-byte aligned; a picture
 * whose ceil(w / 8) x ceil(h / 8) units exceed the bound sn_yuv_diff_stats checks. */
#define SN_DIFF_STATS_MV 8
int sn_yuv_diff_stats_mv(const uint8_t* a, const uint8_t* b, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */,
                         const int8_t* mv, int64_t* dst /* [T - 1][SN_DIFF_STATS_MV] */, int T, int H, int W, void* stream);

/* ---- the blend of a tiled window (csrc/sn_tile.hip; a new symbol, SN_ABI_VERSION stays 20) --------------------------------------------------------
 * The video restorer can run the network on overlapping tiles of a window's frames instead of on whole frames (VideoRestorer(tile=...)); each tile's
 * float32 result is added into one float32 canvas with feather weights that are separable: a tile's weight at (y, x) is wy[y] * wx[x].
 *   tile:[T][C][th][tw] f32, canvas:[T][C][Hc][Wc] f32, wy:[th] f32, wx:[tw] f32, all contiguous device memory; (y0, x0) is the tile's first sample
 *   in a plane of the canvas.  For every t < T, c < C, y < th, x < tw:
 *     w  = wy[y] * wx[x]                                        (one float32 product, rounded)
 *     canvas[t][c][y0 + y][x0 + x] = canvas[t][c][y0 + y][x0 + x] + w * tile[t][c][y][x]      (one product, rounded; one sum, rounded)
 * Three float32 operations, each rounded to nearest even on its own: no FMA, and the same bits for every launch geometry and for the 16-byte and the
 * element-wise path of the kernel (it moves 4 consecutive samples as one float4 where the addresses of both tensors allow, which it tests itself:
 * x0, tw and Wc are arbitrary).  The canvas is ADDED to, never overwritten: the caller zeroes it before a window's first tile.  Nothing outside the
 * th x tw rectangle of each plane is read or written.  Launches on one stream are ordered, so overlapping tiles accumulated one after the other
 * never race; there are no atomics.  The weights are not looked at: any float32 contents are legal.
 * (tests/tile_ref.py restates it in numpy; the kernel equals it bit for bit.)
 * SN_EINVAL before anything is launched: a null pointer; a pointer that is not 4-byte aligned; T, C, th, tw, Hc or Wc < 1; y0 < 0, x0 < 0,
 * y0 + th > Hc or x0 + tw > Wc; T * C > 65535 (the grid's z). */
int sn_tile_accumulate(const float* tile, float* canvas, const float* wy, const float* wx, int T, int C, int th, int tw, int Hc, int Wc,
                       int y0, int x0, void* stream);

/* ---- the data movement of the self-ensemble (csrc/sn_geo.hip; new symbols, SN_ABI_VERSION stays 20) ------------------------------------------------
 * The video restorer and GShiftNet.forward_ensemble_fp32_out can run the network on mirrored, transposed and time-reversed copies of a window
 * (shiftnet_amd/ensemble.py); each float32 result is mapped back and added into one float32 canvas, which the last launch divides by the number of
 * members.  A window then costs M forwards, M the number of members.  The transposed members have another input signature (H and W swapped), so the
 * engine keeps a plan -- and, where forwards are replayed from captured graphs, a graph -- of its own for them.  NOBODY HAS MEASURED WHAT THE ENSEMBLE GAINS
 * ON THIS NETWORK: the +0.05 to +0.2 dB quoted for image super-resolution is a figure from the literature for other networks, not a property of
 * Shift-Net, and no trained checkpoint ships here.  The four inference/test_*.py harnesses, where a PSNR against ground truth could be measured once
 * somebody has a checkpoint, do not take the option yet; GShiftNet.forward_ensemble_fp32_out is there for it.
 *   op: any OR of the four bits, 0 .. 15.  H and W are the sides of src / canvas, both [T][C][H][W]; dst / member is [T][C][H'][W'] with
 *   (H', W') = (W, H) if SN_GEO_TRANSPOSE is set and (H, W) otherwise.  All contiguous device memory.
 * One index map defines both kernels.  For a sample (t', c, y', x') of the transformed tensor (dst / member):
 *     (u, v) = (y', x');   SN_GEO_FLIP_Y: u = H' - 1 - u;   SN_GEO_FLIP_X: v = W' - 1 - v;
 *     (y, x) = (v, u) with SN_GEO_TRANSPOSE, else (u, v);   t = T - 1 - t' with SN_GEO_REVERSE_T, else t'
 *   sn_geo_transform :  dst[t'][c][y'][x'] = src[t][c][y][x] -- pure data movement of esz-byte elements, esz = 2 (bf16 and fp16 alike) or 4
 *   sn_geo_accumulate:  a = init ? member[t'][c][y'][x'] : canvas[t][c][y][x] + member[t'][c][y'][x']     (one float32 sum, rounded)
 *                       canvas[t][c][y][x] = a * scale                                                    (one float32 product, rounded)
 *     No FMA; with init != 0 the canvas is not read, so whatever it held -- NaN included -- does not reach the result.
 * The map is a bijection, so every sample of the tensor written is written exactly once; nothing outside the two tensors is read or written.  The
 * inverse of an op with the transpose bit is the op with its two flip bits swapped (5 and 6 are each other's inverses, 4 and 7 their own); without
 * it every op is its own inverse.  So sn_geo_accumulate(member = sn_geo_transform(a, op), op, init = 1, scale = 1) gives a back.
 * Without SN_GEO_TRANSPOSE a thread moves 16 bytes of a row where both addresses are 16-byte aligned (it tests the addresses itself; the mirrored
 * chunk of SN_GEO_FLIP_X is aligned only when W * esz is a multiple of 16) and goes element by element otherwise; with it a workgroup moves a
 * 64 x 64 tile through LDS so that reads and writes both run along rows.  Every path gives the same bits.  No atomics: the launches of a window
 * run one after the other on one stream.  T * C is NOT limited by the grid: the kernels loop over the planes beyond 65535.
 * (tests/geo_ref.py restates both in numpy; the kernels equal it bit for bit.)
 * SN_EINVAL before anything is launched: a null pointer; a pointer that is not esz-byte aligned (4 for sn_geo_accumulate); esz not 2 or 4; op outside
 * 0 .. 15; T, C, H or W < 1; T * C * H * W * esz beyond 2^63 - 1 (the kernels index with 64 bits); a scale that is not finite; src / dst
 * (member / canvas) byte ranges that overlap. */
#define SN_GEO_FLIP_X 1      /* mirror the columns */
#define SN_GEO_FLIP_Y 2      /* mirror the rows */
#define SN_GEO_TRANSPOSE 4   /* swap rows and columns (applied before the flips) */
#define SN_GEO_REVERSE_T 8   /* frame t' is frame T - 1 - t' */
int sn_geo_transform(const void* src, void* dst, int esz, int op, int T, int C, int H, int W, void* stream);
int sn_geo_accumulate(const float* member, float* canvas, int op, int init, float scale, int T, int C, int H, int W, void* stream);

/* ---- the cross-fade of overlapping windows (csrc/sn_time.hip; a new symbol, SN_ABI_VERSION stays 20) ------------------------------------------------
 * The video restorer can let consecutive windows of a scene overlap by V frames (VideoRestorer(window_overlap=V)); the V shared frames then have two
 * float32 answers, the older window's last V frames and the newer window's first V, which are cross-faded with a linear ramp in time.
 *   prev, cur:[V][C][Hp][Wp] f32, w_prev, w_cur:[V] f32, sq: NULL or [V][C] u64, all contiguous device memory; h x w is the picture inside the padded
 *   Hp x Wp plane.  prev is read only, cur is updated in place.  For every j < V, c < C, y < Hp, x < Wp:
 *     cur[j][c][y][x] = (w_prev[j] * prev[j][c][y][x]) + (w_cur[j] * cur[j][c][y][x])      (two products and one sum, each rounded)
 * Three float32 operations, each rounded to nearest even on its own: no FMA, and the same bits for every launch geometry and for the 16-byte and the
 * element-wise path of the kernel (it moves 4 consecutive samples as one float4 where the addresses in both tensors allow, which it tests itself:
 * Hp and Wp are arbitrary).  The weights are not looked at: any float32 contents are legal.
 * With sq the kernel also measures how far the two answers are apart, from the values BEFORE the blend and over the picture only (y < h and x < w):
 *     d = prev - cur                                            (one float32 difference, rounded)
 *     q = rint(min(max(d, -8), 8) * 65536)                      (round half to even; an integer, |q| <= 2^19; a NaN d counts as -8)
 *     sq[j][c] += q * q                                         (unsigned 64-bit integers)
 * sq is ADDED to, never overwritten: the caller zeroes it.  Integer sums are exact and do not depend on the launch geometry; a workgroup adds its sum
 * with one 64-bit vector atomic.  h * w <= 2^25 keeps a plane's sum below 2^63.  A difference beyond +-8 counts as 8: the clamp bounds the sum, and
 * the restorer's values are pictures in [0, 1] give or take an overshoot.  With sq == NULL an instantiation without any of the statistic runs.
 * (tests/time_ref.py restates both in numpy and Python integers; the kernel equals them bit for bit.)
 * SN_EINVAL before anything is launched: a null prev, cur, w_prev or w_cur; one of them not 4-byte aligned, or sq not 8-byte aligned; V, C, Hp or
 * Wp < 1; h outside 1 .. Hp or w outside 1 .. Wp; V * C > 65535 (the grid's z); with sq, h * w > 2^25. */
int sn_time_crossfade(const float* prev, float* cur, const float* w_prev, const float* w_cur, unsigned long long* sq /* NULL: no statistic */,
                      int V, int C, int Hp, int Wp, int h, int w, void* stream);

/* ---- no-reference quality: the per-pixel part of NIQE (csrc/sn_niqe.hip; a new symbol, SN_ABI_VERSION stays 20) ------------------------------------
 * NIQE (Mittal, Soundararajan, Bovik 2013) scores a picture by the distance of the statistics of its 96 x 96 blocks, at two scales, from those of
 * pristine natural images.  Per block and scale it fits five asymmetric generalised Gaussians: to the locally normalised luma and to its products with
 * four neighbours.  Each fit needs five sums of its map; sn_yuv_niqe_sums makes those sums, shiftnet_amd/niqe.py does the rest on the host in float64.
 *   src: T payloads as sn_ingest_yuv takes them; only the luma plane is read, and of fmt only bits and range decide anything.  rect (NULL: the whole
 *   frame) as sn_ingest_yuv_rect takes it: the picture is its h x w luma samples and everything below is what the cropped stream would give.
 *   win7: 7 float32 taps win7[0..6] in device memory, the separable factor of the model's 7 x 7 window.  dst:[T][2][nbh][nbw][SN_NIQE_MAPS][SN_NIQE_SUMS]
 *   doubles, nbh = h / 96, nbw = w / 96 (integer division); only the top-left 96 nbh x 96 nbw samples of the picture count and are read.
 * Everything is float64, every product and sum rounded on its own (no FMA), square root and division correctly rounded.
 * Sample value:  limited range v = code * 2^-(bits - 8);  full range v = 16 + code * k, k = (double)(float)(219.0 / (2^bits - 1)): both on the 16 .. 235
 *   scale of an 8-bit limited-range Y', and both exact (a 10-bit code times a 24-bit constant).
 * Scale 1: I = v, hs x ws = 96 nbh x 96 nbw.  Scale 2: I(y, x) = 0.25 * ((v(2y, 2x) + v(2y, 2x+1)) + (v(2y+1, 2x) + v(2y+1, 2x+1))), hs x ws half of that
 *   (exact).
 * Taps: a 7-tap sum adds its terms p0 .. p6 from the outside in, sum7(p) = (((p0 + p6) + (p1 + p5)) + (p2 + p4)) + p3.  w[i] = (double)win7[i],
 *   g[i] = w[i] / sum7(w): the float32 taps over their own sum, which add up to 1 to an ulp whatever their roundings added up to.
 *   (Taps that add up to 0 give NaNs; nothing checks device memory.)
 * Per scale and per block of side B = 96 / scale, block (by, bx) being rows by B .. by B + B - 1 and columns bx B .. of that scale: the filters run on
 * the deviations from the block's own first sample, J = I - p with p = I(by B, bx B) (exact), for the block's samples and for the 3 samples around it
 * that belong to its neighbours alike; n and the variance do not change under that shift, and a flat area has J = 0, every product and sum 0 and
 * n = 0 / (0 + 1) = 0 exactly, at every code.  cy / cx clamp to 0 .. hs - 1 / 0 .. ws - 1 (the replication is at the crop of that scale, not at the
 * frame), (y, x) inside the block:
 *     r1(y, x) = sum7_i g[i] * J(y, cx(x + i - 3))             r2(y, x) = sum7_i g[i] * (J * J)(y, cx(x + i - 3))
 *     mu(y, x) = sum7_j g[j] * r1(cy(y + j - 3), x)            m2(y, x) = sum7_j g[j] * r2(cy(y + j - 3), x)
 *     n = (J - mu) / (sqrt(|m2 - mu * mu|) + 1)                kept as a double
 *     map 0: m = n(y, x);   maps 1..4: m = n(y, x) * n((y - dy) mod B, (x - dx) mod B), (dy, dx) = (0, 1), (1, 0), (1, 1), (1, -1)   (one product;
 *     the wrap is inside the block).
 * dst[t][scale - 1][by][bx][map] holds five doubles:
 *     [0] the count of m < 0   [1] the sum of m^2 over m < 0   [2] the count of m > 0   [3] the sum of m^2 over m > 0   [4] the sum of |m|
 * One workgroup owns one (frame, scale, block), adds in one fixed order and writes its 25 doubles with plain stores; there are no atomics.  The
 * result does not depend on the launch geometry or the schedule, and a second launch gives the same bits.  Only dst is written, every word of it.
 * (tests/niqe_ref.py restates this rounding for rounding: the counts are equal and the sums differ by the order in which a block's values are added,
 * 1e-12 at most.  Against the same formula on the values themselves in long double with unrounded taps the sums are within 3e-8, the rounding of
 * the taps to float32, on textured and on near-flat frames alike.  Until the kernel computed in float64 on deviations it was float32 on the values,
 * and lost up to 8e-3 of a sum on near-flat bright frames and left a one-signed residue on flat frames of some codes: DESIGN.md 3.33.)
 * SN_EINVAL before anything is launched: a null src, fmt, win7 or dst; bits not 8 or 10 or an unknown chroma code; a rectangle sn_ingest_yuv_rect
 * refuses; T outside 1 .. 65535; H or W < 1; no whole block (nbh * nbw == 0); dst not 8-byte or win7 not 4-byte aligned; src at an odd address at
 * 10 bit. */
#define SN_NIQE_BLOCK 96
#define SN_NIQE_MAPS 5
#define SN_NIQE_SUMS 5
int sn_yuv_niqe_sums(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */,
                     const float* win7 /* device, 7 taps */, double* dst /* [T][2][nbh][nbw][5][5] */,
                     int T, int H, int W, void* stream);

/* ---- full-reference quality: the per-pixel part of SSIM (csrc/sn_ssim.hip; a new symbol, SN_ABI_VERSION stays 20) -----------------------------------
 * The video restorer can compare what it read and what it wrote with a ground-truth stream (VideoRestorer.restore(..., gt=...)): PSNR of all three
 * planes comes from the exact sums of sn_yuv_diff_stats with a set to the truth, and SSIM of the luma from sn_yuv_ssim_sums; shiftnet_amd/fullref.py
 * does the rest on the host in float64.  The definition is the Y-channel SSIM of the evaluation harnesses (upstream's _ssim_cly): an 11 x 11 Gaussian
 * window, the border replicated, every position counted.  sn_ssim_u8 above is the harness CLI's volume SSIM over interleaved 8-bit RGB: another formula
 * on another layout.
 *   a, b, fmt, rect (NULL: the whole frame), H, W and stream exactly as sn_yuv_diff_stats takes them.  Only the luma planes are read and samples are
 *   taken as stored (a 16-bit word may hold up to 65535).  The picture is h x w, the rectangle or the frame; coordinates below count from its first
 *   sample, and cy / cx clamp to 0 .. h - 1 / 0 .. w - 1: the border is replicated at the edge of the picture, not of the frame, so a rectangle gives
 *   what the cropped stream gives.
 * Constants: g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum_j exp(-(j - 5)^2 / (2 * 1.5^2)), i = 0 .. 10, float64, computed on the host; the window is their
 *   outer product.  p = 2^bits - 1, C1 = (0.01 p)^2, C2 = (0.03 p)^2, float64.  At 8 bit this is the harnesses' formula on their 0 .. 255 scale; at
 *   10 bit it is the same formula on codes * 255 / 1023, because SSIM does not change when the constants scale with the data.
 * Float64 from the codes on (a product of two codes is exact), every product, sum and difference rounded on its own (no FMA); an 11-tap sum adds its
 *   products p0 .. p10 from the outside in, ((((p0 + p10) + (p1 + p9)) + (p2 + p8)) + (p3 + p7)) + (p4 + p6)) + p5:
 *     r_X(y, x) = sum_i g[i] * X(y, cx(x + i - 5))  for the five maps X = a, b, a * a, b * b, a * b  (the product first, then the tap)
 *     G_X(y, x) = sum_j g[j] * r_X(cy(y + j - 5), x)
 *     s_aa = G_aa - G_a * G_a,  s_bb = G_bb - G_b * G_b,  s_ab = G_ab - G_a * G_b
 *     map  = ((2 * (G_a * G_b) + C1) * (2 * s_ab + C2)) / (((G_a * G_a + G_b * G_b) + C1) * ((s_aa + s_bb) + C2))
 *   (Until the near-flat pairs of tests/ssim_cases.py this was float32 on codes minus mid-grey: the variances of a flat area far from mid-grey lost
 *   their digits, a frame of code 2 came out 2e-5 from the reference and a tile 6e-5.)
 * dst[t][i][j] is the float64 sum of map over tile (i, j) of frame t: positions y = SN_SSIM_TILE i .. , x = SN_SSIM_TILE j .. of
 * the picture, SN_SSIM_TILE each way, the last row and column of tiles partial; nty = ceil(h / SN_SSIM_TILE), ntx = ceil(w / SN_SSIM_TILE).  All h w
 * positions count; a frame's SSIM is the sum of its tiles over h w.  dst:[T][nty][ntx] doubles is OVERWRITTEN, never added to; nothing outside those
 * words is written.  One workgroup owns one (frame, tile), adds in one fixed order and writes its double with a plain store; there are no atomics.
 * The result does not depend on the launch geometry or the schedule, and a second launch gives the same bits.  a == b is legal: numerator and
 * denominator are then the same float64 expressions, map is exactly 1 everywhere, and every tile's sum is exactly its number of positions.
 * (tests/ssim_ref.py restates it with numpy; the kernel's per-frame SSIM is within 1e-5 of what the harnesses' code gives, on near-flat pictures too.)
 * SN_EINVAL before anything is launched: everything sn_yuv_diff_stats refuses (it takes no edge); dst not 8-byte aligned; a tile grid, nty * ntx,
 * beyond the bound sn_yuv_diff_stats puts on its units (2^31 - 1 - 2^18). */
#define SN_SSIM_TILE 32
int sn_yuv_ssim_sums(const uint8_t* a, const uint8_t* b, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */,
                     double* dst /* [T][nty][ntx] */, int T, int H, int W, void* stream);

/* ---- noise added to a clean stream (csrc/sn_degrade.hip; a new symbol and a new struct, SN_ABI_VERSION stays 20) -------------------------------------
 * The first half of the experiment the ground truth above is for: a degraded copy of a clean stream (VideoRestorer(add_noise=...)), as upstream's
 * denoise harnesses make one -- in_tensor + normal_(0, sigma) on R'G'B' -- but from payloads to payloads, with no float frame in memory.
 *   src: T payloads of fmt, H x W, as sn_ingest_yuv takes them; dst: T payloads of the same format and size, whole frames, as sn_egress_yuv writes them.
 *   Payload t is frame f = noise->t0 + t of the stream.  Per pixel (y, x), every float32 product and sum rounded separately (no FMA):
 *   1. R, G, B: sn_ingest_yuv's float32 values of the pixel (its constants, its integer chroma upsampling for both 4:2:0 sitings, clamped to [0, 1]);
 *      they are not rounded to a module dtype.
 *   2. s: the curve noise->knots -- SN_NLF_BANDS = 16 sigmas in 8-bit R'G'B' code units, knot b at luma code lo + (b + 0.5) (hi - lo) / 16 with lo, hi
 *      the format's black and white luma codes (16 s, 235 s limited; 0, 2^bits - 1 full) -- at the pixel's own CLEAN luma code Y, with
 *      sn_noise_map_level's interpolation:  k[b] = knots[b] / 255, a float64 quotient rounded ONCE to float32;
 *        u = min(max((float(Y) - float(lo)) * sc - 0.5, 0), 15)   with sc = 16 / (hi - lo), a float64 expression rounded ONCE to float32
 *        i = min(int(floor(u)), 14);  e = u - float(i);  s = k[i] + e * (k[i + 1] - k[i])
 *      A flat curve gives exactly k[0] at every pixel; a curve written here and one read by sn_noise_map_level mean the same thing.
 *   3. R' = R + s * g(f, 0, y, x), G' = G + s * g(f, 1, y, x), B' = B + s * g(f, 2, y, x), NOT clamped, with g(f, c, y, x) = gauss[h >> 16] and
 *        h = the murmur3 finaliser of  (y * 0x9E3779B1) ^ (x * 0x85EBCA77) ^ (f * 0xC2B2AE3D) ^ ((3 + c) * 0x27D4EB2F) ^ seed       (uint32, products wrap)
 *      exactly as sn_egress_yuv_dither hashes: planes 3 .. 5 of the seed space whose planes 0 .. 2 are the dither's, so the two are independent.
 *      gauss: 65536 float32 in DEVICE memory that the host makes once (shiftnet_amd/degrade.py: gauss_table): entry k is the standard normal quantile
 *      at (k + 0.5) / 65536 in float64, divided by the root mean square of the 65536 quantiles, then rounded: mean 0, variance 1, antisymmetric, the
 *      largest about 4.3.  A lookup and not Box-Muller: the numpy restatement is the kernel bit for bit.
 *   4. The codes written are sn_egress_yuv's for the frame R', G', B': clamped to [0, 1], the matrix, both 4:2:0 downsampling filters with coordinates
 *      clamped to the frame (a clamped pixel is the frame's pixel at the clamped place, its noise included), rounding, the legal code range.
 * The noise is a pure function of (seed, f, c, y, x): the bytes do not depend on the launch geometry, and T frames in one launch are the T launches
 * with t0, t0 + 1, ...  (tests/degrade_ref.py restates it in numpy; the kernel equals it bit for bit.)  The per-thread layout is sn_egress_yuv's: 8 x 2
 * pixels, wide loads and stores where the address allows, element-wise with the same arithmetic elsewhere; the left-sited 4:2:0 filter's pixel
 * x0 - 1 is recomputed by the thread that needs it.  Only dst is written.
 * SN_EINVAL before anything is launched: everything sn_egress_yuv refuses of fmt, T, H, W and dst, the same of src; a null noise or gauss; gauss not
 * 4-byte aligned; t0 < 0; a knot that is negative or not finite; byte ranges [src, src + T frame_bytes) and [dst, dst + T frame_bytes) that overlap. */
typedef struct sn_yuv_degrade_noise { uint32_t seed; int t0; float knots[16]; } sn_yuv_degrade_noise;
int sn_yuv_degrade(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_degrade_noise* noise, const float* gauss /* device, 65536 */, uint8_t* dst,
                   int T, int H, int W, void* stream);

/* ---- motion blur of a sharp stream (csrc/sn_blur.hip; a new symbol and a new struct, SN_ABI_VERSION stays 20) ----------------------------------------
 * The same experiment for the deblurrers (VideoRestorer(add_blur=...)): a blurred copy of a sharp stream, made as the deblur datasets are -- GOPRO and
 * DVD average consecutive frames of a high-frame-rate stream, GOPRO in linear light through an inverse gamma of 2.2, and keep the sharp centre frame
 * for the truth -- but from payloads to payloads, with no float frame in memory.
 *   src: S payloads of fmt, H x W, as sn_ingest_yuv takes them; dst: T payloads of the same format and size, whole frames, as sn_egress_yuv writes them.
 *   win: n taps, odd, 1 .. SN_BLUR_MAX_TAPS, r = n / 2.  Output t is the mean over j = -r .. r of source payload clamp(c0 + t + j, lo, hi): a clamped
 *   index counts as often as it occurs, so the ends of a stream or of a scene [lo, hi] are replicated.
 *   Per pixel (y, x) and channel, every float32 product and sum rounded separately (no FMA), no division, no powf, no exp2f:
 *   1. Per tap j, R, G, B: sn_ingest_yuv's float32 values of the pixel in that source payload (its constants, its integer chroma upsampling for both
 *      4:2:0 sitings, clamped to [0, 1]); they are not rounded to a module dtype.
 *   2. With tables, each of them is decoded into linear light:
 *        u = R * 4095.0f;  i = min((int)u, 4094);  e = u - (float)i;  v = lin[i] + e * (lin[i + 1] - lin[i])
 *      Without tables (lin and rinv both NULL: gamma 1), v = R.
 *   3. acc = v(-r), then acc = acc + v(j) in ascending j; m = acc * inv_n with inv_n = 1.0 / n, a float64 quotient rounded ONCE to float32.
 *   4. With tables, the mean is encoded: i = the largest index in 0 .. 4094 with lin[i] <= m;
 *        e = min((m - lin[i]) * rinv[i], 1.0f);  x = ((float)i + e) * k        with k = 1.0 / 4095, a float64 quotient rounded ONCE to float32
 *      Without tables, x = m.
 *      lin: 4096 float32 in DEVICE memory, strictly increasing from 0 to 1; rinv: 4095 float32 in DEVICE memory, rinv[i] = 1 / (lin[i + 1] - lin[i]); the
 *      host makes both once per gamma (shiftnet_amd/degrade.py: gamma_tables: lin[i] = (i / 4095) ** gamma in float64, rounded once).  Tables and not
 *      powf: the numpy restatement is the kernel bit for bit.  A pure power law, not the sRGB curve.
 *   5. The codes written are sn_egress_yuv's for the frame x: clamped to [0, 1], the matrix, both 4:2:0 downsampling filters with coordinates clamped
 *      to the frame, rounding, the legal code range.
 * The bytes do not depend on the launch geometry, and T outputs in one launch are the T launches of one output with c0, c0 + 1, ...; n = 1 without
 * tables is egress(ingest(src)).  (tests/blur_ref.py restates it in numpy; the kernel equals it bit for bit.)  The per-thread layout is sn_egress_yuv's:
 * 8 x 2 pixels, wide loads and stores where the address allows, element-wise with the same arithmetic elsewhere; the left-sited 4:2:0 filter's pixel
 * x0 - 1 is recomputed by the thread that needs it; blockIdx.z is the output frame; both tables are copied into LDS (32 KB).  Only dst is written.
 * SN_EINVAL before anything is launched: everything sn_yuv_degrade refuses of fmt, T, H, W, src and dst; S < 1; a null win; n even or outside
 * 1 .. SN_BLUR_MAX_TAPS; anything but 0 <= lo <= hi < S; c0 < lo or c0 + T - 1 > hi; exactly one of lin / rinv being null; a table that is not 4-byte
 * aligned; byte ranges [src, src + S frame_bytes) and [dst, dst + T frame_bytes) that overlap.  No index reaches the device unchecked. */
#define SN_BLUR_MAX_TAPS 15
typedef struct sn_yuv_blur_window { int n; int c0; int lo; int hi; } sn_yuv_blur_window;
int sn_yuv_blur(const uint8_t* src, int S, const sn_yuv_fmt* fmt, const sn_yuv_blur_window* win,
                const float* lin /* device, 4096, or NULL */, const float* rinv /* device, 4095, or NULL */,
                uint8_t* dst, int T, int H, int W, void* stream);

/* ---- grain put back on a restored stream (csrc/sn_grain.hip; a new symbol and a new struct, SN_ABI_VERSION stays 20) ---------------------------------
 * The last step of "denoise, encode, re-grain" (VideoRestorer(grain=...)): a controlled share of fine, spatially correlated Gaussian grain on the codes
 * that were written, from payloads to payloads.
 *   src: T payloads of fmt, H x W; dst: T payloads of the same format and size.  rect == NULL: whole frames; else only the rectangle's samples, luma
 *   and chroma, are read and written, and it is the picture (sn_egress_yuv_rect's rules).  Payload t is frame f = grain->t0 + t of its clip.
 *   Float32 throughout, every product and sum rounded separately (no FMA); rint is round-to-nearest-even (__float2int_rn).
 *   White field of plane p (6: Y, 7: Cb, 8: Cr; the dither owns 0 .. 2, sn_yuv_degrade 3 .. 5 of the same seed space):
 *        g_p(f, y, x) = gauss[h >> 16],  h = the murmur3 finaliser of  (y * 0x9E3779B1) ^ (x * 0x85EBCA77) ^ (f * 0xC2B2AE3D) ^ (p * 0x27D4EB2F) ^ seed
 *      y, x: the sample's row and column IN ITS OWN PLANE counted from the picture's first sample (the frame's, or the rectangle's as the dither counts
 *      them).  Any integer is legal: negative coordinates wrap as uint32, so the field has no edge and nothing is clamped.  gauss: sn_yuv_degrade's table.
 *   Correlated field: a separable 5-tap filter (w2, w1, w0, w1, w2) with taps = {w0, w1, w2}:
 *        h(y, x) = (((w2 * g(y, x - 2) + w1 * g(y, x - 1)) + w0 * g(y, x)) + w1 * g(y, x + 1)) + w2 * g(y, x + 2)
 *        c(y, x) = (((w2 * h(y - 2, x) + w1 * h(y - 1, x)) + w0 * h(y, x)) + w1 * h(y + 1, x)) + w2 * h(y + 2, x)
 *   Level: s(Y), the curve grain->knots -- SN_NLF_BANDS = 16 values ALREADY IN LUMA CODE UNITS OF fmt (the host converts them) -- at a luma code, with
 *      sn_yuv_degrade's interpolation: u = min(max((float(Y) - float(lo)) * sc - 0.5, 0), 15), sc = 16 / (hi - lo) in float64 rounded once;
 *      i = min(int(floor(u)), 14); s = k[i] + (u - float(i)) * (k[i + 1] - k[i]).
 *   Luma:   Y' = clamp(rint(float(Y) + s(Y) * c_6), min(ylo, Y), max(yhi, Y))
 *   Chroma: C' = clamp(rint(float(C) + (chroma * s(Ym)) * c_p), min(clo, C), max(chi, C)), p = 7, 8; Ym is the luma code READ FROM src: at 4:4:4 the
 *      same pixel's; at either 4:2:0 siting (Y00 + Y01 + Y10 + Y11 + 2) >> 2 of the sample's 2 x 2 block, coordinates clamped to the picture.  The
 *      chroma field lives on the chroma plane's own lattice.
 *   So: all knots 0 returns src byte for byte, illegal codes included; chroma == 0 leaves chroma as it came; taps {1, 0, 0} is white grain.
 * The grain is a pure function of (seed, f, p, y, x): the bytes do not depend on the launch geometry or the tiling, and T frames in one launch are
 * the T launches with t0, t0 + 1, ...  (tests/grain_ref.py restates it in numpy, knowing no tiles; the kernel equals it byte for byte.)  A workgroup
 * owns 256 x 16 luma samples: the white field of the tile plus a halo of 2 is gathered once into LDS, the horizontal pass goes LDS to LDS, the
 * vertical pass LDS to registers, the chroma tiles follow in the same buffers where chroma != 0.  dst == src (in place) is legal: a thread owns its
 * 8 x 2 luma samples and their chroma, reads them before it stores, and takes the filter's neighbours from the hash, not from memory.
 * SN_EINVAL before anything is launched: everything sn_yuv_degrade refuses of fmt, T, H, W, src, dst and gauss; a rectangle sn_egress_yuv_rect
 * refuses; a null grain; t0 < 0; a knot or chroma that is negative or not finite; a tap that is negative or not finite, w0 <= 0, or
 * w0^2 + 2 w1^2 + 2 w2^2 further than 1e-3 from 1; byte ranges of src and dst that overlap without being the same. */
typedef struct sn_yuv_grain_noise { uint32_t seed; int t0; float knots[16]; float chroma; float taps[3]; } sn_yuv_grain_noise;
int sn_yuv_grain(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* or NULL */, const sn_yuv_grain_noise* grain,
                 const float* gauss /* device, 65536 */, uint8_t* dst, int T, int H, int W, void* stream);

/* ---- brightness flicker taken out (csrc/sn_deflicker.hip; two new symbols, SN_ABI_VERSION stays 20) ---------------------------------------------------
 * The two device steps of VideoRestorer(deflicker=R): the luma histogram of every payload, and one tone curve per frame applied to the payloads.  The
 * rule between them is the host's (shiftnet_amd/deflicker.py; restated by tests/deflicker_ref.py).  No float frame, no colour conversion.
 *   The rule (host, float64 and exact integers; h_t the histogram of frame t, C_t its running sum, C_t[-1] = 0, the clip [lo, hi), R = 1 .. 15):
 *        r = min(R, t - lo, hi - 1 - t); for every code c with h_t[c] > 0: a = C_t[c - 1] + C_t[c]; for s = t - r .. t + r: k the smallest code with
 *        2 C_s[k] >= a and Q_s = ((2k - 1) h_s[k] + a - 2 C_s[k - 1]) / (2 h_s[k]), one division; lutY_t[c] = clamp(floor(median_s Q_s + 0.5), 0, L - 1);
 *        an absent code takes the value of the nearest present code below it, or of the first present one.
 *        Chroma: m, m' the mean luma code before and after the table (sum of code * count, one division by N), yo the luma black code,
 *        k = clamp((m' - yo) / (m - yo), 0.5, 2), k = 1 when m - yo < 1 or lutY is the identity on every present code;
 *        lutC_t[c] = clamp(floor(co + k (c - co) + 0.5), 0, L - 1), co = 128 * 2^(bits - 8); or the identity.
 *   L = 2^bits.  A 10-bit payload is 16-bit words and may hold anything: BOTH kernels index with min(code, L - 1) before any use.
 * sn_yuv_code_hist: src: T payloads of fmt, H x W -> dst[t][c], t < T, c < L, uint32: the number of luma samples of payload t -- of the whole frame
 *   (rect == NULL) or of the rectangle (sn_egress_yuv_rect's rules) -- whose index min(code, L - 1) is c.  Exact; every frame's bins sum to its sample
 *   count.  dst is ZEROED BY THE CALL (on the stream, ahead of the kernel), as sn_yuv_noise_hist zeroes its own: it is overwritten, not added to.
 *   Private histograms in LDS (32 copies at 8 bit, 8 at 10; equal neighbours among a lane's 16 bytes of samples are one add of the run's length, so
 *   a flat frame costs a sixteenth of the LDS atomics and never two lanes of a group on one word at 8 bit), one global atomic per non-empty bin.
 * sn_yuv_apply_lut: lut: device, [T][2][L] uint16, 4-byte aligned: per payload the table of the luma plane, then the table of BOTH chroma planes.
 *   dst[sample] = lut[t][plane ? 1 : 0][min(src[sample], L - 1)] for every sample of the frame, or of the rectangle; the value is stored as the
 *   format stores a code (8 bit: its low byte; tables hold codes <= L - 1).  Samples outside rect are not touched.  No table is assumed monotone.
 *   dst == src (in place) is legal: a thread stores only the samples it alone has read.  The tables of a frame go into LDS once per workgroup.
 * SN_EINVAL before anything is launched, both: a null src / fmt / dst / lut; bits other than 8 and 10, a chroma, matrix or range code out of range;
 * T outside 1 .. 65535; H or W < 1; at 10 bit an odd address of a payload; dst (histograms) or lut not 4-byte aligned; a rectangle
 * sn_egress_yuv_rect refuses; more than 2^32 - 1 samples in the picture (histograms); byte ranges of src and dst that overlap without being the same
 * (tables). */
int sn_yuv_code_hist(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* or NULL */,
                     uint32_t* dst /* [T][1 << bits] */, int T, int H, int W, void* stream);
int sn_yuv_apply_lut(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* or NULL */,
                     const uint16_t* lut /* device, [T][2][1 << bits]: Y, then Cb and Cr */, uint8_t* dst,
                     int T, int H, int W, void* stream);

/* ---- dirt and blotches taken out (csrc/sn_despot.hip; a new symbol, SN_ABI_VERSION stays 20) -----------------------------------------------------------
 * The device step of VideoRestorer(despot=T): the spike detection index of the film-restoration literature (Kokaram) along the integer block vectors
 * of sn_yuv_block_motion, and the repair.  Payloads in, payloads out, the whole frame; no float frame, no colour conversion; fmt->matrix and
 * fmt->range decide nothing.  Samples are taken as stored (a 16-bit word may hold up to 65535) and all arithmetic is on ints.
 * src: S payloads of fmt, H x W.  dst[i], i < n, is frame f = f0 + i repaired from the ORIGINAL frames f - 1, f, f + 1 of src, never from a repaired
 * neighbour.  mv_next, mv_prev: device, [S - 1][nby][nbx][2] int8 (dy, dx) in the layout of sn_yuv_block_motion for the same picture: mv_next[f] is
 * what it writes for the pair (f, f + 1), mv_prev[f - 1] the vector of frame f's block into frame f - 1 (the matcher run on the time-reversed stack,
 * flipped back along its first axis).  counts: device, [n][2] uint32, OVERWRITTEN: per frame the core seeds and the luma samples replaced.
 *   Vectors.  The vector of luma sample (y, x) is that of block (min(y / 16, nby - 1), min(x / 16, nbx - 1)): a last odd row or column, which belongs
 *        to no block, borrows its neighbour's.  Displaced coordinates are CLAMPED to the plane; with the matcher's vectors the clamp acts on that odd
 *        row or column only, and with ANY int8 contents it keeps every read inside the payloads.  A picture without a vector block (H < 2 or W < 2)
 *        has no seeds: dst is a copy and the counts are 0; the vectors are not read.
 *   Seed.  c = Y_f(y, x), p = Y_{f-1} at the place displaced by the previous vector, n = Y_{f+1} at the place displaced by the next; a = c - p,
 *        b = c - n; d = min(|a|, |b|) if a and b are both positive or both negative, else 0.  The sample is a SEED iff d > threshold + |p - n|.
 *   Support.  A seed is a CORE seed iff at least `support` of its eight neighbours are seeds; samples outside the picture are not seeds.
 *   Grow.  The mask M is the core seeds dilated by the (2 grow + 1) x (2 grow + 1) square, inside the picture.
 *   Repair.  A luma sample in M becomes (p + n + 1) >> 1; every other luma sample is the source's.  Chroma, chroma == 1 (follow): at 4:4:4 a chroma
 *        sample is repaired iff its luma sample is in M, with the same vector; at 4:2:0 (either siting) iff any of its up to four luma samples inside
 *        the picture is in M, with the vector of luma sample (2 cy, 2 cx), both components halved by an arithmetic shift right, the coordinates clamped
 *        to the chroma plane; the value is (pu + nu + 1) >> 1, likewise for V.  chroma == 0 (off): chroma is the source's.
 *   One launch: a workgroup owns a 128 x 32 luma tile (8 x 2 vector blocks) and its chroma, makes the seeds of the tile plus a halo of 1 + grow into
 *   an LDS byte mask, derives the core seeds and M from LDS, and adds its two counts with two global atomics at most.  Integer sums commute.
 * (tests/despot_ref.py restates the rule with numpy on Python ints; the kernel equals it byte for byte and count for count.)
 * SN_EINVAL before anything is launched: a null src / fmt / mv_prev / mv_next / dst / counts; bits other than 8 and 10, a chroma, matrix or range
 * code out of range; S outside 1 .. 65535; H or W < 1; at 10 bit an odd address of src or dst; counts not 4-byte aligned; f0 < 1, n < 1 or
 * f0 + n > S - 1; threshold < 0, support outside 0 .. 8, grow outside 0 .. 2, chroma other than 0 and 1; byte ranges of dst (n payloads) and src
 * (S payloads) that overlap, because a frame's neighbours read its original; more than 65535 x 32 rows (a grid dimension). */
int sn_yuv_despot(const uint8_t* src, const sn_yuv_fmt* fmt, const int8_t* mv_prev, const int8_t* mv_next, uint8_t* dst, uint32_t* counts /* [n][2] */,
                  int S, int f0, int n, int threshold /* in the format's codes */, int support, int grow, int chroma /* 0 off, 1 follow */,
                  int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif
