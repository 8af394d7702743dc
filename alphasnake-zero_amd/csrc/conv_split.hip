// conv_split.hip -- the Q-net's 3x3 residual-tower layer (alpha_nnet.py:25-47) at float32 accuracy on the
// f16 matrix pipe of gfx950.
//
// Every float32 operand v is carried as two f16 numbers, hi = f16(v) and lo = f16(v - hi) (22 significand bits
// together); a product is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with float32 accumulation (the lo*lo
// term is below float32 resolution).  Three 32-cycle MFMAs of k = 16 replace eight 64-cycle f32 MFMAs of k = 2:
// 5.3x the f32 MFMA rate, 2.6x the Winograd kernel's arithmetic rate, at the same |dQ| (about 3e-7 for the whole
// net, tests/test_net_gpu.py).  Weights are pre-scaled by a power of two so that their lo parts are normal f16
// numbers; the inverse goes into the batch-norm scale (exact).  Activations are multiplied by a caller-chosen power
// of two on the way into LDS (so that their lo parts are normal numbers too) and clamped to +-65504 after it; a clamp
// sets the layer's range flag (a word behind the scales in the weight image) so that the host can refuse the result.
//
// GEMM rows are the image's pixels in row-major order, 32 per M tile (14 tiles at 21x21, 7 junk rows).  One block =
// up to 8 consecutive M tiles of one image (7 + 7 at 21x21) x all 128 outputs, 4 wavefronts, at most 128 accumulator
// registers per wave, so TWO blocks share a CU (2 waves per SIMD, 68 KB of LDS each): while one is in its prologue or
// epilogue the other one's MFMAs keep the matrix pipe busy.
// The image rows a block needs (those of its pixels, one above, one below) sit in LDS with a zero border, rows pitched
// W + 1 so that the right border of a row is the left border of the next: the input of output pixel (y, x) for tap
// (dy, dx) is at LDS position of (y, x) + dy (W+1) + dx, so all nine taps of an MFMA A-fragment are the SAME LDS image
// at nine constant offsets from the lane's pixel address -- the rows are staged (and split into hi/lo) once per
// 16-channel chunk, not once per tap.  Wave wn owns outputs 32 wn .. 32 wn + 31 for all M tiles; per (chunk, tap) and M
// tile it reads two ds_read_b128 (hi, lo) for three MFMAs, two tiles ahead of their use.  B fragments (the pre-split weights, 576 KB,
// L2 resident, stored in fragment order so that a wave's load is 1 KB contiguous) stream straight into a 3-deep
// register ring two taps ahead; the next chunk's strip is loaded at the chunk's first tap, split and written to the
// other LDS buffer in the chunk's last MFMA regions; one block barrier per chunk.  Epilogue: accumulators -> LDS
// (64 rows at a time, double-buffered), read back as float4 rows, * scale + shift + residual, ReLU, whole 512-byte
// pixel rows written; the residual loads of the next 64 rows are in flight meanwhile.  In the tower's last layer the
// epilogue also reduces the head's 1x1 convolution per pixel and skips the layer output.  Workgroups map to (image,
// part) XCD-aware: the parts of an image, which share halo rows, run on the same XCD (same L2) back to back.
// The block body (hs_block) has two callers: k_conv3x3_f16s (whole images) and k_conv3x3_f16s_rect (the part of an image
// that depends on the state: the first tower layers of the self-play path, see the comment above that kernel).
#include "common.h"
#include "train_fold.h"
#include <stdlib.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned uint4_t __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

// the 16-bit activation type of the reduced-precision towers is f16 or (BF) bf16; both travel through the kernel as 16-bit
// patterns typed _Float16 (staging copies them untouched), only the MFMA and these two conversions know the difference
template <bool BF> __device__ __forceinline__ float hs_from16(_Float16 v)
{
    if (BF) return (float)__builtin_bit_cast(__bf16, v);
    return (float)v;
}
template <bool BF> __device__ __forceinline__ _Float16 hs_to16(float v)
{
    if (BF) return __builtin_bit_cast(_Float16, (__bf16)v);            // v_cvt_pk_bf16_f32: round to nearest even, float32's range
    return (_Float16)__builtin_amdgcn_fmed3f(v, -65504.f, 65504.f);    // saturating: an f16 infinity would turn the next layer into NaNs
}

#define HS_C 128
#define HS_KC 16                                         // input channels per chunk = one MFMA k step
#define HS_LDP 80                                        // bytes per LDS pixel: [hi k0-15 | lo k0-15] + 16 (16 x odd: conflict-free b128)
#define HS_NPB 352                                       // pixels per LDS buffer
#define HS_NPB_PK 416                                    // the same in the packed sub-rectangle form (PK below): the block's LDS is the
                                                         //   epilogue's 67 584 bytes anyway, and two strips carry four halo rows
#define HS_MLD 132                                       // epilogue row (floats): 528 bytes = 16 x 33
#define HS_SMEM_STAGE (2 * HS_BUF16)                     // 65 536 bytes (split form: 2 x 352 x 80 = 56 320)
#define HS_SMEM_EPI (2 * 64 * HS_MLD * 4)                // 67 584 bytes
#ifdef HS_ONE_PER_CU      // development build only: a block alone on its compute unit (what does the co-resident block cost it?)
#define HS_SMEM (96 * 1024)
#else
#define HS_SMEM (HS_SMEM_EPI > HS_SMEM_STAGE ? HS_SMEM_EPI : HS_SMEM_STAGE)
#endif
#define HS_ROWMAP (256 * 8)                              // the packed form's row map behind the block's LDS: 8 bytes per GEMM row (2 x 69 632 <= 160 KB per CU)
#define HS_WS_ELEMS (9 * HS_C * HS_C * 2)                // f16 numbers in the split weight image; four floats follow it
#define HS_RING 3
#define HS_AHEAD 2
#ifndef HS_XLOAD_TAP
#define HS_XLOAD_TAP 0                                   // the tap at whose start the next chunk's pixel loads are issued (A/B: make variant EXTRA=-DHS_XLOAD_TAP=1)
#endif
#define HS_NST 5                                         // staging items per thread and chunk: 64 pixels x 4 float4 each
// the frame of the towers with 16-bit activations (IO16 bit 0; BASELINE configs[4]): a chunk is 32 input channels = two MFMA k
// steps, so the 80-byte LDS pixel holds [channels 0-15 | 16-31] where the split form keeps [hi | lo]: half the chunks, barriers and
// A-pipeline restarts per block, and a chunk's MFMAs (2 x 9 x NI) outlast the HBM latency of the next chunk's pixel loads even
// when the block has the SIMDs to itself (with 16-channel chunks a block's chunk loop was bound by that latency: 3.7 k cycles per
// chunk for 1.4 k of MFMA issue, profiles/r5_a16_stamps.log).  No lo parts: the same LDS bytes hold more pixels (8-tile blocks on a
// 37-pixel-wide canvas) and a staging item is one 16-byte load and one ds_write_b128.
#define HS_NST16 6                                       // 16-bit frame: staging items per thread and chunk (64 pixels x 4 pieces of 16 bytes each)
#define HS_BUF16 32768                                   // 16-bit frame: bytes per LDS buffer.  Its rows are pitched in BYTES:
//   80 W + 256 (whole images: the 256-byte gap holds the zero border on both sides) or 80 (w + 2) + 96 (sub-rectangles: real halo
//   columns), so that stepping from a row's last pixel to the next row's first moves the address by 336 bytes = 21 bank quads = 5
//   mod 16, exactly like a step inside a row: the sixteen lanes a ds_read_b128 serves together never share a bank quad.  (With
//   rows pitched W + 1 pixels a lane group that straddles a row end spans 17 slots and two lanes collide: 37 % of this frame's
//   LDS cycles were conflict cycles, profiles/r5_a16_sq_counters_before.json, and the LDS, which serves a fragment read per MFMA
//   here, is what the co-resident block's epilogue and prologue wait for.)
#define HS_GAP16_FULL 256
#define HS_GAP16_RECT 96
#ifndef HS_PRIO
#define HS_PRIO 3
#endif
#ifndef HS_RING16
#define HS_RING16 3                                      // 16-bit frame: B-fragment ring (A/B: make variant EXTRA="-DHS_RING16=4 -DHS_AHEAD16=3")
#define HS_AHEAD16 2
#endif

struct ConvHsArgs {
    const float *x;            // [n][Hd][Wd][128]
    const f16x8 *wS;           // [chunk 8][tap 9][wn 4][hi/lo][lane 64] x 8 f16
    const float *wscale_inv;   // tail of the weight image: {2^-k (weights), 2^k, activation scale s (a power of two), 1 / s,
                               //   int32 range flag (set by the kernel when an input was clamped), 3 words of padding}
    const float *scale, *shift;
    const float *res;          // or NULL
    float *out;                // or NULL when only the fused 1x1 head output is wanted
    const float *w1x1;         // optional fused head (alpha_nnet.py:49-50): h1[pixel] = relu(dot(out[pixel][:], w1x1) * s1 + b1)
    float *h1;                 // [n][Hd * Wd], written when w1x1 is given
    float s1, b1;
    int Hd, Wd, n_blk, tiles_base, tiles_rem, relu;      // block b of an image has tiles_base + (b < tiles_rem) M tiles
    int n_img_grouped;         // images (a multiple of 8) that use the XCD-aware block order
    const float *center;       // MODE 4 (training forward): per-channel centre of the batch-norm sums (or NULL = 0)
    float *stat_part;          // MODE 4: [gridDim.x][2][128] sums of (out - center) and (out - center)^2 over the block's pixels
    // sub-rectangle form (k_conv3x3_f16s_rect): one descriptor per block, written on the device by k_rect_plan
    const uint4 *desc;         // { image, y0 | x0 << 8 | h << 16 | w << 24, tile0 | ntile << 8 | part << 16 | parts << 24, bounding box }
    const int *n_desc;         // number of descriptors (blocks past it leave at once)
    const float *bg_out;       // or NULL; [Hd][Wd][128]: this layer's output on an all-background image, copied into every pixel
                               //   of the canvas outside the rectangle (the layer's readers are full layers)
    const float *bg_in;        // or NULL; the input's background image: x is valid on the bounding box grown by grow_in (cut to the
    const float *bg_res;       //   canvas) and stale outside, where the producing layer's constant is read instead; the same for res
    int grow_in, grow_res;
    // MODE 5 (training step, input gradient): the batch-norm backward sums of the layer whose output gradient this launch produces
    const float *g_y;          // that layer's pre-batch-norm output [n][Hd][Wd][128]
    const unsigned char *g_mask;   // its ReLU bits, one byte per quad of channels (csrc/train.hip)
    const float *g_inv;        // its 1 / sigma per channel (center = its batch mean)
    // MODE 6 / 7 (training step, a block's first layer whose batch norm + ReLU is never written out, see MODE 6 below): the
    // producer's batch-norm scale and shift per channel -- MODE 6 applies relu(x * aff_scale + aff_shift) to every staged input,
    // MODE 7 takes the ReLU decision of g_y from the same expression instead of from mask bytes
    const float *aff_scale, *aff_shift;
    float *amax_part;          // MODE 4 (optional): [gridDim.x][128] largest |out - center| per channel over the block's pixels
    const unsigned char *res_mask;     // MODE 8: ReLU bits (one byte per quad of channels) the shortcut rows are taken through
};

// The kernels' MODE (an int template parameter; described at length above hs_block), named for the host code:
enum HsMode : int {
    HS_MODE_ARGS = 0,              // every option of the epilogue read from the arguments at run time
    HS_MODE_RELU = 1,              // ReLU, no shortcut
    HS_MODE_RES_RELU = 2,          // ReLU + shortcut
    HS_MODE_HEAD = 3,              // ReLU + shortcut + the fused 1x1 head, no layer output
    HS_MODE_STATS = 4,             // training forward: the bare convolution + its batch-norm sums (+ maxima where amax_part is given)
    HS_MODE_IGRAD = 5,             // training input gradient (+ the shortcut's) + the layer below's backward sums, its ReLU from mask bytes
    HS_MODE_STATS_AFF = 6,         // STATS whose input goes through relu(x * aff_scale + aff_shift) on its way in
    HS_MODE_IGRAD_AFF = 7,         // IGRAD whose ReLU decision is recomputed from aff_scale / aff_shift; never a shortcut
    HS_MODE_IGRAD_MRES = 8,        // IGRAD whose shortcut gradient is taken through res_mask's bits
    HS_MODE_STATS_AFF_AMAX = 9,    // STATS_AFF + the per-channel maxima
    HS_MODE_IGRAD_MRES_AFF = 10,   // IGRAD_MRES whose ReLU decision for the sums is recomputed like IGRAD_AFF's
};

#ifdef HS_STAMPS       // development build only (tools/conv_stamps.py): s_memtime at the phase boundaries of every block
__device__ unsigned long long hs_stamp_buf[16384 * 8];
#define HS_STAMP(k) if (tid == 0 && blockIdx.x < 16384) hs_stamp_buf[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memtime();
#define HS_STAMP_REAL(k) if (tid == 0 && blockIdx.x < 16384) hs_stamp_buf[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime();
// where the block runs: HW_ID (hwreg 4: wave slot, SIMD, CU, SH, SE, workgroup slot) | XCC_ID (hwreg 20) << 32
#define HS_STAMP_HWID(k) if (tid == 0 && blockIdx.x < 16384) hs_stamp_buf[blockIdx.x * 8 + (k)] = \
        (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32;
// per-tap stamps of wave 0 of the first 2 048 blocks: [block][chunk 0..7][tap 0..8 + chunk end]
__device__ unsigned long long hs_tap_buf[2048 * 8 * 10];
#define HS_TSTAMP(c_, s_) if (tid == 0 && blockIdx.x < 2048 && (c_) < 8) hs_tap_buf[(blockIdx.x * 8 + (c_)) * 10 + (s_)] = __builtin_amdgcn_s_memtime();
extern "C" int snk_dbg_conv_tap_stamps(unsigned long long *h_out)
{
    SNK_CHECK_HIP(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(hs_tap_buf), sizeof(unsigned long long) * 2048 * 8 * 10));
    return 0;
}
extern "C" int snk_dbg_conv_stamps(unsigned long long *h_out, int n_blocks)
{
    SNK_CHECK_HIP(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(hs_stamp_buf), (size_t)n_blocks * 8 * sizeof(unsigned long long)));
    return 0;
}
#else
#define HS_STAMP(k)
#define HS_STAMP_REAL(k)
#define HS_STAMP_HWID(k)
#define HS_TSTAMP(c_, s_)
#endif

// NI: M tiles (of 32 GEMM rows) per block, <= 8.  MODE fixes the epilogue's options at compile time (no branches per row):
//   0 all read from the arguments; 1 ReLU, no residual; 2 ReLU + residual; 3 ReLU + residual + fused head, no layer output;
//   4 the training step's forward pass: the bare convolution (no scale / shift / ReLU / residual) plus the per-channel sums its
//     batch norm needs, taken from the values on their way out (one pass over the activation less per layer and step)
//   5 the training step's input gradient: the bare convolution (+ the shortcut's gradient as residual) = the gradient at the previous
//     layer's output, plus the two per-channel sums that layer's batch-norm backward needs -- sum(g), sum(g xhat), g = the gradient
//     where the layer's ReLU let the value through -- taken from the values on their way out (snk_bn_train_grad_sums_f64's pass saved)
//   6 MODE 4 whose INPUT is the previous layer's pre-batch-norm output: relu(x * aff_scale + aff_shift) -- that layer's batch norm
//     and ReLU, the very expression of k_bn_apply (csrc/train.hip) -- is applied to every value on its way into LDS, so the
//     activation between the two convolutions of a residual block is never written to HBM nor read back (a pass over two
//     462 MB tensors less per block and step); the zero border stays zero (it is the padding of the ACTIVATION)
//   7 MODE 5 for such a layer below: its ReLU decision is y * aff_scale + aff_shift > 0, recomputed from the g_y values the sums
//     read anyway (no mask bytes exist for it)
//   8 MODE 5 whose shortcut gradient is res WHERE res_mask's bit is set: res is then the gradient at the block's OUTPUT as the layer
//     above received it, res_mask that output's ReLU bits -- the batch-norm backward of the block's second layer no longer writes
//     the masked copy (462 MB per block) just for this epilogue to read it back.  out may be res itself (a thread reads the rows
//     it writes, and reads them first)
//   9 MODE 6 that also takes MODE 4's per-channel maxima (its own batch norm is deferred too: the layer above a deferred stem)
//  10 MODE 8 whose ReLU decision for the sums is recomputed like MODE 7's (the layer below is the deferred stem: no mask bytes)
#define hs_dpp(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, true))

// ---- MX-FP8 (the mxfp8 tower, SNK_CONV_ALGO=mxfp8): OCP e4m3fn codes with one E8M0 scale per block of 32 input channels --------
// The rule (kernel, tests/mxfp8_ref.py and DESIGN.md section 4 state the same one):
//   block    activations: channels 32j .. 32j + 31 of one pixel; weights: the same 32 input channels of one (output channel, tap)
//   amax     the largest |v| of the block in float32 (bf16 activations are exact there; weights come from the float32 values)
//   E        the smallest integer with amax * 2^-E <= 448, clamped to [-127, 127]; amax == 0 gives E = -127 (all codes zero);
//            the scale byte is E + 127
//   code     e4m3fn round-to-nearest-even of v * 2^-E, subnormals kept; by the choice of E nothing saturates
// With amax = m 2^e (1 <= m < 2): E = e - 8 when m <= 1.75 (m 2^8 <= 448 < m 2^9), else e - 7 -- read off amax's float bits.
__device__ __forceinline__ unsigned mx_scale_byte(float amax)
{
    const unsigned b = __builtin_bit_cast(unsigned, amax);                  // amax >= 0: exponent field = b >> 23
    const int s = (int)(b >> 23) - 8 + ((b & 0x7FFFFFu) > 0x600000u ? 1 : 0);  // E + 127; a float32 subnormal or zero clamps to 0
    return (unsigned)max(s, 0);
}
// 2^-E as a float32 (E <= 120 for any finite amax: a normal number)
__device__ __forceinline__ float mx_inv_scale(unsigned sbyte) { return __builtin_bit_cast(float, (254u - sbyte) << 23); }
// four values (already multiplied by 2^-E, exact: a power-of-two product) -> four e4m3fn codes, RNE (the converter's scale is 1)
__device__ __forceinline__ unsigned mx_pack4(float a, float b, float c, float d)
{
    s16x2 w = {0, 0};
    w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, a, b, 1.0f, false);
    w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, c, d, 1.0f, true);
    return __builtin_bit_cast(unsigned, w);
}
// The staging path's quantizer: eight bf16 channels (bit patterns) of one lane -> eight codes (bytes 0..7) and the block's scale
// byte.  The block is this lane's quad (lanes 4q .. 4q + 3 hold its channels 8i .. 8i + 7): amax over the quad by two DPP steps,
// so every lane of the wave must run it.  k_mxfp8_quantize runs the same function on a plain bf16 array.
__device__ __forceinline__ uint2 mx_quant8(const f16x8 v, unsigned &sbyte)
{
    const uint4 u = __builtin_bit_cast(uint4, v);          // bf16 -> float32 by bits (exact): the pair (lo, hi) of each dword
    const float f[8] = {__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xFFFF0000u),
                        __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xFFFF0000u),
                        __builtin_bit_cast(float, u.z << 16), __builtin_bit_cast(float, u.z & 0xFFFF0000u),
                        __builtin_bit_cast(float, u.w << 16), __builtin_bit_cast(float, u.w & 0xFFFF0000u)};
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(f[j]));
    m = fmaxf(m, hs_dpp(m, 0xB1));                        // quad_perm [1, 0, 3, 2]
    m = fmaxf(m, hs_dpp(m, 0x4E));                        // quad_perm [2, 3, 0, 1]
    sbyte = mx_scale_byte(m);
    const float k = mx_inv_scale(sbyte);
    return make_uint2(mx_pack4(f[0] * k, f[1] * k, f[2] * k, f[3] * k), mx_pack4(f[4] * k, f[5] * k, f[6] * k, f[7] * k));
}
// SPLIT = false: the reduced-precision form for BASELINE configs[4] ("bf16 MFMA conv"): the same kernel with the hi parts
//   only, one MFMA per product instead of three (f16 operands: 11 significand bits against bf16's 8, float32 accumulate).
// IO16 (reduced-precision form only): bit 0 = the input and the residual are f16 arrays [n][H][W][128], bit 1 = the output
//   is written as f16.  The activations of BASELINE configs[4]'s tower then cost 2 bytes in HBM instead of 4 (the f16 form
//   with float32 activations is HBM-bound), staging is a plain copy (the values are f16 already: no scale, no clamp, no
//   conversion) and the range guard has nothing to watch.
// RECT: the block's "image" is a sub-rectangle (ry0, rx0, rh, rw) of the Hd x Wd canvas (see k_rect_plan below): GEMM rows are
//   the rectangle's pixels in row-major order, the LDS rows are pitched rw + 2 with the halo columns taken from the canvas
//   (zero outside it), global rows stay pitched Wd.
// BF (with IO16 bit 0, reduced-precision form only): the 16-bit type is bf16 -- BASELINE configs[4]'s "bf16 MFMA conv" as it is
//   worded: bf16 activations in HBM, bf16 weights, v_mfma_f32_32x32x16_bf16, float32 accumulation and epilogue.  bf16 has
//   float32's exponent range, so there is no scale to choose and nothing to clamp.
// MX (with BF): the mxfp8 tower -- bf16 activations in HBM as in the bf16 form, but a chunk is 64 input channels (one K step of
//   v_mfma_scale_f32_32x32x64_f8f6f4) quantized at staging time by the rule above: the 80-byte LDS pixel holds [codes of block 0
//   (32 bytes) | codes of block 1 | scale byte 0, scale byte 1 | 14 unused], so the frame's geometry (pitches, pixels per buffer,
//   384 staged pixels per chunk) and with it the rectangle plan are the 16-bit frame's.  The MFMA takes bytes 16 b .. 16 b + 15 of
//   both lane halves as k-block b and the scale of (row r, block b) from lane (b, r) (measured with exact integer data,
//   tests/test_mxfp8_gpu.py): lane (h, r) reads channels 16 h .. 16 h + 15 of each block of pixel r -- the 16-bit frame's two
//   ds_read_b128 at +16 h and +32 + 16 h -- and the scale byte of block h; B likewise from k_mxfp8_weights' image.  Per (tile,
//   tap) the bf16 form issues 2 MFMAs of 32 cycles in each of 4 chunks, this form 1 MFMA of 64 cycles in each of 2 chunks: a
//   quarter of the MFMAs, half the MFMA time, half the chunks and barriers.
// PK (with RECT, float32-accurate form only): the PACKED sub-rectangle form (k_rect_plan_pack below).  The images of a launch
//   whose rectangles have the same shape share one GEMM row space, so a block's rows are up to TWO segments: pixels tile0 ..
//   tile0 + ntile - 1 of image img's rectangle (here tile0 / ntile count ROWS, and the segment may start anywhere), then pixels
//   0 .. nB - 1 of image imgB's rectangle (same shape, its own position ryB / rxB and bounding box).  Each segment has its own
//   strip in LDS (A's rows first, B's behind them, same pitch); only the address set-up knows about segments -- the staging
//   items, the lanes' pixel addresses, the epilogue's row map, the shortcut / background choice and the fill -- the chunk loop
//   is the unpacked form's, and every GEMM row accumulates the same (chunk, tap, k) sequence whichever tile it sits in.
template <int NI, int MODE, bool SPLIT, int IO16, bool RECT, bool BF = false, bool MX = false, bool PK = false>
__device__ __forceinline__ void hs_block(const ConvHsArgs &p, unsigned char *smem, const int img, const int tile0, const int ntile,
                                         const int ry0, const int rx0, const int rh, const int rw, const unsigned bbox,
                                         const int part, const int parts, const int imgB = 0, const int ryB = 0, const int rxB = 0,
                                         const unsigned bboxB = 0u, const int nB = 0)
{
    static_assert(!PK || (RECT && SPLIT && IO16 == 0 && (MODE == 1 || MODE == 2)), "the packed form exists for the float32-accurate sub-rectangle layers only");
    static_assert(IO16 == 0 || !SPLIT, "f16 activations only exist in the reduced-precision form");
    static_assert(!BF || (IO16 & 1), "the bf16 form reads bf16 activations");
    static_assert(!MX || BF, "the mxfp8 form reads bf16 activations");
    constexpr bool IN16 = (IO16 & 1) != 0, OUT16 = (IO16 & 2) != 0;
    constexpr bool STATS = MODE == 4 || MODE == 6 || MODE == 9, GSTATS = MODE == 5 || MODE == 7 || MODE == 8 || MODE == 10, BARE = STATS || GSTATS;
    constexpr bool RESMASK = MODE == 8 || MODE == 10, AMAX = MODE == 4 || MODE == 9;
    constexpr bool AFF = MODE == 6 || MODE == 9, GAFF = MODE == 7 || MODE == 10, NORES = MODE == 7;
    static_assert(!(AFF || GAFF || RESMASK) || (IO16 == 0 && !RECT), "the deferred batch norm exists in the training step's forms (float32 tensors, whole images) only");
    constexpr bool K32 = IN16;
    constexpr int RING = K32 ? HS_RING16 : HS_RING, AHEAD = K32 ? HS_AHEAD16 : HS_AHEAD;      // B-fragment register ring: slots (a divisor of 9), taps ahead
    constexpr bool TWO = SPLIT || K32;                     // two A fragments / two B fragments per (tap, M tile)
    constexpr int KC = MX ? 64 : K32 ? 32 : HS_KC, NCHUNK = HS_C / KC;
    constexpr int NST = K32 ? HS_NST16 : HS_NST, BUFB = K32 ? HS_BUF16 : (PK ? HS_NPB_PK : HS_NPB) * HS_LDP;
    constexpr int PIECE = K32 ? 8 : 4;                     // channels of a staging item
    // MX: a 64-channel chunk is staged in two halves of 32 channels (one MX block per pixel each) with the 16-bit frame's items --
    // half 0 loaded at tap 0 and written from region MXR0 on, half 1 loaded at the start of tap MXT1 into the same registers and
    // written in the chunk's last 2 NST regions (twelve items in flight at once spill the 8-tile bodies)
    // (half 0 is written from region MXR0 on: not before the region whose tap issued its loads, HS_XLOAD_TAP)
    constexpr int MXR0_ = 9 * NI > 4 * NST ? (9 * NI - 4 * NST) / 2 : 0;
    constexpr int MXR0 = MXR0_ > HS_XLOAD_TAP * NI ? MXR0_ : HS_XLOAD_TAP * NI, MXT1 = (MXR0 + 2 * NST + NI - 1) / NI;
    constexpr int MXR1 = 9 * NI - 2 * NST > MXT1 * NI ? 9 * NI - 2 * NST : MXT1 * NI;
    constexpr bool MXIN = MX && 9 * NI >= 4 * NST && MXT1 <= 8 && MXR1 + 2 * NST <= 9 * NI;     // else both halves at the chunk's end
    static_assert(!MXIN || (MXR0 >= HS_XLOAD_TAP * NI && MXR0 + 2 * NST <= MXT1 * NI), "MX staging: a half is written before it is loaded");
    constexpr bool P8 = IN16 && OUT16;                     // the epilogue handles 8 channels (16 bytes in and out) per thread and row
    // (MODE 7 never takes a shortcut's gradient: it produces the gradient at a block's FIRST layer's output -- its epilogue has the
    // registers the shortcut rows would take for the g_y rows instead, requested a pass ahead)
    const bool has_res = NORES ? false : RESMASK ? true : (MODE == 0 || GSTATS) ? p.res != nullptr : (MODE == 2 || MODE == 3);
    const bool has_head = MODE == 0 ? p.w1x1 != nullptr : MODE == 3;
    const bool has_out = MODE == 0 ? p.out != nullptr : MODE != 3;
    const float relu_floor = ((MODE != 0 && !BARE) || (MODE == 0 && p.relu)) ? 0.f : -__builtin_inff();
    (void)has_head; (void)has_out; (void)relu_floor;       // (the input-gradient epilogue uses none of them)
    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;        // wave wn owns outputs 32 wn .. 32 wn + 31
    const int h = lane >> 5, l31 = lane & 31;
    const int Wr = RECT ? rw : p.Wd;                       // width of the GEMM's image
    const int cy0 = RECT ? ry0 : 0, cx0 = RECT ? rx0 : 0;  // its origin on the canvas
    const int HW = RECT ? rh * rw : p.Hd * p.Wd;           // its pixels = GEMM rows
    const int HWc = p.Hd * p.Wd;                           // the canvas: what the tensors in HBM are pitched by
    const int m0 = PK ? tile0 : 32 * tile0, m1 = PK ? tile0 + ntile : min(32 * (tile0 + ntile), HW);   // the block's GEMM rows = pixels m0 .. m1 - 1 of the image (PK: its first segment's)
    const int P = RECT ? Wr + 2 : Wr + 1;                  // padded pitch (pixels)
    const int PB = K32 ? (RECT ? (Wr + 2) * HS_LDP + HS_GAP16_RECT : Wr * HS_LDP + HS_GAP16_FULL) : P * HS_LDP;   // LDS row pitch (bytes)
    const float invW = 1.0f / (float)Wr;
    const int y_first = (int)(((float)m0 + 0.5f) * invW), y_last = (int)(((float)(m1 - 1) + 0.5f) * invW);
    // LDS row r holds image row y_first - 1 + r (zero when outside the canvas), LDS column x + 1 image column x

    // ---- staging role: item k of this thread = pixel (tid / 4 + 64 k) of the strip (the rows and columns of the canvas the
    //      block's taps reach), float4 (tid % 4) of the chunk
    const int ya = max(cy0 + y_first - 1, 0), yb = min(cy0 + y_last + 1, p.Hd - 1);          // canvas rows of the strip
    const int xa = RECT ? max(cx0 - 1, 0) : 0, xb = RECT ? min(cx0 + Wr, p.Wd - 1) : p.Wd - 1;   // its canvas columns
    const int ry_lo = ya - (cy0 + y_first - 1), cx_lo = RECT ? xa - (cx0 - 1) : 1;             // LDS row / column of (ya, xa)
    const int ws = xb - xa + 1;
    const int npx = (yb - ya + 1) * ws;
    const float invWs = RECT ? 1.0f / (float)ws : invW;
    const float *xrow = p.x + (((long)img * p.Hd + ya) * p.Wd + xa) * HS_C + PIECE * (tid & 3);
    const _Float16 *xrow16 = (const _Float16 *)p.x + (((long)img * p.Hd + ya) * p.Wd + xa) * HS_C + PIECE * (tid & 3);
    const int pix0 = tid >> 2;
    const float xs = p.wscale_inv[2];                      // activations are multiplied by this power of two before the split
    unsigned ldo[NST];                                     // LDS byte offset (inside a buffer) of the thread's items
    unsigned gof[NST];                                     // element offset of the items in x (chunk 0)
    const float *gp[NST];                                  // RECT: the items' addresses (chunk 0): in x where the producing layer wrote
    const _Float16 *gp16[NST];                             //   (bounding box grown by grow_in), else in that layer's background image
    const int by0 = bbox & 255, bx0 = (bbox >> 8) & 255, by1 = (bbox >> 16) & 255, bx1 = bbox >> 24;
    const bool sel_in = RECT && p.bg_in != nullptr;
    (void)imgB; (void)ryB; (void)rxB; (void)bboxB; (void)nB;
    // PK: the second segment's strip (image rows -1 .. its last row + 1) sits behind the first one's RA rows
    const int nA = m1 - m0, RA = y_last - y_first + 3;
    const int yB_last = (int)(((float)max(nB - 1, 0) + 0.5f) * invW);
    const int yaB = max(ryB - 1, 0), ybB = min(ryB + yB_last + 1, p.Hd - 1), xaB = max(rxB - 1, 0), xbB = min(rxB + Wr, p.Wd - 1);
    const int ry_loB = RA + yaB - (ryB - 1), cx_loB = xaB - (rxB - 1), wsB = xbB - xaB + 1, npxB = nB > 0 ? (ybB - yaB + 1) * wsB : 0;
    const int byB0 = bboxB & 255, bxB0 = (bboxB >> 8) & 255, byB1 = (bboxB >> 16) & 255, bxB1 = bboxB >> 24;
    (void)nA; (void)RA; (void)ry_loB; (void)cx_loB; (void)npxB; (void)byB0; (void)bxB0; (void)byB1; (void)bxB1;
    // PK: the epilogue's row map, once per block instead of once per lane: thread r writes the entry of GEMM row r behind the
    // block's staging / exchange LDS (the chunk loop's barriers stand between this and the epilogue's reads) --
    //   .x  the row's element offset in the tensors, its image included; -1 past the block's pixels
    //   .y  where its shortcut value is: .x when the shortcut's producer computed the pixel (bounding box grown by grow_res), else
    //       the pixel's offset in that producer's background image with bit 31 set; 0 past the block's pixels (read, never used)
    if constexpr (PK) {
        const int r_ = tid;
        const bool sb_ = r_ >= nA;                         // row -> (segment, pixel) -> address in the segment's image
        const int mm_ = sb_ ? r_ - nA : m0 + r_;
        const int y_ = (int)(((float)mm_ + 0.5f) * invW), x_ = mm_ - y_ * Wr;
        const int Y_ = (sb_ ? ryB : cy0) + y_, X_ = (sb_ ? rxB : cx0) + x_;
        const bool in_ = r_ < nA + nB;
        const int o_ = (((sb_ ? imgB : img) * p.Hd + Y_) * p.Wd + X_) * HS_C;
        const bool stale_ = MODE == 2 && p.bg_res != nullptr &&
                            (Y_ < (sb_ ? byB0 : by0) - p.grow_res || Y_ > (sb_ ? byB1 : by1) + p.grow_res ||
                             X_ < (sb_ ? bxB0 : bx0) - p.grow_res || X_ > (sb_ ? bxB1 : bx1) + p.grow_res);
        *(int2 *)(smem + HS_SMEM + 8 * r_) = make_int2(in_ ? o_ : -1, !in_ ? 0 : stale_ ? (int)(((unsigned)(Y_ * p.Wd + X_) * HS_C) | 0x80000000u) : o_);
    }
    // items past the strip's last pixel repeat it (same value to the same LDS address): no predication, no branches
    if constexpr (PK) {
        const float invWsB = 1.0f / (float)wsB;
#pragma unroll
        for (int k = 0; k < NST; ++k) {
            const int pq_ = pix0 + 64 * k;
            const bool sb_ = npxB > 0 && pq_ >= npx;          // the item belongs to the second strip
            const int pix_ = sb_ ? min(pq_ - npx, npxB - 1) : min(pq_, npx - 1);
            const int w_ = sb_ ? wsB : ws;
            const int r_ = (int)(((float)pix_ + 0.5f) * (sb_ ? invWsB : invWs)), x_ = pix_ - r_ * w_;
            ldo[k] = ((sb_ ? ry_loB : ry_lo) + r_) * PB + ((sb_ ? cx_loB : cx_lo) + x_) * HS_LDP + (tid & 3) * 8;
            gof[k] = 0u;
            const int Y = (sb_ ? yaB : ya) + r_, X = (sb_ ? xaB : xa) + x_;
            const int y0_ = sb_ ? byB0 : by0, x0_ = sb_ ? bxB0 : bx0, y1_ = sb_ ? byB1 : by1, x1_ = sb_ ? bxB1 : bx1;
            const bool stale = sel_in && (Y < y0_ - p.grow_in || Y > y1_ + p.grow_in || X < x0_ - p.grow_in || X > x1_ + p.grow_in);
            const long o_ = (long)(Y * p.Wd + X) * HS_C + PIECE * (tid & 3);
            gp[k] = (stale ? p.bg_in : p.x + (long)(sb_ ? imgB : img) * HWc * HS_C) + o_;
            gp16[k] = nullptr;
        }
    } else
#pragma unroll
    for (int k = 0; k < NST; ++k) {
        const int pix_ = min(pix0 + 64 * k, npx - 1);
        const int r_ = (int)(((float)pix_ + 0.5f) * invWs), x_ = pix_ - r_ * ws;
        ldo[k] = (ry_lo + r_) * PB + (cx_lo + x_) * HS_LDP + (tid & 3) * (MX ? 8 : K32 ? 16 : 8);     // (MX: the piece's 8 codes in half 0)
        gof[k] = (r_ * p.Wd + x_) * HS_C;
        if (RECT) {
            const int Y = ya + r_, X = xa + x_;
            const bool stale = sel_in && (Y < by0 - p.grow_in || Y > by1 + p.grow_in || X < bx0 - p.grow_in || X > bx1 + p.grow_in);
            const long o_ = (long)(Y * p.Wd + X) * HS_C + PIECE * (tid & 3);
            gp[k] = (stale ? p.bg_in : p.x + (long)img * HWc * HS_C) + o_;
            gp16[k] = (stale ? (const _Float16 *)p.bg_in : (const _Float16 *)p.x + (long)img * HWc * HS_C) + o_;
        }
    }
    float4 st[K32 ? 1 : NST];
    f16x4 st16[K32 ? 1 : NST];
    f16x8 st8[K32 ? NST : 1];                              // the 16-bit frame's items: eight channels, staged as they are
    f16x8 st8b[MX ? NST : 1];                              // MX: half 1 of the first chunk, and of every chunk in the 1-2 tile bodies
    uint2 mq_t = make_uint2(0u, 0u);                       // MX: an item's eight codes and its block's scale byte (split half A -> B)
    unsigned ms_t = 0u;
    const unsigned ms_off = 64 - 8 * (tid & 3);            // MX: from an item's codes (half 0) to the pixel's scale byte of half 0
    f16x4 hi_t;
    float4 d_t;
    float4 asc = make_float4(1.f, 1.f, 1.f, 1.f), ash = make_float4(0.f, 0.f, 0.f, 0.f);    // MODE 6: the producer's scale / shift of the
    //   four channels this thread stages in the chunk being split; all 128 of each sit in LDS behind the two staging buffers
#define HS_AFF_READ(c) { asc = *(const float4 *)(smem + 2 * BUFB + (16 * (c) + 4 * (tid & 3)) * 4);      \
                         ash = *(const float4 *)(smem + 2 * BUFB + 512 + (16 * (c) + 4 * (tid & 3)) * 4); }
    float amax = 0.f;                                      // largest |scaled input| this thread staged: 65504 = something was clamped
#define HS_LOAD(c) _Pragma("unroll") for (int k_ = 0; k_ < NST; ++k_) {                         \
        if (K32) st8[k_] = *(const f16x8 *)((RECT ? gp16[k_] : xrow16 + gof[k_]) + KC * (c));   \
        else if (IN16) st16[k_] = *(const f16x4 *)((RECT ? gp16[k_] : xrow16 + gof[k_]) + KC * (c)); \
        else st[k_] = *(const float4 *)((RECT ? gp[k_] : xrow + gof[k_]) + KC * (c)); }
// MX: half 1 (channels 32-63) of chunk c
#define HS_LOAD_H1(dst, c) _Pragma("unroll") for (int k_ = 0; k_ < NST; ++k_)                  \
        dst[k_] = *(const f16x8 *)((RECT ? gp16[k_] : xrow16 + gof[k_]) + KC * (c) + 32);
// split of one staged float4 in two halves that sit in different MFMA regions (a region hides about 15 VALU instructions):
//   A: clamp to the f16 range, hi = f16(v), d = v - hi;   B: lo = f16(d), both written to LDS
#define HS_SPLIT_A(kk)                                                                          \
    if (MX) { mq_t = mx_quant8(st8[kk], ms_t); } else                                           \
    if (K32) { } else if (IN16) { hi_t = st16[kk]; } else                                       \
    {                                                                                           \
        float4 v_ = st[kk];                                                                     \
        if (AFF) {          /* the producer's batch norm + ReLU, as k_bn_apply computes it (multiply, then add: no fma) */ \
            v_.x = fmaxf(v_.x * asc.x + ash.x, 0.f); v_.y = fmaxf(v_.y * asc.y + ash.y, 0.f);   \
            v_.z = fmaxf(v_.z * asc.z + ash.z, 0.f); v_.w = fmaxf(v_.w * asc.w + ash.w, 0.f);   \
        }                                                                                       \
        v_.x *= xs; v_.y *= xs; v_.z *= xs; v_.w *= xs;                                         \
        v_.x = __builtin_amdgcn_fmed3f(v_.x, -65504.f, 65504.f); v_.y = __builtin_amdgcn_fmed3f(v_.y, -65504.f, 65504.f); \
        v_.z = __builtin_amdgcn_fmed3f(v_.z, -65504.f, 65504.f); v_.w = __builtin_amdgcn_fmed3f(v_.w, -65504.f, 65504.f); \
        amax = fmaxf(fmaxf(amax, fabsf(v_.x)), fabsf(v_.y)); amax = fmaxf(fmaxf(amax, fabsf(v_.z)), fabsf(v_.w)); /* 2 v_max3 */ \
        hi_t[0] = (_Float16)v_.x; hi_t[1] = (_Float16)v_.y; hi_t[2] = (_Float16)v_.z; hi_t[3] = (_Float16)v_.w; \
        if (SPLIT) {                                                                            \
            d_t.x = v_.x - (float)hi_t[0]; d_t.y = v_.y - (float)hi_t[1];                       \
            d_t.z = v_.z - (float)hi_t[2]; d_t.w = v_.w - (float)hi_t[3];                       \
        }                                                                                       \
    }
// MX: an item's codes and its block's scale byte into half hf_ of the pixel (the quad's four lanes write the same byte)
#define HS_MXB(k_, bufoff, hf_)                                                                 \
    {                                                                                           \
        *(uint2 *)(smem + (bufoff) + ldo[k_] + 32 * (hf_)) = mq_t;                              \
        smem[(bufoff) + ldo[k_] + ms_off + (hf_)] = (unsigned char)ms_t;                        \
    }
#define HS_SPLIT_B(k_, bufoff)                                                                  \
    if (MX) { HS_MXB(k_, bufoff, 0) } else                                                      \
    if (K32) { *(f16x8 *)(smem + (bufoff) + ldo[k_]) = st8[k_]; } else                          \
    {                                                                                           \
        unsigned char *d_ = smem + (bufoff) + ldo[k_];                                          \
        *(f16x4 *)d_ = hi_t;                                                                    \
        if (SPLIT) {                                                                            \
            f16x4 lo_;                                                                          \
            lo_[0] = (_Float16)d_t.x; lo_[1] = (_Float16)d_t.y; lo_[2] = (_Float16)d_t.z; lo_[3] = (_Float16)d_t.w; \
            *(f16x4 *)(d_ + 32) = lo_;                                                          \
        }                                                                                       \
    }

    HS_STAMP(0)
    HS_STAMP_HWID(7)
    const f16x8 *wl = p.wS + wn * 128 + lane;              // this wave's fragments of global step g = 9 chunk + tap: wl[g * 512 + {0 hi, 64 lo}]
    f16x8 Bq[RING][2];
    // MX: the image's codes are [step 18][wn 4][half 2][lane 64] x 16 bytes (the same strides), its scale bytes [step 18][wn 4][lane 64] behind them
    const unsigned char *wsb = (const unsigned char *)p.wS + 9 * HS_C * HS_C + wn * 64 + lane;
    unsigned Bs[RING];
#define HS_LOADB(slot, g)                                                                       \
    {                                                                                           \
        const f16x8 *w_ = wl + (long)(g) * 512;                                                 \
        Bq[slot][0] = w_[0];                                                                    \
        if (TWO) Bq[slot][1] = w_[64];                                                          \
        if (MX) Bs[slot] = wsb[(g) * 256];                                                      \
    }
    HS_LOAD(0)
    if (MX) { HS_LOAD_H1(st8b, 0) }
#pragma unroll
    for (int s = 0; s < AHEAD; ++s) HS_LOADB(s, s);
    if (K32) {
        // the 16-bit frame zeroes only what is read and never staged (both buffers): per LDS row the left border / halo slot and the
        // 176 bytes from slot Wr + 1 to the end of the row (the right border; a halo column inside the canvas is staged over it
        // after the barrier), and the rows above / below the canvas -- 4-6 stores per thread instead of 16
        const int R = y_last - y_first + 3;
        for (int i = tid; i < 2 * 16 * R; i += 256) {
            const int b = i >= 16 * R, j = i - b * 16 * R, r = j >> 4, q = j & 15;
            *(uint4 *)(smem + b * BUFB + r * PB + (q < 5 ? q * 16 : (Wr + 1) * HS_LDP + (q - 5) * 16)) = make_uint4(0u, 0u, 0u, 0u);
        }
        const bool top = ry_lo > 0, bot = cy0 + y_last + 1 > p.Hd - 1;
        if (top || bot)
            for (int i = tid; i < 2 * (PB >> 4); i += 256) {
                const int b = i >= (PB >> 4), q = i - b * (PB >> 4);
                if (top) *(uint4 *)(smem + b * BUFB + q * 16) = make_uint4(0u, 0u, 0u, 0u);
                if (bot) *(uint4 *)(smem + b * BUFB + (R - 1) * PB + q * 16) = make_uint4(0u, 0u, 0u, 0u);
            }
    } else
    for (int o = tid * 16; o < 2 * BUFB; o += 256 * 16) *(uint4 *)(smem + o) = make_uint4(0u, 0u, 0u, 0u);   // borders stay zero
    if (AFF && tid < 64) *(float4 *)(smem + 2 * BUFB + 16 * tid) = *(const float4 *)((tid < 32 ? p.aff_scale : p.aff_shift - HS_C) + 4 * tid);
    f32x16 acc[NI];
#pragma unroll
    for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    __syncthreads();
    if (AFF) HS_AFF_READ(0)
#pragma unroll
    for (int k = 0; k < NST; ++k) { HS_SPLIT_A(k) HS_SPLIT_B(k, 0) }
    if (MX) {
#pragma unroll
        for (int k = 0; k < NST; ++k) { mq_t = mx_quant8(st8b[k], ms_t); HS_MXB(k, 0, 1) }
    }
    __syncthreads();

    unsigned la[NI];                                       // LDS byte address (buffer 0, centre tap) of the lane's pixel in M tile i
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if constexpr (PK) {                                // rows past the block's last pixel repeat it
            const int r_ = 32 * i + l31;
            const bool sb_ = nB > 0 && r_ >= nA;
            const int m_ = sb_ ? min(r_ - nA, nB - 1) : min(m0 + r_, m1 - 1);
            const int y_ = (int)(((float)m_ + 0.5f) * invW), x_ = m_ - y_ * Wr;
            la[i] = (unsigned)((sb_ ? RA + y_ + 1 : y_ - (y_first - 1)) * PB + (x_ + 1) * HS_LDP) + 16 * h;
            continue;
        }
        const int m_ = min(m0 + 32 * i + l31, HW - 1);     // rows past the image repeat its last pixel (computed, never stored)
        const int y_ = (int)(((float)m_ + 0.5f) * invW), x_ = m_ - y_ * Wr;
        la[i] = (unsigned)((y_ - (y_first - 1)) * PB + (x_ + 1) * HS_LDP) + 16 * h;
    }
    const unsigned as_off = 64 - 15 * h;                   // MX: from the lane's first codes to the scale byte of block h of the pixel
#define HS_LDS(off) (*(const f16x8 *)(smem + (off)))
#define HS_MFMA(a, b, c) c = BF ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0) \
                              : __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)
// MX: A = 32 codes (two 16-byte halves) with the lane's scale byte, B the same; format 0 (e4m3) for both, scales in byte 0
#define HS_MFMA_MX(ah, al, as, bh, bl, bs, c) c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(                           \
        __builtin_shufflevector(__builtin_bit_cast(i32x4, ah), __builtin_bit_cast(i32x4, al), 0, 1, 2, 3, 4, 5, 6, 7),          \
        __builtin_shufflevector(__builtin_bit_cast(i32x4, bh), __builtin_bit_cast(i32x4, bl), 0, 1, 2, 3, 4, 5, 6, 7),          \
        c, 0, 0, 0, (int)(as), 0, (int)(bs))
// One tap of a chunk = NI fenced regions, each = { the ds_reads of the tile two ahead; a share of the staging work;
// this tile's three MFMAs }.  The fences keep the A fragments two tiles ahead of their use (the compiler otherwise
// sinks the reads to the MFMAs that consume them and the wave eats the LDS latency once per tile).  The tile sequence
// runs across taps: tile t of the chunk is (tap t / NI, M tile t % NI).  Staging of the next chunk: HS_NST global
// loads at tap 0, their split halves (A, B) in the chunk's last 2 HS_NST regions.
#define HS_AOFF(t) (la[(t) % NI] + rb + (unsigned)((((t) / NI) / 3 - 1) * PB + (((t) / NI) % 3 - 1) * HS_LDP))
#define HS_TAP(s, MORE)                                                                         \
        {                                                                                       \
            _Pragma("unroll") for (int i = 0; i < NI; ++i) {                                    \
                const int t2_ = (s) * NI + i + 2;                                               \
                f16x8 nh = a1h, nl = a1l;                                                       \
                unsigned ns = a1s;                                                              \
                if (t2_ < 9 * NI) {                                                             \
                    nh = HS_LDS(HS_AOFF(t2_)); if (TWO) nl = HS_LDS(HS_AOFF(t2_) + 32);         \
                    if (MX) ns = smem[HS_AOFF(t2_) + as_off];                                   \
                }                                                                               \
                __builtin_amdgcn_sched_barrier(0);                                              \
                if (i == 0) {                                                                   \
                    HS_TSTAMP(c, (s))                                                           \
                    if (MORE || (s) + AHEAD < 9) { HS_LOADB(((s) + AHEAD) % RING, gnext + (s)); } \
                    if ((s) == HS_XLOAD_TAP && MORE) { HS_LOAD(c + 1) }                         \
                    if (MXIN && MORE && (s) == MXT1) { HS_LOAD_H1(st8, c + 1) }                 \
                    if (MX && !MXIN && MORE && (s) == HS_XLOAD_TAP) { HS_LOAD_H1(st8b, c + 1) } \
                }                                                                               \
                if (MXIN && MORE) {                                                             \
                    const int u0_ = (s) * NI + i - MXR0, u1_ = (s) * NI + i - MXR1;             \
                    if (u0_ >= 0 && u0_ < 2 * NST) {                                            \
                        if ((u0_ & 1) == 0) { HS_SPLIT_A((u0_ < 0 ? 0 : min(u0_ >> 1, NST - 1))) }            \
                        else { HS_MXB((u0_ < 0 ? 0 : min(u0_ >> 1, NST - 1)), wb, 0) }                        \
                    }                                                                           \
                    if (u1_ >= 0 && u1_ < 2 * NST) {                                            \
                        if ((u1_ & 1) == 0) { HS_SPLIT_A((u1_ < 0 ? 0 : min(u1_ >> 1, NST - 1))) }            \
                        else { HS_MXB((u1_ < 0 ? 0 : min(u1_ >> 1, NST - 1)), wb, 1) }                        \
                    }                                                                           \
                }                                                                               \
                {                                                                               \
                    const int tl_ = (s) * NI + i - (9 * NI - 2 * NST);                          \
                    if (AFF && MORE && 9 * NI >= 2 * NST && tl_ == -1) HS_AFF_READ(c + 1)       \
                    if (!MX && MORE && 9 * NI >= 2 * NST && tl_ >= 0) {                         \
                        if ((tl_ & 1) == 0) { HS_SPLIT_A((tl_ < 0 ? 0 : tl_ >> 1)) }            \
                        else { HS_SPLIT_B((tl_ < 0 ? 0 : tl_ >> 1), wb) }                       \
                    }                                                                           \
                }                                                                               \
                if (MX) {                                /* the chunk's 64 channels in one MFMA */ \
                    HS_MFMA_MX(a0h, a0l, a0s, Bq[(s) % RING][0], Bq[(s) % RING][1], Bs[(s) % RING], acc[i]); \
                } else {                                                                        \
                HS_MFMA(a0h, Bq[(s) % RING][0], acc[i]);                                     \
                if (SPLIT) {                                                                    \
                    HS_MFMA(a0h, Bq[(s) % RING][1], acc[i]);                                 \
                    HS_MFMA(a0l, Bq[(s) % RING][0], acc[i]);                                 \
                } else if (K32) {                        /* the chunk's second k step: channels 16-31 */ \
                    HS_MFMA(a0l, Bq[(s) % RING][1], acc[i]);                                 \
                }                                                                               \
                }                                                                               \
                a0h = a1h; a0l = a1l; a1h = nh; a1l = nl; a0s = a1s; a1s = ns;                  \
                __builtin_amdgcn_sched_barrier(0);                                              \
            }                                                                                   \
        }
#define HS_CHUNK(MORE)                                                                          \
    {                                                                                           \
        const unsigned rb = (unsigned)(c & 1) * BUFB;                                           \
        const unsigned wb = (unsigned)((c & 1) ^ 1) * BUFB;                                     \
        const int gnext = c * 9 + AHEAD;             /* global step the first prefetch of this chunk fetches */ \
        f16x8 a0h = HS_LDS(HS_AOFF(0)), a1h = HS_LDS(HS_AOFF(1)), a0l = a0h, a1l = a1h;         \
        unsigned a0s = 0u, a1s = 0u;                                                            \
        if (TWO) { a0l = HS_LDS(HS_AOFF(0) + 32); a1l = HS_LDS(HS_AOFF(1) + 32); }              \
        if (MX) { a0s = smem[HS_AOFF(0) + as_off]; a1s = smem[HS_AOFF(1) + as_off]; }          \
        HS_TAP(0, MORE) HS_TAP(1, MORE) HS_TAP(2, MORE) HS_TAP(3, MORE) HS_TAP(4, MORE)         \
        HS_TAP(5, MORE) HS_TAP(6, MORE) HS_TAP(7, MORE) HS_TAP(8, MORE)                         \
        if (!MX && MORE && 9 * NI < 2 * NST) {          /* too few regions to spread the split over: do it here */ \
            if (AFF) HS_AFF_READ(c + 1)                                                         \
            _Pragma("unroll") for (int k = 0; k < NST; ++k) { HS_SPLIT_A(k) HS_SPLIT_B(k, wb) } \
        }                                                                                       \
        if (MX && MORE && !MXIN) {      /* MX, 1-2 tiles: both halves loaded at tap HS_XLOAD_TAP (registers to spare), written here */ \
            _Pragma("unroll") for (int k = 0; k < NST; ++k) { HS_SPLIT_A(k) HS_MXB(k, wb, 0) }  \
            _Pragma("unroll") for (int k = 0; k < NST; ++k) { mq_t = mx_quant8(st8b[k], ms_t); HS_MXB(k, wb, 1) } \
        }                                                                                       \
        __syncthreads();                                                                        \
    }
    int c = 0;
    HS_STAMP(1)
    // the chunk loop's waves go before the co-resident block's prologue / epilogue waves (16-bit frame: a third of the split form's
    // MFMAs per block, so a block's frame is 30 % of its life and what it costs the partner's matrix stream shows: +2.5-3 %, A/B
    // in one call, profiles/r5_a16_ab.log; the split form measured no gain in rounds 3-4)
    if (K32) __builtin_amdgcn_s_setprio(HS_PRIO);
    HS_STAMP_REAL(5)
#pragma unroll 1
    for (; c < NCHUNK - 1; ++c) HS_CHUNK(true)
    HS_STAMP(2)
    // MODE 7: the g_y rows of the epilogue's first pass are requested here, into the registers the staging items no longer need: their
    // HBM latency passes under the last chunk's MFMAs (the epilogue below requests every later pass's rows one pass ahead)
    float4 gyv[NORES ? 2 : 1][NORES ? 8 : 1];
    if (NORES) {
#pragma unroll
        for (int j = 0; j < (NI >= 2 ? 8 : 4); ++j) {
            const int m_ = min(m0 + (tid >> 5) + 8 * j, m1 - 1);
            gyv[0][j] = *(const float4 *)(p.g_y + (long)img * HWc * HS_C + 4 * (tid & 31) + (long)m_ * HS_C);
        }
    }
    HS_CHUNK(false)                    // the last chunk stages nothing
    HS_STAMP(3)
    if (K32) __builtin_amdgcn_s_setprio(0);
    // range guard: an input beyond the f16 range after scaling was clamped, the layer's result is then NOT float32-accurate.
    // The flag word sits behind the scales in the weight image (one per layer); the host reads it (QNet.check_range).
    // The same event is also stored to the device word tail[6..7] points to, when the caller registered one (ONE word for all
    // layers of a net, snk_conv3x3_f16s_set_guard_word): the kernels of a rollout tick that follow the evaluation are gated on it
    // (csrc/mcts.hip TICK_GATE), and the host learns from one word whether any launch of a forward clamped.
    if (amax >= 65504.f) {
        int *t = (int *)const_cast<float *>(p.wscale_inv);
        atomicOr(t + 4, 1);
        int *shared = *(int *const *)(t + 6);
        if (shared) __hip_atomic_store(shared, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    HS_STAMP_REAL(6)
#undef HS_TAP
#undef HS_CHUNK
#undef HS_AOFF
#undef HS_LOAD
#undef HS_SPLIT_A
#undef HS_SPLIT_B
#undef HS_MXB
#undef HS_LOAD_H1
#undef HS_LOADB
#undef HS_AFF_READ
#undef HS_LDS
#undef HS_MFMA
#undef HS_MFMA_MX

    // ---- epilogue: 64 GEMM rows (2 M tiles) at a time through a double-buffered LDS exchange, so that every thread
    //      handles float4 pieces of whole pixel rows: thread (rr0 = tid / 32, cq = tid % 32) takes rows rr0 + 8 j of the
    //      pass, outputs 4 cq .. 4 cq + 3.  The residual loads of pass k + 1 are issued before pass k is exchanged and
    //      stored; one block barrier per pass (the other block of the CU computes meanwhile).
    if constexpr (P8) {
        // ---- the 16-bit frame's epilogue: the same double-buffered exchange, but a thread takes EIGHT channels of a row (16 bytes of
        //      shortcut in, 16 bytes out; 16 lanes per pixel row, rows rr0 + 16 j of the pass): half the memory instructions
        const int cq = tid & 15, rr0 = tid >> 4;
        const float winv = p.wscale_inv[0] * p.wscale_inv[3];
        float4 scA = *(const float4 *)(p.scale + 8 * cq), scB = *(const float4 *)(p.scale + 8 * cq + 4);
        const float4 shA = *(const float4 *)(p.shift + 8 * cq), shB = *(const float4 *)(p.shift + 8 * cq + 4);
        scA.x *= winv; scA.y *= winv; scA.z *= winv; scA.w *= winv; scB.x *= winv; scB.y *= winv; scB.z *= winv; scB.w *= winv;
        float *Ms = (float *)smem;                                      // [2][64 rows][HS_MLD]
        constexpr int NPASS = (NI + 1) / 2;
        f16x8 rv[NPASS][4];                 // ALL shortcut rows of the block are requested before the first pass: one HBM latency per
        unsigned off[NPASS][4];             //   block instead of one per pass (the registers of the main loop's fragments are free by now)
        // the output goes through a buffer descriptor of the image: rows past the block's pixels carry an offset beyond the image and
        // the hardware's range check drops their stores.  No branch around a store: with branches the compiler cannot count the
        // stores in flight and puts s_waitcnt vmcnt(0) before every use of a shortcut row -- each row then waits for the previous
        // row's store to be acknowledged by HBM (16 round trips per block: 11 k of this epilogue's 16 k cycles, profiles/r5_a16_stamps.log)
        const auto o_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)((_Float16 *)p.out + (long)img * HWc * HS_C), 0, HWc * HS_C * 2, 0x00020000);
        float omax = 0.f;                   // f16 tower: the largest |output| this thread wrote (65504 = it was saturated)
        const auto r_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)((_Float16 *)(has_res ? p.res : p.out) + (long)img * HWc * HS_C), 0, HWc * HS_C * 2, 0x00020000);
        const bool sel_res = RECT && p.bg_res != nullptr;
#define HS_ROWS(pass) (((pass) + 1 < NPASS ? 2 : NI - 2 * (NPASS - 1)) * 32)
#define HS_EPI_PREP(pass)                 /* element offsets of this thread's rows (-1: past the block's pixels) + shortcut loads */ \
        {                                                                                       \
            _Pragma("unroll") for (int j = 0; j < HS_ROWS(pass) / 16; ++j) {                    \
                const int m_ = m0 + 64 * (pass) + rr0 + 16 * j;                                 \
                bool stale_ = false;                                                            \
                if (RECT) {                                                                     \
                    const int y_ = (int)(((float)m_ + 0.5f) * invW), x_ = m_ - y_ * Wr;         \
                    off[pass][j] = m_ < m1 ? (unsigned)(((cy0 + y_) * p.Wd + cx0 + x_) * HS_C + 8 * cq) : 0x40000000u; \
                    stale_ = sel_res && (cy0 + y_ < by0 - p.grow_res || cy0 + y_ > by1 + p.grow_res || \
                                         cx0 + x_ < bx0 - p.grow_res || cx0 + x_ > bx1 + p.grow_res); \
                } else off[pass][j] = m_ < m1 ? (unsigned)(m_ * HS_C + 8 * cq) : 0x40000000u;  \
                if (has_res && !RECT) {       /* whole images: the shortcut through the image's descriptor too (one offset register per row) */ \
                    rv[pass][j] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(r_rsrc, 2u * off[pass][j], 0, 0)); \
                } else if (has_res) {                                                           \
                    const _Float16 *rb_ = stale_ ? (const _Float16 *)p.bg_res : (const _Float16 *)p.res + (long)img * HWc * HS_C; \
                    rv[pass][j] = *(const f16x8 *)(rb_ + (off[pass][j] < 0x40000000u ? off[pass][j] : 8u * cq)); \
                }                                                                               \
            }                                                                                   \
        }
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) HS_EPI_PREP(pass)
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
            float *Mb = Ms + (pass & 1) * (64 * HS_MLD);
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
                if (2 * pass + ii < NI) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        Mb[(32 * ii + (r & 3) + 8 * (r >> 2) + 4 * h) * HS_MLD + 32 * wn + l31] = acc[2 * pass + ii][r];
                }
            __syncthreads();
            float4 mA[4], mB[4];
#pragma unroll
            for (int j = 0; j < HS_ROWS(pass) / 16; ++j) {
                mA[j] = *(const float4 *)&Mb[(rr0 + 16 * j) * HS_MLD + 8 * cq];
                mB[j] = *(const float4 *)&Mb[(rr0 + 16 * j) * HS_MLD + 8 * cq + 4];
            }
#pragma unroll
            for (int j = 0; j < HS_ROWS(pass) / 16; ++j) {
                float v[8] = {__builtin_fmaf(mA[j].x, scA.x, shA.x), __builtin_fmaf(mA[j].y, scA.y, shA.y),
                              __builtin_fmaf(mA[j].z, scA.z, shA.z), __builtin_fmaf(mA[j].w, scA.w, shA.w),
                              __builtin_fmaf(mB[j].x, scB.x, shB.x), __builtin_fmaf(mB[j].y, scB.y, shB.y),
                              __builtin_fmaf(mB[j].z, scB.z, shB.z), __builtin_fmaf(mB[j].w, scB.w, shB.w)};
                f16x8 o_;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float t_ = v[e];
                    if (has_res) t_ += hs_from16<BF>(rv[pass][j][e]);
                    t_ = fmaxf(t_, relu_floor);
                    if (!BF && off[pass][j] < 0x40000000u) omax = fmaxf(omax, fabsf(t_));      // f16 activations saturate at 65504: seen, not silent
                    o_[e] = hs_to16<BF>(t_);
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4_t, o_), o_rsrc, 2u * off[pass][j], 0, 0);
            }
        }
#undef HS_ROWS
#undef HS_EPI_PREP
        if (!BF && omax >= 65504.f) {        // the f16 tower's range guard: the same flag word and guard word as the split form's clamp
            int *t = (int *)const_cast<float *>(p.wscale_inv);
            atomicOr(t + 4, 1);
            int *shared = *(int *const *)(t + 6);
            if (shared) __hip_atomic_store(shared, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (RECT && p.bg_out) {              // see the other frame's copy loop below: 16 lanes per pixel here
            const float invF = 1.0f / (float)p.Wd;
            for (int q = part * 16 + rr0; q < HWc; q += 16 * parts) {
                const int y_ = (int)(((float)q + 0.5f) * invF), x_ = q - y_ * p.Wd;
                if (y_ >= cy0 && y_ < cy0 + rh && x_ >= cx0 && x_ < cx0 + rw) continue;
                const int o_ = (y_ * p.Wd + x_) * HS_C + 8 * cq;
                *(f16x8 *)((_Float16 *)p.out + (long)img * HWc * HS_C + o_) = *(const f16x8 *)((const _Float16 *)p.bg_out + o_);
            }
        }
    } else if constexpr (GSTATS) {
    // ---- the training step's input-gradient epilogue (MODE 5 / 7 / 8): the same 64-row exchange; everything a pass needs from HBM --
    //      the shortcut rows, the g_y rows, the mask bytes -- is requested in ONE batch before the pass is exchanged, at clamped
    //      addresses, and NO branch surrounds a load or a store: rows past the block's pixels are computed, kept out of the sums by
    //      their mask, and stored to an offset the image's buffer descriptor drops.  (Round 5's first form kept the g_y row and
    //      the mask byte inside `if (row is the block's)`: the compiler then waited vmcnt(0) in every row -- for the row's own two
    //      loads AND for the previous row's store -- 28 HBM round trips one after the other per thread and block, which is what
    //      made this launch 0.11 ms slower than the bare convolution.)  MODE 7 has no shortcut rows and holds the g_y rows of TWO
    //      passes instead: requested a pass ahead, the first pass's under the last chunk above.
    const int cq = tid & 31, rr0 = tid >> 5;
    const float winv = p.wscale_inv[0] * p.wscale_inv[3];
    const float4 cen4 = *(const float4 *)(p.center + 4 * cq), iv4 = *(const float4 *)(p.g_inv + 4 * cq);
    float4 gsc = cen4, gsh = cen4;
    if (GAFF) { gsc = *(const float4 *)(p.aff_scale + 4 * cq); gsh = *(const float4 *)(p.aff_shift + 4 * cq); }
    float4 st_s = make_float4(0.f, 0.f, 0.f, 0.f), st_q = st_s;
    float *Ms = (float *)smem;                                      // [2][64 rows][HS_MLD]
    // every tensor through a buffer descriptor of the IMAGE: one offset register serves all rows of all passes (a row is a constant
    // further on), and what lies past the image reads as zero (mask byte 0: out of the sums)
    const long ielem = (long)img * HWc * HS_C;
    const auto o_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(p.out + ielem), 0, HWc * HS_C * 4, 0x00020000);
    const auto y_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(p.g_y + ielem), 0, HWc * HS_C * 4, 0x00020000);
    const auto r_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)((has_res ? p.res : p.g_y) + ielem), 0, HWc * HS_C * 4, 0x00020000);
    const auto m_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)((GAFF ? (const unsigned char *)p.g_y : p.g_mask) + (ielem >> 2)), 0, HWc * (HS_C / 4), 0x00020000);
    const auto q_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)((RESMASK ? p.res_mask : (const unsigned char *)p.g_y) + (ielem >> 2)), 0, HWc * (HS_C / 4), 0x00020000);
    const unsigned vo4 = (unsigned)((m0 + rr0) * HS_C + 4 * cq) * 4u, vo1 = (unsigned)((m0 + rr0) * (HS_C / 4) + cq);
    constexpr int NPASS = (NI + 1) / 2;
    float4 rv[8], yv[NORES ? 1 : 8];
    unsigned mbv[GAFF ? 1 : 8], rmv[RESMASK ? 8 : 1];
#define HS_ROWS(pass) (((pass) + 1 < NPASS ? 2 : NI - 2 * (NPASS - 1)) * 32)
#define HS_LD4(rsrc, pass, j) __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, vo4, (64 * (pass) + 8 * (j)) * HS_C * 4, 0))
#define HS_LD1(rsrc, pass, j) (unsigned)(unsigned char)__builtin_amdgcn_raw_buffer_load_b8(rsrc, vo1, (64 * (pass) + 8 * (j)) * (HS_C / 4), 0)
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < HS_ROWS(pass) / 8; ++j) {
            if (!NORES) rv[j] = HS_LD4(r_rsrc, pass, j);     // (MODE 5 without a shortcut: the row is read -- through g_y's descriptor -- and not used)
            if (RESMASK) rmv[j] = HS_LD1(q_rsrc, pass, j);
            if (!NORES) yv[j] = HS_LD4(y_rsrc, pass, j);
            if (!GAFF) mbv[j] = HS_LD1(m_rsrc, pass, j);
        }
        __builtin_amdgcn_sched_barrier(0);
        float *Mb = Ms + (pass & 1) * (64 * HS_MLD);
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
            if (2 * pass + ii < NI) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    Mb[(32 * ii + (r & 3) + 8 * (r >> 2) + 4 * h) * HS_MLD + 32 * wn + l31] = acc[2 * pass + ii][r];
            }
        __syncthreads();
        float4 m[8];
#pragma unroll
        for (int j = 0; j < HS_ROWS(pass) / 8; ++j) m[j] = *(const float4 *)&Mb[(rr0 + 8 * j) * HS_MLD + 4 * cq];
        if (NORES && pass + 1 < NPASS) {
#pragma unroll
            for (int j = 0; j < HS_ROWS(pass + 1) / 8; ++j) gyv[(pass + 1) & 1][j] = HS_LD4(y_rsrc, pass + 1, j);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < HS_ROWS(pass) / 8; ++j) {
            const bool mine = m0 + 64 * pass + rr0 + 8 * j < m1;
            float4 v = m[j];
            v.x = __builtin_fmaf(v.x, winv, 0.f); v.y = __builtin_fmaf(v.y, winv, 0.f);
            v.z = __builtin_fmaf(v.z, winv, 0.f); v.w = __builtin_fmaf(v.w, winv, 0.f);
            if (has_res) {
                float4 r_ = rv[j];
                if (RESMASK) r_ = make_float4((rmv[j] & 1u) ? r_.x : 0.f, (rmv[j] & 2u) ? r_.y : 0.f, (rmv[j] & 4u) ? r_.z : 0.f, (rmv[j] & 8u) ? r_.w : 0.f);
                v.x += r_.x; v.y += r_.y; v.z += r_.z; v.w += r_.w;
            }
            const float4 y_ = NORES ? gyv[pass & 1][j] : yv[j];
            bool bx, by, bz, bw;
            if (GAFF) {                      // the layer's output was never written: its sign is that of k_bn_apply's expression
                bx = y_.x * gsc.x + gsh.x > 0.f; by = y_.y * gsc.y + gsh.y > 0.f; bz = y_.z * gsc.z + gsh.z > 0.f; bw = y_.w * gsc.w + gsh.w > 0.f;
            } else { bx = mbv[j] & 1u; by = mbv[j] & 2u; bz = mbv[j] & 4u; bw = mbv[j] & 8u; }
            const float gx = (mine && bx) ? v.x : 0.f, gy = (mine && by) ? v.y : 0.f, gz = (mine && bz) ? v.z : 0.f, gw = (mine && bw) ? v.w : 0.f;
            st_s.x += gx; st_s.y += gy; st_s.z += gz; st_s.w += gw;
            st_q.x += gx * ((y_.x - cen4.x) * iv4.x); st_q.y += gy * ((y_.y - cen4.y) * iv4.y);
            st_q.z += gz * ((y_.z - cen4.z) * iv4.z); st_q.w += gw * ((y_.w - cen4.w) * iv4.w);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4_t, v), o_rsrc, mine ? vo4 : 0x80000000u,
                                                   (64 * pass + 8 * j) * HS_C * 4, 0);
            // gfx950 reads a 16-byte store's data registers over several cycles; the compiler guards a VALU write to them that follows at
            // once only when the store has NO scalar offset (measured here: rows whose data register pair was rewritten by the
            // next row's v_pk_fma_f32 in the cycle after the store reached HBM with the NEXT row's values in the last four lanes of
            // every sixteen, tools/dbg/igrad_dbg.py) -- so: wait states by hand, and nothing scheduled across them.  The rule as
            // measured (tools/micro/store_hazard.hip, profiles/r6_store_hazard_micro.json): with an SGPR soffset ONE wait state is
            // enough, without one it takes two (those the compiler inserts).  tests/test_store_hazard_cpu.py checks every wide
            // store of the shipped code objects against it; HS_NO_STORE_NOP is that test's proof that it bites.
#ifndef HS_NO_STORE_NOP
            asm volatile("s_nop 2");
#endif
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef HS_ROWS
#undef HS_LD4
#undef HS_LD1
    __syncthreads();                       // the eight row lanes' sums of a channel quad are added through LDS, in a fixed order
    float4 *R = (float4 *)smem;            // [2][8][32]
    R[rr0 * 32 + cq] = st_s;
    R[(8 + rr0) * 32 + cq] = st_q;
    __syncthreads();
    if (rr0 < 2) {
        float4 t = R[(8 * rr0) * 32 + cq];
#pragma unroll
        for (int r = 1; r < 8; ++r) { const float4 u = R[(8 * rr0 + r) * 32 + cq]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        *(float4 *)(p.stat_part + (size_t)blockIdx.x * 256 + rr0 * 128 + 4 * cq) = t;
    }
    } else {
    const int cq = tid & 31, rr0 = tid >> 5;
    const float winv = p.wscale_inv[0] * p.wscale_inv[3];
    float4 sc4 = make_float4(1.f, 1.f, 1.f, 1.f), sh4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!BARE) { sc4 = *(const float4 *)(p.scale + 4 * cq); sh4 = *(const float4 *)(p.shift + 4 * cq); }
    sc4.x *= winv; sc4.y *= winv; sc4.z *= winv; sc4.w *= winv;
    float4 cen4 = make_float4(0.f, 0.f, 0.f, 0.f), st_s = cen4, st_q = cen4;
    if (BARE && p.center) cen4 = *(const float4 *)(p.center + 4 * cq);
    float4 st_m = cen4;
    float *Ms = (float *)smem;                                      // [2][64 rows][HS_MLD]
    const long obase = (PK ? 0l : (long)img * HWc * HS_C) + 4 * cq;     // (PK: a row's offset carries its image)
    float4 wh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_head) wh = *(const float4 *)(p.w1x1 + 4 * cq);
    constexpr int NPASS = (NI + 1) / 2;
    float4 rv[2][8];
    int off[2][8];
    bool res_stale[8];
    int rsrc[8] = {};                                                    // PK: the rows' shortcut sources (the map's .y)
    const float *resq = p.res + 4 * cq, *bgq = p.bg_res + 4 * cq;        // PK: this thread's channels in the shortcut tensor / its background image
    (void)rsrc; (void)resq; (void)bgq;
    const bool sel_res = RECT && p.bg_res != nullptr;
#define HS_ROWS(pass) (((pass) + 1 < NPASS ? 2 : NI - 2 * (NPASS - 1)) * 32)
#define HS_EPI_PREP(pass)                 /* element offsets of this thread's rows (-1: past the block's pixels) + residual loads */ \
    {                                                                                           \
        _Pragma("unroll") for (int j = 0; j < HS_ROWS(pass) / 8; ++j) {                         \
            const int m_ = m0 + 64 * (pass) + rr0 + 8 * j;                                      \
            if (PK) {                         /* the row's entry of the block's map (written in the prologue): a broadcast read */ \
                const int2 e_ = *(const int2 *)(smem + HS_SMEM + 8 * (64 * (pass) + rr0 + 8 * j)); \
                off[(pass) & 1][j] = e_.x;                                                      \
                rsrc[j] = e_.y;                                                                 \
            } else if (RECT) {                                                                  \
                const int y_ = (int)(((float)m_ + 0.5f) * invW), x_ = m_ - y_ * Wr;             \
                off[(pass) & 1][j] = m_ < m1 ? ((cy0 + y_) * p.Wd + cx0 + x_) * HS_C : -1;      \
                res_stale[j] = sel_res && (cy0 + y_ < by0 - p.grow_res || cy0 + y_ > by1 + p.grow_res || \
                                           cx0 + x_ < bx0 - p.grow_res || cx0 + x_ > bx1 + p.grow_res); \
            } else off[(pass) & 1][j] = m_ < m1 ? m_ * HS_C : -1;                               \
        }                                                                                       \
        if (has_res) {                                                                          \
            _Pragma("unroll") for (int j = 0; j < HS_ROWS(pass) / 8; ++j) {                     \
                if (IN16) {                                                                     \
                    const _Float16 *rb_ = (RECT && res_stale[j]) ? (const _Float16 *)p.bg_res + 4 * cq : (const _Float16 *)p.res + obase; \
                    const f16x4 r16_ = *(const f16x4 *)(rb_ + max(off[(pass) & 1][j], 0));      \
                    rv[(pass) & 1][j] = make_float4(hs_from16<BF>(r16_[0]), hs_from16<BF>(r16_[1]), hs_from16<BF>(r16_[2]), hs_from16<BF>(r16_[3])); \
                } else if (PK) {              /* (the entry names the source and the offset in it: see the map) */ \
                    rv[(pass) & 1][j] = *(const float4 *)((rsrc[j] < 0 ? bgq : resq) + (rsrc[j] & 0x7FFFFFFF)); \
                } else {                                                                        \
                    const float *rb_ = (RECT && res_stale[j]) ? p.bg_res + 4 * cq : p.res + obase; \
                    rv[(pass) & 1][j] = *(const float4 *)(rb_ + max(off[(pass) & 1][j], 0));    \
                }                                                                               \
            }                                                                                   \
        }                                                                                       \
    }
    HS_EPI_PREP(0)
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
        if (pass + 1 < NPASS) HS_EPI_PREP(pass + 1)
        float *Mb = Ms + (pass & 1) * (64 * HS_MLD);
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
            if (2 * pass + ii < NI) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    Mb[(32 * ii + (r & 3) + 8 * (r >> 2) + 4 * h) * HS_MLD + 32 * wn + l31] = acc[2 * pass + ii][r];
            }
        __syncthreads();
        float4 m[8];
#pragma unroll
        for (int j = 0; j < HS_ROWS(pass) / 8; ++j) m[j] = *(const float4 *)&Mb[(rr0 + 8 * j) * HS_MLD + 4 * cq];
#pragma unroll
        for (int j = 0; j < HS_ROWS(pass) / 8; ++j) {
            float4 v = m[j];
            v.x = __builtin_fmaf(v.x, sc4.x, sh4.x); v.y = __builtin_fmaf(v.y, sc4.y, sh4.y);
            v.z = __builtin_fmaf(v.z, sc4.z, sh4.z); v.w = __builtin_fmaf(v.w, sc4.w, sh4.w);
            if (has_res) {
                const float4 r_ = rv[pass & 1][j];
                v.x += r_.x; v.y += r_.y; v.z += r_.z; v.w += r_.w;
            }
            v.x = fmaxf(v.x, relu_floor); v.y = fmaxf(v.y, relu_floor); v.z = fmaxf(v.z, relu_floor); v.w = fmaxf(v.w, relu_floor);
            if (STATS && off[pass & 1][j] >= 0) {
                const float ex = v.x - cen4.x, ey = v.y - cen4.y, ez = v.z - cen4.z, ew = v.w - cen4.w;
                st_s.x += ex; st_s.y += ey; st_s.z += ez; st_s.w += ew;
                st_q.x += ex * ex; st_q.y += ey * ey; st_q.z += ez * ez; st_q.w += ew * ew;
                if (AMAX) {                  // the range of what this layer's batch norm can make of it (snk_bn_train_finalize_range)
                    st_m.x = fmaxf(st_m.x, fabsf(ex)); st_m.y = fmaxf(st_m.y, fabsf(ey));
                    st_m.z = fmaxf(st_m.z, fabsf(ez)); st_m.w = fmaxf(st_m.w, fabsf(ew));
                }
            }
            if (has_out && off[pass & 1][j] >= 0) {
                if (OUT16) {
                    f16x4 o16_;
                    o16_[0] = hs_to16<BF>(v.x); o16_[1] = hs_to16<BF>(v.y); o16_[2] = hs_to16<BF>(v.z); o16_[3] = hs_to16<BF>(v.w);
                    *(f16x4 *)((_Float16 *)p.out + obase + off[pass & 1][j]) = o16_;
                } else *(float4 *)(p.out + obase + off[pass & 1][j]) = v;
            }
            if (has_head) {                 // the 32 lanes of this row hold its 128 outputs: reduce their dot product with w1x1
                float d_ = (v.x * wh.x + v.y * wh.y) + (v.z * wh.z + v.w * wh.w);
                // butterfly inside each 16-lane DPP row (quad swaps, half-row mirror, row mirror), then the other row of the 32
                d_ += hs_dpp(d_, 0xB1); d_ += hs_dpp(d_, 0x4E); d_ += hs_dpp(d_, 0x141); d_ += hs_dpp(d_, 0x140);
                d_ += __shfl_xor(d_, 16, 64);
                if (cq == 0 && off[pass & 1][j] >= 0)
                    p.h1[(long)img * HWc + off[pass & 1][j] / HS_C] = fmaxf(__builtin_fmaf(d_, p.s1, p.b1), 0.f);
            }
        }
    }
#undef HS_ROWS
#undef HS_EPI_PREP
    if (BARE) {                            // the eight row lanes' sums of a channel quad are added through LDS, in a fixed order
        __syncthreads();
        float4 *R = (float4 *)smem;        // [2 (3)][8][32]
        R[rr0 * 32 + cq] = st_s;
        R[(8 + rr0) * 32 + cq] = st_q;
        if (AMAX) R[(16 + rr0) * 32 + cq] = st_m;
        __syncthreads();
        if (AMAX && rr0 == 2 && p.amax_part) {
            float4 t = R[16 * 32 + cq];
#pragma unroll
            for (int r = 1; r < 8; ++r) {
                const float4 u = R[(16 + r) * 32 + cq];
                t.x = fmaxf(t.x, u.x); t.y = fmaxf(t.y, u.y); t.z = fmaxf(t.z, u.z); t.w = fmaxf(t.w, u.w);
            }
            *(float4 *)(p.amax_part + (size_t)blockIdx.x * HS_C + 4 * cq) = t;
        }
        if (rr0 < 2) {
            float4 t = R[(8 * rr0) * 32 + cq];
#pragma unroll
            for (int r = 1; r < 8; ++r) { const float4 u = R[(8 * rr0 + r) * 32 + cq]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
            *(float4 *)(p.stat_part + (size_t)blockIdx.x * 256 + rr0 * 128 + 4 * cq) = t;
        }
    }
    if (PK && p.bg_out) {
        // the packed form: a segment with pixels m .. m + n - 1 of the HW of its rectangle fills the same share of its image's canvas,
        // pixels ceil(m HWc / HW) .. ceil((m + n) HWc / HW) - 1: an image's segments tile its canvas, each does work in step with its rows
        const float invF = 1.0f / (float)p.Wd;
        for (int s = 0; s < 2; ++s) {
            const int sm = s ? 0 : m0, sn = s ? nB : nA;
            if (sn == 0) continue;
            const int q_lo = (sm * HWc + HW - 1) / HW, q_hi = ((sm + sn) * HWc + HW - 1) / HW;
            const int fy = s ? ryB : cy0, fx = s ? rxB : cx0;
            float *ob = p.out + (long)(s ? imgB : img) * HWc * HS_C;
            for (int q = q_lo + rr0; q < q_hi; q += 8) {
                const int y_ = (int)(((float)q + 0.5f) * invF), x_ = q - y_ * p.Wd;
                if (y_ >= fy && y_ < fy + rh && x_ >= fx && x_ < fx + rw) continue;
                const int o_ = (y_ * p.Wd + x_) * HS_C + 4 * cq;
                *(float4 *)(ob + o_) = *(const float4 *)(p.bg_out + o_);
            }
        }
    } else if (RECT && p.bg_out) {
        // the layers that read this output are full layers: every pixel of the canvas outside the rectangle takes the layer's
        // state-independent background value; the image's parts share the pixels, 32 lanes per pixel
        const float invF = 1.0f / (float)p.Wd;
        for (int q = part * 8 + rr0; q < HWc; q += 8 * parts) {
            const int y_ = (int)(((float)q + 0.5f) * invF), x_ = q - y_ * p.Wd;
            if (y_ >= cy0 && y_ < cy0 + rh && x_ >= cx0 && x_ < cx0 + rw) continue;
            const int o_ = (y_ * p.Wd + x_) * HS_C + 4 * cq;
            if (OUT16) *(f16x4 *)((_Float16 *)p.out + (long)img * HWc * HS_C + o_) = *(const f16x4 *)((const _Float16 *)p.bg_out + o_);
            else *(float4 *)(p.out + (long)img * HWc * HS_C + o_) = *(const float4 *)(p.bg_out + o_);
        }
    }
    }      // the epilogue of the other frames
    HS_STAMP(4)
}

template <int NI, int MODE, bool SPLIT = true, int IO16 = 0, bool BF = false, bool MX = false>
__global__ __launch_bounds__(256, 2) void k_conv3x3_f16s(ConvHsArgs p)
{
    __shared__ __align__(16) unsigned char smem[HS_SMEM];
    // XCD-aware block -> (image, part) map: workgroups go round-robin to the 8 XCDs, each with its own L2, and the parts of
    // an image share halo rows; parts of one image are therefore 8 workgroups apart (same XCD, dispatched back to back)
    int img, blk;
    {
        const int b = blockIdx.x, per = 8 * p.n_blk;
        if (b < p.n_img_grouped * p.n_blk) { const int r = b % per; img = (b / per) * 8 + (r & 7); blk = r >> 3; }
        else { img = b / p.n_blk; blk = b - img * p.n_blk; }
    }
    const int tile0 = blk * p.tiles_base + min(blk, p.tiles_rem), ntile = p.tiles_base + (blk < p.tiles_rem ? 1 : 0);
    // an image whose tile count is not a multiple of its block count has blocks of NI - 1 tiles: the 16-bit towers' kernel carries
    // that body too (37 x 37: 43 tiles = one block of 8 + five of 7, which all ran the 8-tile body before: a ninth of the full
    // layers' MFMAs computed rows nobody stored); the choice is wave-uniform
    if constexpr (IO16 != 0 && NI > 1) {
        switch (ntile) {
        case NI - 1: hs_block<NI - 1, MODE, SPLIT, IO16, false, BF, MX>(p, smem, img, tile0, ntile, 0, 0, 0, 0, 0u, 0, 1); break;
        default: hs_block<NI, MODE, SPLIT, IO16, false, BF, MX>(p, smem, img, tile0, ntile, 0, 0, 0, 0, 0u, 0, 1); break;
        }
    } else hs_block<NI, MODE, SPLIT, IO16, false, BF, MX>(p, smem, img, tile0, ntile, 0, 0, 0, 0, 0u, 0, 1);
}

// The sub-rectangle form.  The reference's observation (game.py:215-257) is one background pixel (0, WALL, 0) everywhere
// outside the board window, so the output of tower layer k (0-based) is the same for every state outside the window grown
// by k + 2 pixels (the stem: 1): only that rectangle is computed and written per image; what a reader needs beyond its
// producer's rectangle it takes from the producer's constant background image (QNet.backgrounds; p.bg_in / p.bg_res, chosen
// per staging item and per shortcut row when the block sets up its addresses).  Blocks take (image, rectangle, tile range,
// bounding box) from descriptors written by k_rect_plan; the M-tile count of a block selects the body at run time
// (wave-uniform), so one launch covers every rectangle shape of the batch.
template <int MODE, bool SPLIT = true, int IO16 = 0, bool BF = false, bool MX = false>
__global__ __launch_bounds__(256, 2) void k_conv3x3_f16s_rect(ConvHsArgs p)
{
    __shared__ __align__(16) unsigned char smem[HS_SMEM];
    const int nd = *p.n_desc;
    const uint4 d = p.desc[blockIdx.x];                    // both loads in flight together: the grid never exceeds the array
    if ((int)blockIdx.x >= nd) return;
    const int img = (int)d.x, ry0 = d.y & 255, rx0 = (d.y >> 8) & 255, rh = (d.y >> 16) & 255, rw = d.y >> 24;
    const int tile0 = d.z & 255, ntile = (d.z >> 8) & 255, part = (d.z >> 16) & 255, parts = d.z >> 24;
#define HS_RECT_CASE(NI_) case NI_: hs_block<NI_, MODE, SPLIT, IO16, true, BF, MX>(p, smem, img, tile0, ntile, ry0, rx0, rh, rw, d.w, part, parts); break;
    switch (ntile) {
        HS_RECT_CASE(1) HS_RECT_CASE(2) HS_RECT_CASE(3) HS_RECT_CASE(4) HS_RECT_CASE(5) HS_RECT_CASE(6) HS_RECT_CASE(7)
    default: hs_block<8, MODE, SPLIT, IO16, true, BF, MX>(p, smem, img, tile0, ntile, ry0, rx0, rh, rw, d.w, part, parts); break;
    }
#undef HS_RECT_CASE
}

// The packed sub-rectangle form (float32-accurate tower): a block's descriptor is two uint4, one per segment --
//   { image, y0 | x0 << 8 | h << 16 | w << 24, first pixel | pixels << 16, bounding box } and
//   { image B, the same with B's position, pixels of B (0: one segment) | M tiles << 16, B's bounding box }
// (a one-segment block repeats its image in the second word group, so that every 16-byte entry names an image and its rectangle);
// *n_desc counts 16-byte entries.  Written by k_rect_plan_pack / k_rect_pack_resolve.
template <int MODE>
__global__ __launch_bounds__(256, 2) void k_conv3x3_f16s_rectp(ConvHsArgs p)
{
    __shared__ __align__(16) unsigned char smem[HS_SMEM + HS_ROWMAP];                  // the block's row map sits behind the staging / exchange buffers
    const int nd = *p.n_desc;
    const uint4 dA = p.desc[2 * blockIdx.x], dB = p.desc[2 * blockIdx.x + 1];      // the grid never exceeds the array
    if (2 * (int)blockIdx.x >= nd) return;
    const int img = (int)dA.x, ry0 = dA.y & 255, rx0 = (dA.y >> 8) & 255, rh = (dA.y >> 16) & 255, rw = dA.y >> 24;
    const int mA = dA.z & 0xFFFF, nA = dA.z >> 16, nB = dB.z & 0xFFFF, ntile = (dB.z >> 16) & 15;
    const int imgB = (int)dB.x, ryB = dB.y & 255, rxB = (dB.y >> 8) & 255;
#define HS_RECT_CASE(NI_) case NI_: hs_block<NI_, MODE, true, 0, true, false, false, true>(p, smem, img, mA, nA, ry0, rx0, rh, rw, dA.w, 0, 1, imgB, ryB, rxB, dB.w, nB); break;
    switch (ntile) {
        HS_RECT_CASE(1) HS_RECT_CASE(2) HS_RECT_CASE(3) HS_RECT_CASE(4) HS_RECT_CASE(5) HS_RECT_CASE(6) HS_RECT_CASE(7)
    default: hs_block<8, MODE, true, 0, true, false, false, true>(p, smem, img, mA, nA, ry0, rx0, rh, rw, dA.w, 0, 1, imgB, ryB, rxB, dB.w, nB); break;
    }
#undef HS_RECT_CASE
}

// max |w| of the layer -> k with 256 <= max * 2^k < 512; writes {2^-k, 2^k, x_scale, 1 / x_scale, range flag = 0} behind the fragment image
__global__ __launch_bounds__(1024) void k_f16s_wscale(const float *__restrict__ w, float *__restrict__ tail, float x_scale,
                                                      const float *__restrict__ in_tail = nullptr)
{
    __shared__ float red[1024];
    float m = 0.f;
    const float4 *w4 = (const float4 *)w;                      // 9 * 128 * 128 / 4 = 36 float4 per thread, all in flight
#pragma unroll 12
    for (int i = threadIdx.x; i < 9 * HS_C * HS_C / 4; i += 1024) {
        const float4 v = w4[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float mx = red[0];
        int k = 0;
        if (mx > 0.f && mx < 3.0e38f) k = 8 - ilogbf(mx);
        k = max(-119, min(100, k));                           // (-119 is never reached: ilogb <= 127; a clamp at -100 left
                                                              //  max * 2^k >= 65536 from max = 2^116 on: hi halves of infinity)
        tail[0] = ldexpf(1.0f, -k);
        tail[1] = ldexpf(1.0f, k);
        tail[2] = in_tail ? in_tail[2] : x_scale;             // the producer of the input measured its range (train.hip)
        tail[3] = in_tail ? in_tail[3] : 1.0f / x_scale;
        tail[4] = tail[5] = tail[6] = tail[7] = 0.f;          // range flag (an int32, bit pattern 0) + padding
    }
}

// the tail of an image of the SAME kernel values (their power-of-two scale is known) with another input's range
__global__ void k_f16s_tail_from(const float *__restrict__ w_tail, const float *__restrict__ in_tail, float *__restrict__ tail)
{
    if (threadIdx.x == 0) {
        tail[0] = w_tail[0]; tail[1] = w_tail[1];
        tail[2] = in_tail[2]; tail[3] = in_tail[3];
        tail[4] = tail[5] = tail[6] = tail[7] = 0.f;
    }
}

// f16(v), round to nearest even, a zero result with v's sign: the compiler folds the product in front of the conversion into
// v_fma_mixlo_f16 (w, 2^k, +0), whose +0 addend turns a weight of -0.0 into hi = +0 and lo = -0 (the same value; the images are
// specified byte for byte, tests/weight_image_ref.py)
__device__ __forceinline__ _Float16 hs_f16_keep_sign(float v)
{
    const unsigned short b = __builtin_bit_cast(unsigned short, (_Float16)v) | (unsigned short)((__builtin_bit_cast(unsigned, v) >> 16) & 0x8000u);
    return __builtin_bit_cast(_Float16, b);
}

// Keras kernel (kh, kw, cin, cout) float32 -> split f16 fragments in the order the conv kernel's waves load them
// FLIP: the kernel of the INPUT GRADIENT of the same layer -- taps mirrored, channel axes swapped: w'[tap][ci][co] = w[8 - tap][co][ci]
template <bool FLIP>
__global__ void k_f16s_weights(const float *__restrict__ w, _Float16 *__restrict__ wS, const float *__restrict__ tail)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;          // one f16x8 fragment piece
    if (v >= HS_WS_ELEMS / 8) return;
    const float mul = tail[1];
    const int g = v / 512, rem = v - g * 512;
    const int c = g / 9, tap = g - 9 * c;                       // 16-channel chunk, tap
    const int wn = rem >> 7, hl = (rem >> 6) & 1, lane = rem & 63;
    const int h = lane >> 5, l31 = lane & 31;
    const int cout = 32 * wn + l31;
    for (int j = 0; j < 8; ++j) {
        const int cin = HS_KC * c + 8 * h + j;
        const float val = (FLIP ? w[(long)((8 - tap) * HS_C + cout) * HS_C + cin] : w[(long)(tap * HS_C + cin) * HS_C + cout]) * mul;
        const _Float16 hi = hs_f16_keep_sign(val);
        wS[(long)v * 8 + j] = hl ? (_Float16)(val - (float)hi) : hi;
    }
}

// the 16-bit frame's weight image: [chunk of 32 input channels 4][tap 9][wn 4][k step 2][lane 64] x 8 values (f16, or bf16
// patterns): the two fragments a wave loads per (chunk, tap) are the chunk's two MFMA k steps, where the split image keeps hi and lo
template <bool BF>
__global__ void k_a16_weights(const float *__restrict__ w, _Float16 *__restrict__ wS, const float *__restrict__ tail)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;          // one fragment piece of eight values
    if (v >= 9 * HS_C * HS_C / 8) return;
    const float mul = tail[1];
    const int g = v / 512, rem = v - g * 512;
    const int c = g / 9, tap = g - 9 * c;
    const int wn = rem >> 7, ks = (rem >> 6) & 1, lane = rem & 63;
    const int h = lane >> 5, l31 = lane & 31;
    const int cout = 32 * wn + l31;
    for (int j = 0; j < 8; ++j) {
        const int cin = 32 * c + 16 * ks + 8 * h + j;
        const float val = w[(long)(tap * HS_C + cin) * HS_C + cout] * mul;
        wS[(long)v * 8 + j] = BF ? __builtin_bit_cast(_Float16, (__bf16)val) : hs_f16_keep_sign(val);
    }
}

// the mxfp8 tower's weight image (snk_conv3x3_prepare_weights_mxfp8), quantized by the MX rule (see mx_scale_byte) from the float32
// kernel: e4m3fn codes [step 18 = (chunk of 64 input channels) x 9 + tap][wn 4][half p 2][lane 64] x 16 bytes -- lane (h, r) of wave wn
// holds input channels 64 chunk + 32 p + 16 h + 0..15 of output channel 32 wn + r in half p: the MFMA takes bytes 16 b .. 16 b + 15 of
// BOTH lane halves as its k-block b, whose scale comes from lane (b, r) -- then the blocks' scale bytes [step][wn][lane] (lane (h, r):
// block h), then at the 16-bit images' tail offset {1, 1, 1, 1, flag 0, 0, guard 0}: the MFMA applies the scales, the epilogue
// has nothing to undo.  One thread per (step, output channel): its two blocks.
__global__ __launch_bounds__(256) void k_mxfp8_weights(const float *__restrict__ w, unsigned char *__restrict__ wS)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= 18 * 128) return;
    const int g = v >> 7, wn = (v >> 5) & 3, r = v & 31;
    const int c = g / 9, tap = g - 9 * c, cout = 32 * wn + r;
    const float *src = w + (long)(tap * HS_C + 64 * c) * HS_C + cout;         // input channel 64 c + i: src[i * HS_C]
    unsigned sb[2];
    float k[2];
    for (int b = 0; b < 2; ++b) {
        float m = 0.f;
        for (int j = 0; j < 32; ++j) m = fmaxf(m, fabsf(src[(32 * b + j) * HS_C]));
        sb[b] = mx_scale_byte(m);
        k[b] = mx_inv_scale(sb[b]);
    }
    for (int h = 0; h < 2; ++h)
        for (int pp = 0; pp < 2; ++pp) {
            const float *s_ = src + (32 * pp + 16 * h) * HS_C;
            unsigned q[4];
            for (int j = 0; j < 4; ++j)
                q[j] = mx_pack4(s_[(4 * j) * HS_C] * k[pp], s_[(4 * j + 1) * HS_C] * k[pp], s_[(4 * j + 2) * HS_C] * k[pp],
                                s_[(4 * j + 3) * HS_C] * k[pp]);
            *(uint4 *)(wS + ((long)((g * 4 + wn) * 2 + pp) * 64 + 32 * h + r) * 16) = make_uint4(q[0], q[1], q[2], q[3]);
        }
    for (int h = 0; h < 2; ++h) wS[9 * HS_C * HS_C + (g * 4 + wn) * 64 + 32 * h + r] = (unsigned char)sb[h];
    if (v < 8) ((float *)(wS + 2 * HS_WS_ELEMS))[v] = v < 4 ? 1.0f : 0.0f;
}

// the staging path's quantizer on a plain bf16 array, for the tests: block b = x[32 b .. 32 b + 31] -> codes[32 b ..], scales[b];
// four lanes per block as in staging (mx_quant8); lanes past the last block repeat it (every lane runs the quad's DPP steps)
__global__ __launch_bounds__(256) void k_mxfp8_quantize(const _Float16 *__restrict__ x, long n_blocks, unsigned char *__restrict__ codes,
                                                        unsigned char *__restrict__ scales)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x, b = t >> 2, bc = b < n_blocks ? b : n_blocks - 1;
    const int q = (int)(t & 3);
    unsigned sb;
    const uint2 c = mx_quant8(*(const f16x8 *)(x + bc * 32 + 8 * q), sb);
    if (b < n_blocks) {
        *(uint2 *)(codes + b * 32 + 8 * q) = c;
        if (q == 0) scales[b] = (unsigned char)sb;
    }
}

extern "C" int snk_conv3x3_prepare_weights_mxfp8(const float *d_w_hwio, void *d_wS, void *stream)
{
    SNK_REQUIRE(d_w_hwio && d_wS, "snk_conv3x3_prepare_weights_mxfp8: NULL argument");
    k_mxfp8_weights<<<9, 256, 0, (hipStream_t)stream>>>(d_w_hwio, (unsigned char *)d_wS);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_mxfp8_quantize_bf16(const void *d_x, int n_blocks, void *d_codes, void *d_scales, void *stream)
{
    SNK_REQUIRE(d_x && d_codes && d_scales, "snk_mxfp8_quantize_bf16: NULL argument");
    SNK_REQUIRE(n_blocks > 0 && n_blocks <= (1 << 28), "snk_mxfp8_quantize_bf16: %d blocks", n_blocks);
    k_mxfp8_quantize<<<(int)(((long)n_blocks * 4 + 255) / 256), 256, 0, (hipStream_t)stream>>>((const _Float16 *)d_x, n_blocks,
                                                                                             (unsigned char *)d_codes, (unsigned char *)d_scales);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the guard word: one device int32 that every layer of a net reports clamps to ----------------------------------------------
__global__ void k_f16s_set_guard_word(int *tail, int *word) { *(int **)(tail + 6) = word; }

extern "C" int snk_conv3x3_f16s_set_guard_word(void *d_wS, int32_t *d_word, void *stream)
{
    SNK_REQUIRE(d_wS, "snk_conv3x3_f16s_set_guard_word: NULL weight image");
    k_f16s_set_guard_word<<<1, 1, 0, (hipStream_t)stream>>>((int *)((_Float16 *)d_wS + HS_WS_ELEMS), (int *)d_word);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_conv3x3_prepare_weights_f16s(const float *d_w_hwio, void *d_wS, float x_scale, void *stream)
{
    SNK_REQUIRE(d_w_hwio && d_wS, "snk_conv3x3_prepare_weights_f16s: NULL argument");
    int e_ = 0;
    SNK_REQUIRE(x_scale > 0.f && frexpf(x_scale, &e_) == 0.5f, "snk_conv3x3_prepare_weights_f16s: x_scale %g is not a power of two", x_scale);
    float *tail = (float *)((_Float16 *)d_wS + HS_WS_ELEMS);
    k_f16s_wscale<<<1, 1024, 0, (hipStream_t)stream>>>(d_w_hwio, tail, x_scale);
    k_f16s_weights<false><<<(HS_WS_ELEMS / 8 + 255) / 256, 256, 0, (hipStream_t)stream>>>(d_w_hwio, (_Float16 *)d_wS, tail);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

// the weight image of the bf16 tower (snk_conv3x3_bn_bf16_act16): the same layout with bf16 parts, activation scale 1
extern "C" int snk_conv3x3_prepare_weights_bf16(const float *d_w_hwio, void *d_wS, void *stream)
{
    SNK_REQUIRE(d_w_hwio && d_wS, "snk_conv3x3_prepare_weights_bf16: NULL argument");
    float *tail = (float *)((_Float16 *)d_wS + HS_WS_ELEMS);
    k_f16s_wscale<<<1, 1024, 0, (hipStream_t)stream>>>(d_w_hwio, tail, 1.0f);
    k_a16_weights<true><<<(9 * HS_C * HS_C / 8 + 255) / 256, 256, 0, (hipStream_t)stream>>>(d_w_hwio, (_Float16 *)d_wS, tail);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

// the weight image of the f16-activation tower (snk_conv3x3_bn_f16_act16): the same layout with f16 values (pre-scaled by the power of
// two that brings max |w| to [256, 512); undone in the epilogue), activation scale 1
extern "C" int snk_conv3x3_prepare_weights_f16_act16(const float *d_w_hwio, void *d_wS, void *stream)
{
    SNK_REQUIRE(d_w_hwio && d_wS, "snk_conv3x3_prepare_weights_f16_act16: NULL argument");
    float *tail = (float *)((_Float16 *)d_wS + HS_WS_ELEMS);
    k_f16s_wscale<<<1, 1024, 0, (hipStream_t)stream>>>(d_w_hwio, tail, 1.0f);
    k_a16_weights<false><<<(9 * HS_C * HS_C / 8 + 255) / 256, 256, 0, (hipStream_t)stream>>>(d_w_hwio, (_Float16 *)d_wS, tail);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

// the training step's form: the input scale is read on the device from d_in_tail = { ., ., scale, 1 / scale } (what
// snk_bn_train_apply / snk_bn_train_grad_apply measured while writing the tensor this layer reads); input_gradient != 0
// lays out the kernel of the layer's input gradient (the same convolution with mirrored taps and swapped channel axes);
// d_wS_same_kernel (optional): an image made from the same d_w_hwio values, whose weight scale is reused instead of
// scanning the kernel for its largest entry again
extern "C" int snk_conv3x3_prepare_weights_f16s_train(const float *d_w_hwio, void *d_wS, const float *d_in_tail, int input_gradient,
                                                      const void *d_wS_same_kernel, void *stream)
{
    SNK_REQUIRE(d_w_hwio && d_wS && d_in_tail && d_wS != d_wS_same_kernel, "snk_conv3x3_prepare_weights_f16s_train: bad argument");
    float *tail = (float *)((_Float16 *)d_wS + HS_WS_ELEMS);
    if (d_wS_same_kernel)
        k_f16s_tail_from<<<1, 64, 0, (hipStream_t)stream>>>((const float *)((const _Float16 *)d_wS_same_kernel + HS_WS_ELEMS), d_in_tail, tail);
    else k_f16s_wscale<<<1, 1024, 0, (hipStream_t)stream>>>(d_w_hwio, tail, 1.0f, d_in_tail);
    if (input_gradient) k_f16s_weights<true><<<(HS_WS_ELEMS / 8 + 255) / 256, 256, 0, (hipStream_t)stream>>>(d_w_hwio, (_Float16 *)d_wS, tail);
    else k_f16s_weights<false><<<(HS_WS_ELEMS / 8 + 255) / 256, 256, 0, (hipStream_t)stream>>>(d_w_hwio, (_Float16 *)d_wS, tail);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

// All tower layers of a training step at once (snake_engine/train_step.py): for every layer i the power-of-two weight scale (once
// per kernel, shared by its two images), the forward image and -- where h_wS_bwd[i] is given -- the input gradient's image, in TWO
// launches instead of four per layer and direction.  The images' input scales (tail[2..3]) are NOT set here: the training step has
// the element-wise kernel that writes a convolution's input leave them there directly (d_out_scale_tail / d_dx_scale_tail =
// the image's tail), so a weight image is made once per optimizer step and stays valid for as long as the weights do (every
// forward-only step at learning rate 0 reuses it).
#define HS_BATCH_MAX 40
struct F16sBatch { const float *w[HS_BATCH_MAX]; _Float16 *fwd[HS_BATCH_MAX]; _Float16 *bwd[HS_BATCH_MAX]; };

__global__ __launch_bounds__(1024) void k_f16s_wscale_batch(F16sBatch b)
{
    __shared__ float red[1024];
    const float4 *w4 = (const float4 *)b.w[blockIdx.x];
    float m = 0.f;
#pragma unroll 12
    for (int i = threadIdx.x; i < 9 * HS_C * HS_C / 4; i += 1024) {
        const float4 v = w4[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x < 2) {
        _Float16 *img = threadIdx.x == 0 ? b.fwd[blockIdx.x] : b.bwd[blockIdx.x];
        if (!img) return;
        float *tail = (float *)(img + HS_WS_ELEMS);
        const float mx = red[0];
        int k = 0;
        if (mx > 0.f && mx < 3.0e38f) k = 8 - ilogbf(mx);          // as k_f16s_wscale
        k = max(-119, min(100, k));
        tail[0] = ldexpf(1.0f, -k);
        tail[1] = ldexpf(1.0f, k);
        tail[4] = tail[5] = tail[6] = tail[7] = 0.f;              // range flag, no guard word; tail[2..3] belong to the input's producer
    }
}

// grid (pieces / 256, layers, 2 directions); the tails' weight scales were written by k_f16s_wscale_batch (the launch before)
__global__ __launch_bounds__(256) void k_f16s_weights_batch(F16sBatch b)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;          // one f16x8 fragment piece
    const bool flip = blockIdx.z != 0;
    _Float16 *wS = flip ? b.bwd[blockIdx.y] : b.fwd[blockIdx.y];
    if (v >= HS_WS_ELEMS / 8 || !wS) return;
    const float *w = b.w[blockIdx.y];
    const float mul = ((const float *)(wS + HS_WS_ELEMS))[1];
    const int g = v / 512, rem = v - g * 512;
    const int c = g / 9, tap = g - 9 * c;                       // (the fragment order of k_f16s_weights)
    const int wn = rem >> 7, hl = (rem >> 6) & 1, lane = rem & 63;
    const int h = lane >> 5, l31 = lane & 31;
    const int cout = 32 * wn + l31;
    for (int j = 0; j < 8; ++j) {
        const int cin = HS_KC * c + 8 * h + j;
        const float val = (flip ? w[(long)((8 - tap) * HS_C + cout) * HS_C + cin] : w[(long)(tap * HS_C + cin) * HS_C + cout]) * mul;
        const _Float16 hi = hs_f16_keep_sign(val);
        wS[(long)v * 8 + j] = hl ? (_Float16)(val - (float)hi) : hi;
    }
}

extern "C" int snk_conv3x3_prepare_weights_f16s_train_batch(const float *const *h_w_hwio, void *const *h_wS_fwd, void *const *h_wS_bwd,
                                                            int n_layers, void *stream)
{
    SNK_REQUIRE(h_w_hwio && h_wS_fwd && n_layers > 0 && n_layers <= HS_BATCH_MAX,
                "snk_conv3x3_prepare_weights_f16s_train_batch: 1 .. %d layers per call", HS_BATCH_MAX);
    F16sBatch b = {};
    bool any_bwd = false;
    for (int i = 0; i < n_layers; ++i) {
        SNK_REQUIRE(h_w_hwio[i] && h_wS_fwd[i], "snk_conv3x3_prepare_weights_f16s_train_batch: NULL kernel or image (layer %d)", i);
        b.w[i] = h_w_hwio[i];
        b.fwd[i] = (_Float16 *)h_wS_fwd[i];
        b.bwd[i] = h_wS_bwd ? (_Float16 *)h_wS_bwd[i] : nullptr;
        any_bwd = any_bwd || b.bwd[i];
    }
    k_f16s_wscale_batch<<<n_layers, 1024, 0, (hipStream_t)stream>>>(b);
    k_f16s_weights_batch<<<dim3((HS_WS_ELEMS / 8 + 255) / 256, n_layers, any_bwd ? 2 : 1), 256, 0, (hipStream_t)stream>>>(b);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------
// One launch as its entry point states it.  a: the ConvHsArgs members the entry point sets, by name (x, wS and the canvas come from
// conv_form); the launchers fill in the weight image's tail and the block plan.  Nothing is deduced from which pointers are set:
// the entry point names its MODE and frame, and conv_form_check refuses a form whose arguments contradict them.
struct ConvForm {
    const char *who;           // the entry point that was called, for the wording of a refusal
    int mode;                  // HsMode
    bool split;                // true: the split f16s form; false: one MFMA per product (single-pass f16 and the 16-bit towers)
    int io16;                  // 0: float32 tensors; 1: 16-bit activations in, float32 out; 3: 16-bit in and out
    bool bf, mx;               // 16-bit towers: bf16 instead of f16; MX-FP8 operands (with bf)
    int n_images;
    void *stream;
    ConvHsArgs a;
};

static ConvForm conv_form(const char *who, int mode, const void *d_x, const void *d_wS, int n_images, int height, int width, void *stream)
{
    ConvForm f = {};
    f.who = who; f.mode = mode; f.split = true; f.n_images = n_images; f.stream = stream;
    f.a.x = (const float *)d_x; f.a.wS = (const f16x8 *)d_wS; f.a.Hd = height; f.a.Wd = width;
    return f;
}

// the compile-time epilogue of a tower layer: ReLU without / with shortcut; anything else takes the generic one
static int hs_tower_mode(int relu, const void *d_residual) { return !relu ? HS_MODE_ARGS : d_residual ? HS_MODE_RES_RELU : HS_MODE_RELU; }

// The block plan of a full-form launch: n_blk blocks per image of at most tiles_max M tiles (tests/conv_plan_ref.py restates it).
static int conv_f16s_plan(const char *who, int n_images, int height, int width, bool a16, int *n_blk_out, int *tiles_max_out)
{
    const int P = width + 1, HW = height * width;
    // (a16: the 16-bit frame: LDS rows pitched in bytes, six staging items)
    const int nst_px = 64 * (a16 ? HS_NST16 : HS_NST);
    // GEMM rows = the image's pixels in row-major order, 32 per M tile; an image is cut into n_blk blocks of at most 8 M
    // tiles whose input rows (those of its pixels + one above and below) fit the LDS buffer and the staging items
    const int T = (HW + 31) / 32;
    int n_blk = (T + 7) / 8, tiles_max = 0;
    bool fits = false;
    for (;; ++n_blk) {
        tiles_max = (T + n_blk - 1) / n_blk;
        const int rows_out = min((tiles_max * 32 + width - 2) / width + 1, height);       // worst alignment of 32 tiles_max pixels
        fits = (a16 ? (rows_out + 2) * (width * HS_LDP + HS_GAP16_FULL) <= HS_BUF16 : (rows_out + 2) * P + 1 <= HS_NPB) &&
               min(rows_out + 2, height) * width <= nst_px;
        if (fits || tiles_max == 1) break;
    }
    SNK_REQUIRE(fits, "%s: observation width %d not supported (max 80)", who, width);
    // very small batches (measured: up to ~40 images at 21x21): cut the images finer so that the grid covers more of the
    // chip's block slots -- a block's duration, not the throughput, is what such a launch costs (16 states: 31 -> 14 us);
    // from ~48 images on the 7-tile blocks with their compile-time epilogues are faster again
    static const int fine_max = getenv("SNK_CONV_FINE_MAX") ? atoi(getenv("SNK_CONV_FINE_MAX")) : 40;
    if (n_images <= fine_max && n_images * n_blk < 512) {
        n_blk = min(T, max(n_blk, (512 + n_images - 1) / n_images));
        tiles_max = (T + n_blk - 1) / n_blk;
    }
    *n_blk_out = n_blk;
    *tiles_max_out = tiles_max;
    return 0;
}

// What a MODE needs of the arguments and excludes -- the cross-checks the launcher once made by the order in which it looked at pointers.
static int conv_form_check(const ConvForm &f)
{
    const ConvHsArgs &a = f.a;
    const bool aff = a.aff_scale && a.aff_shift, no_aff = !a.aff_scale && !a.aff_shift, igrad = a.g_y && a.g_inv;
    SNK_REQUIRE(!(f.mode == HS_MODE_IGRAD_AFF && a.res), "%s: the layer below a block's second convolution has no shortcut gradient to add", f.who);
    bool ok = false;
    switch (f.mode) {
    case HS_MODE_ARGS:           ok = true; break;
    case HS_MODE_RELU:           ok = a.relu && !a.res && a.out && !a.w1x1; break;
    case HS_MODE_RES_RELU:       ok = a.relu && a.res && a.out && !a.w1x1; break;
    case HS_MODE_HEAD:           ok = a.relu && a.res && !a.out && a.w1x1 && a.h1; break;     // the fused head closes a residual block
    case HS_MODE_STATS:          ok = !a.g_y && no_aff && !a.res_mask; break;
    case HS_MODE_IGRAD:          ok = igrad && a.g_mask && no_aff && !a.res_mask; break;
    case HS_MODE_STATS_AFF:      ok = !a.g_y && aff && !a.amax_part && !a.res_mask; break;
    case HS_MODE_IGRAD_AFF:      ok = igrad && !a.g_mask && aff && !a.res_mask; break;
    case HS_MODE_IGRAD_MRES:     ok = igrad && a.g_mask && no_aff && a.res && a.res_mask; break;
    case HS_MODE_STATS_AFF_AMAX: ok = !a.g_y && aff && a.amax_part && !a.res_mask; break;
    case HS_MODE_IGRAD_MRES_AFF: ok = igrad && !a.g_mask && aff && a.res && a.res_mask; break;
    }
    // the training forms are bare convolutions on float32 tensors that leave sums; the inference forms leave none
    if (f.mode >= HS_MODE_STATS) ok = ok && a.stat_part && a.out && !a.w1x1 && f.io16 == 0 && !f.bf && !f.mx;
    else ok = ok && !a.stat_part && !a.amax_part && !a.g_y && no_aff && !a.res_mask;
    SNK_REQUIRE(ok, "%s: the arguments do not make MODE %d", f.who, f.mode);
    SNK_REQUIRE((f.io16 == 0 || ((f.io16 == 1 || f.io16 == 3) && !f.split)) && (f.io16 != 0 || !f.bf) && (!f.mx || f.bf),
                "%s: no frame split %d, io16 %d, bf %d, mx %d", f.who, f.split, f.io16, f.bf, f.mx);
    return 0;
}

// The NI switch, once: the kernel compiled for n_mt M tiles per block of the frame <MODE, SPLIT, IO16, BF, MX>.
template <int MODE, bool SPLIT, int IO16, bool BF, bool MX>
static void hs_launch(const ConvHsArgs &a, int n_mt, int grid, hipStream_t st)
{
    switch (n_mt) {
    case 1: k_conv3x3_f16s<1, MODE, SPLIT, IO16, BF, MX><<<grid, 256, 0, st>>>(a); break;
    case 2: k_conv3x3_f16s<2, MODE, SPLIT, IO16, BF, MX><<<grid, 256, 0, st>>>(a); break;
    case 3: k_conv3x3_f16s<3, MODE, SPLIT, IO16, BF, MX><<<grid, 256, 0, st>>>(a); break;
    case 4: k_conv3x3_f16s<4, MODE, SPLIT, IO16, BF, MX><<<grid, 256, 0, st>>>(a); break;
    case 5: k_conv3x3_f16s<5, MODE, SPLIT, IO16, BF, MX><<<grid, 256, 0, st>>>(a); break;
    case 6: k_conv3x3_f16s<6, MODE, SPLIT, IO16, BF, MX><<<grid, 256, 0, st>>>(a); break;
    case 7: k_conv3x3_f16s<7, MODE, SPLIT, IO16, BF, MX><<<grid, 256, 0, st>>>(a); break;
    default: k_conv3x3_f16s<8, MODE, SPLIT, IO16, BF, MX><<<grid, 256, 0, st>>>(a); break;
    }
}

// the training forms: float32 tensors, the split form or the single-pass f16 form (the same frames with the hi halves only)
template <int MODE> static void hs_launch_train(const ConvForm &f, const ConvHsArgs &a, int n_mt, int grid)
{
    if (f.split) hs_launch<MODE, true, 0, false, false>(a, n_mt, grid, (hipStream_t)f.stream);
    else hs_launch<MODE, false, 0, false, false>(a, n_mt, grid, (hipStream_t)f.stream);
}

// the 16-bit towers: f16, bf16 or MX-FP8 operands (IO16: 1 = 16-bit in, float32 out; 3 = 16-bit in and out)
template <int MODE, int IO16> static void hs_launch_a16(const ConvForm &f, const ConvHsArgs &a, int n_mt, int grid)
{
    if (f.mx) hs_launch<MODE, false, IO16, true, true>(a, n_mt, grid, (hipStream_t)f.stream);
    else if (f.bf) hs_launch<MODE, false, IO16, true, false>(a, n_mt, grid, (hipStream_t)f.stream);
    else hs_launch<MODE, false, IO16, false, false>(a, n_mt, grid, (hipStream_t)f.stream);
}

// The one place that says which <MODE, SPLIT, IO16, BF, MX> are built; false: this form has no kernel.
static bool hs_dispatch(const ConvForm &f, const ConvHsArgs &a, int n_mt, int grid)
{
    hipStream_t st = (hipStream_t)f.stream;
    if (f.mode >= HS_MODE_STATS) {
        switch (f.mode) {
        case HS_MODE_STATS:          hs_launch_train<HS_MODE_STATS>(f, a, n_mt, grid); return true;
        case HS_MODE_IGRAD:          hs_launch_train<HS_MODE_IGRAD>(f, a, n_mt, grid); return true;
        case HS_MODE_STATS_AFF:      hs_launch_train<HS_MODE_STATS_AFF>(f, a, n_mt, grid); return true;
        case HS_MODE_IGRAD_AFF:      hs_launch_train<HS_MODE_IGRAD_AFF>(f, a, n_mt, grid); return true;
        case HS_MODE_IGRAD_MRES:     hs_launch_train<HS_MODE_IGRAD_MRES>(f, a, n_mt, grid); return true;
        case HS_MODE_STATS_AFF_AMAX: hs_launch_train<HS_MODE_STATS_AFF_AMAX>(f, a, n_mt, grid); return true;
        case HS_MODE_IGRAD_MRES_AFF: hs_launch_train<HS_MODE_IGRAD_MRES_AFF>(f, a, n_mt, grid); return true;
        }
        return false;
    }
    if (f.io16 == 3) {           // a tower layer whose reader is another layer
        switch (f.mode) {
        case HS_MODE_ARGS:     hs_launch_a16<HS_MODE_ARGS, 3>(f, a, n_mt, grid); return true;
        case HS_MODE_RELU:     hs_launch_a16<HS_MODE_RELU, 3>(f, a, n_mt, grid); return true;
        case HS_MODE_RES_RELU: hs_launch_a16<HS_MODE_RES_RELU, 3>(f, a, n_mt, grid); return true;
        }
        return false;
    }
    if (f.io16 == 1) {           // the layer the head reads, or the one that carries the head's 1x1 stage in its epilogue
        switch (f.mode) {
        case HS_MODE_ARGS:     hs_launch_a16<HS_MODE_ARGS, 1>(f, a, n_mt, grid); return true;
        case HS_MODE_RELU:     hs_launch_a16<HS_MODE_RELU, 1>(f, a, n_mt, grid); return true;
        case HS_MODE_RES_RELU: hs_launch_a16<HS_MODE_RES_RELU, 1>(f, a, n_mt, grid); return true;
        case HS_MODE_HEAD:     hs_launch_a16<HS_MODE_HEAD, 1>(f, a, n_mt, grid); return true;
        }
        return false;
    }
    if (!f.split) {              // single-pass f16 on float32 tensors: the generic epilogue only
        if (f.mode != HS_MODE_ARGS) return false;
        hs_launch<HS_MODE_ARGS, false, 0, false, false>(a, n_mt, grid, st);
        return true;
    }
    switch (f.mode) {            // the float32 tower
    case HS_MODE_ARGS:     hs_launch<HS_MODE_ARGS, true, 0, false, false>(a, n_mt, grid, st); return true;
    case HS_MODE_RELU:     hs_launch<HS_MODE_RELU, true, 0, false, false>(a, n_mt, grid, st); return true;
    case HS_MODE_RES_RELU: hs_launch<HS_MODE_RES_RELU, true, 0, false, false>(a, n_mt, grid, st); return true;
    case HS_MODE_HEAD:     hs_launch<HS_MODE_HEAD, true, 0, false, false>(a, n_mt, grid, st); return true;
    }
    return false;
}

// The full form: every image cut into blocks by conv_f16s_plan.  grid_out: the blocks launched (the training forms fold that many rows).
static int conv_f16s_launch(const ConvForm &f, int *grid_out = nullptr)
{
    const int n_images = f.n_images, height = f.a.Hd, width = f.a.Wd;
    SNK_REQUIRE(n_images >= 0 && height >= 1 && width >= 3, "%s: bad shape %d x %d x %d", f.who, n_images, height, width);
    SNK_REQUIRE(f.a.out != f.a.x, "%s: in-place convolution is not possible (blocks read their neighbours' input rows)", f.who);
    SNK_REQUIRE(f.a.out != f.a.res || f.a.res_mask, "%s: the output may overwrite the shortcut in the masked-shortcut form only", f.who);
    if (n_images == 0) return 0;
    int n_blk = 0, tiles_max = 0;
    const int rc = conv_f16s_plan(f.who, n_images, height, width, (f.io16 & 1) != 0, &n_blk, &tiles_max);
    if (rc) return rc;
    SNK_REQUIRE((long)n_images * n_blk < (1l << 31) && (long)height * width * HS_C < (1l << 31), "%s: batch too large", f.who);
    if (conv_form_check(f)) return -1;
    ConvHsArgs a = f.a;
    a.wscale_inv = (const float *)((const _Float16 *)a.wS + HS_WS_ELEMS);
    const int T = (height * width + 31) / 32, grid = n_images * n_blk;
    a.n_blk = n_blk; a.tiles_base = T / n_blk; a.tiles_rem = T % n_blk;
    a.n_img_grouped = (n_images / 8) * 8;
    SNK_REQUIRE(hs_dispatch(f, a, tiles_max, grid), "%s: no kernel is built for MODE %d, split %d, io16 %d", f.who, f.mode, f.split, f.io16);
    SNK_CHECK_HIP(hipGetLastError());
    if (grid_out) *grid_out = grid;
    return 0;
}

// ---- planning of the sub-rectangle form ------------------------------------------------------------------------------
// parts (blocks) a rectangle of hr x wr pixels is cut into and the M tiles of its largest part: the fewest parts of at most
// 8 tiles whose strip (their rows, one above, one below, halo columns) fits the LDS buffer and the staging items
// (a16: the 16-bit towers' frame -- rows pitched in bytes with a gap, six staging items)
__host__ __device__ static inline int hs_rect_parts(int hr, int wr, int Hd, int Wd, int *tiles_max, bool a16 = false)
{
    const int nst_px = 64 * (a16 ? HS_NST16 : HS_NST);
    const int T = (hr * wr + 31) / 32;
    for (int parts = (T + 7) / 8;; ++parts) {
        const int tm = (T + parts - 1) / parts;
        int rows_out = (tm * 32 + wr - 2) / wr + 1;                       // worst alignment of 32 tm pixels
        if (rows_out > hr) rows_out = hr;
        const int rows_in = rows_out + 2 < Hd ? rows_out + 2 : Hd, cols_in = wr + 2 < Wd ? wr + 2 : Wd;
        const bool fits = (a16 ? (rows_out + 2) * ((wr + 2) * HS_LDP + HS_GAP16_RECT) <= HS_BUF16 : (rows_out + 2) * (wr + 2) <= HS_NPB) &&
                          rows_in * cols_in <= nst_px;
        if (fits || tm == 1) { *tiles_max = tm; return fits ? parts : -1; }
    }
}

// bounding box of the pixels of an observation [H][W][3] that differ from the background pixel (b0, b1, b2): one wavefront
// per observation; an observation without such a pixel gets the centre pixel
__global__ __launch_bounds__(256) void k_obs_bbox(const float *__restrict__ planes, int n, int Hd, int Wd, float b0, float b1, float b2,
                                                  unsigned *__restrict__ bbox)
{
    const int img = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (img >= n) return;
    const float *x = planes + (long)img * Hd * Wd * 3;
    const float invW = 1.0f / (float)Wd;
    int y0 = 255, x0 = 255, y1 = -1, x1 = -1;
    for (int q = lane; q < Hd * Wd; q += 64) {
        const float v0 = x[3 * q], v1 = x[3 * q + 1], v2 = x[3 * q + 2];
        if (!(v0 == b0 && v1 == b1 && v2 == b2)) {
            const int y_ = (int)(((float)q + 0.5f) * invW), x_ = q - y_ * Wd;
            y0 = min(y0, y_); y1 = max(y1, y_); x0 = min(x0, x_); x1 = max(x1, x_);
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        y0 = min(y0, __shfl_xor(y0, s, 64)); x0 = min(x0, __shfl_xor(x0, s, 64));
        y1 = max(y1, __shfl_xor(y1, s, 64)); x1 = max(x1, __shfl_xor(x1, s, 64));
    }
    if (lane == 0) {
        if (y1 < 0) { y0 = y1 = Hd / 2; x0 = x1 = Wd / 2; }
        bbox[img] = (unsigned)y0 | (unsigned)x0 << 8 | (unsigned)y1 << 16 | (unsigned)x1 << 24;
    }
}

#define HS_RECT_MAX_LAYERS 24
struct RectPlanArgs {
    int n_layers;
    int grow[HS_RECT_MAX_LAYERS];          // the layer's rectangle = bounding box grown by this many pixels, cut to the canvas
    uint4 *desc;                           // [n_layers][max_blocks]
    long max_blocks;
    int *counts;                           // [n_layers][2]: descriptors written, M tiles they cover
    bool a16;                              // the descriptors are cut for the 16-bit towers' block frame
};

// One workgroup per layer: every image's rectangle -> its parts -> block descriptors, largest blocks first (bins by the
// image's largest part; the order inside a bin is whatever the atomics give -- no result depends on it)
__global__ __launch_bounds__(1024) void k_rect_plan(const unsigned *__restrict__ bbox, int n, int Hd, int Wd, RectPlanArgs a)
{
    __shared__ int cnt[9], cur[9], tiles_sum;
    const int L = blockIdx.x, g = a.grow[L], tid = threadIdx.x;
    if (tid < 9) cnt[tid] = 0;
    if (tid == 0) tiles_sum = 0;
    __syncthreads();
    int tiles = 0;
    for (int img = tid; img < n; img += 1024) {
        const unsigned b = bbox[img];
        const int y0 = max((int)(b & 255) - g, 0), x0 = max((int)((b >> 8) & 255) - g, 0);
        const int y1 = min((int)((b >> 16) & 255) + g, Hd - 1), x1 = min((int)(b >> 24) + g, Wd - 1);
        int tm;
        const int parts = hs_rect_parts(y1 - y0 + 1, x1 - x0 + 1, Hd, Wd, &tm, a.a16);
        atomicAdd(&cnt[tm], parts);
        tiles += ((y1 - y0 + 1) * (x1 - x0 + 1) + 31) / 32;
    }
    atomicAdd(&tiles_sum, tiles);
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int tm = 8; tm >= 1; --tm) { cur[tm] = o; o += cnt[tm]; }
        a.counts[2 * L] = o;
        a.counts[2 * L + 1] = tiles_sum;
    }
    __syncthreads();
    uint4 *desc = a.desc + (long)L * a.max_blocks;
    for (int img = tid; img < n; img += 1024) {
        const unsigned b = bbox[img];
        const int y0 = max((int)(b & 255) - g, 0), x0 = max((int)((b >> 8) & 255) - g, 0);
        const int y1 = min((int)((b >> 16) & 255) + g, Hd - 1), x1 = min((int)(b >> 24) + g, Wd - 1);
        const int hr = y1 - y0 + 1, wr = x1 - x0 + 1;
        int tm;
        const int parts = hs_rect_parts(hr, wr, Hd, Wd, &tm, a.a16);
        const int T = (hr * wr + 31) / 32, base = T / parts, rem = T % parts;
        const unsigned rect = (unsigned)y0 | (unsigned)x0 << 8 | (unsigned)hr << 16 | (unsigned)wr << 24;
        const int slot = atomicAdd(&cur[tm], parts);
        for (int k = 0; k < parts; ++k) {
            const int tile0 = k * base + min(k, rem), ntile = base + (k < rem ? 1 : 0);
            desc[slot + k] = make_uint4((unsigned)img, rect, (unsigned)tile0 | (unsigned)ntile << 8 | (unsigned)k << 16 | (unsigned)parts << 24, b);
        }
    }
}

static int rect_max_parts(int height, int width, bool act16)
{
    static int cache_h[2] = {0, 0}, cache_w[2] = {0, 0}, cache_v[2] = {0, 0};
    const int f = act16 ? 1 : 0;
    if (cache_h[f] == height && cache_w[f] == width) return cache_v[f];
    int worst = 1;
    for (int hr = 1; hr <= height; ++hr)
        for (int wr = 1; wr <= width; ++wr) {
            int tm;
            const int parts = hs_rect_parts(hr, wr, height, width, &tm, act16);
            if (parts < 0) return -1;
            if (parts > worst) worst = parts;
        }
    cache_h[f] = height; cache_w[f] = width; cache_v[f] = worst;
    return worst;
}

static long rect_max_blocks(int n_images, int height, int width, bool act16)
{
    if (n_images < 0 || height < 3 || width < 3 || height > 80 || width > 80) return -1;
    const int mp = rect_max_parts(height, width, act16);
    return mp < 0 ? -1 : (long)n_images * mp;
}

extern "C" long snk_conv_rect_max_blocks(int n_images, int height, int width) { return rect_max_blocks(n_images, height, width, false); }
// the towers with 16-bit activations cut rectangles for their own block frame (more pixels per LDS buffer and per staging pass)
extern "C" long snk_conv_rect_max_blocks_act16(int n_images, int height, int width) { return rect_max_blocks(n_images, height, width, true); }

static int rect_plan(const float *d_planes, float b0, float b1, float b2, int n_images, int height, int width,
                     int n_layers, const int *grow, void *d_bbox, void *d_desc, int *d_counts, void *stream, bool act16)
{
    SNK_REQUIRE(d_planes && grow && d_bbox && d_desc && d_counts, "snk_conv_rect_plan: NULL argument");
    SNK_REQUIRE(n_layers >= 1 && n_layers <= HS_RECT_MAX_LAYERS, "snk_conv_rect_plan: %d layers (at most %d)", n_layers, HS_RECT_MAX_LAYERS);
    const long mb = rect_max_blocks(n_images, height, width, act16);
    SNK_REQUIRE(mb >= 0 && mb < (1l << 31), "snk_conv_rect_plan: bad shape %d x %d x %d", n_images, height, width);
    if (n_images == 0) return 0;
    RectPlanArgs a;
    a.n_layers = n_layers;
    for (int i = 0; i < n_layers; ++i) {
        SNK_REQUIRE(grow[i] >= 0 && grow[i] < 128, "snk_conv_rect_plan: grow[%d] = %d", i, grow[i]);
        a.grow[i] = grow[i];
    }
    a.desc = (uint4 *)d_desc; a.max_blocks = mb; a.counts = d_counts;
    a.a16 = act16;
    hipStream_t st = (hipStream_t)stream;
    k_obs_bbox<<<(n_images + 3) / 4, 256, 0, st>>>(d_planes, n_images, height, width, b0, b1, b2, (unsigned *)d_bbox);
    k_rect_plan<<<n_layers, 1024, 0, st>>>((const unsigned *)d_bbox, n_images, height, width, a);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_conv_rect_plan(const float *d_planes, float b0, float b1, float b2, int n_images, int height, int width,
                                  int n_layers, const int *grow, void *d_bbox, void *d_desc, int *d_counts, void *stream)
{
    return rect_plan(d_planes, b0, b1, b2, n_images, height, width, n_layers, grow, d_bbox, d_desc, d_counts, stream, false);
}

// the plan of the towers with 16-bit activations (descriptor array: snk_conv_rect_max_blocks_act16 per layer)
extern "C" int snk_conv_rect_plan_act16(const float *d_planes, float b0, float b1, float b2, int n_images, int height, int width,
                                        int n_layers, const int *grow, void *d_bbox, void *d_desc, int *d_counts, void *stream)
{
    return rect_plan(d_planes, b0, b1, b2, n_images, height, width, n_layers, grow, d_bbox, d_desc, d_counts, stream, true);
}


// ---- the packed plan (float32-accurate tower) -------------------------------------------------------------------------
// A rectangle of h x w pixels alone pads its rows to whole M tiles: 15 x 15 = 225 = 7 x 32 + 1 runs an eighth tile for one pixel.
// Which pixels share a tile changes no result bit, so the images of a launch whose rectangles have the same SHAPE (the shape
// fixes the LDS pitch and the tap offsets; the position may differ) are given one concatenated row space, and only its end is
// padded.  The rule, stated once here for the device (k_rect_plan_pack), the host (snk_conv_rect_plan_pack_host) and the tests:
//   bin      the images of a layer by (h, w), in any order;
//   group    P = min(8, 32 / gcd(h w, 32)) consecutive images of a bin, the bin's last group whatever is left: groups are cut
//            independently of each other, so equal groups are cut alike (one thread cuts a group: short groups keep the plan kernel
//            short; 32 / gcd images would be a whole number of tiles, 8 images leave less than one tile of padding in 8 images);
//   block    hs_pack_walk: a group of one image is cut like the unpacked plan cuts a rectangle (hs_rect_parts); otherwise from the group's first unassigned pixel, the longest run of 8, 7, .. 1 tiles (or up to the group's end)
//            that touches at most two images and whose strips -- per segment its pixel rows, one above, one below, halo columns --
//            fit the LDS buffer (HS_NPB_PK pixels together) and the staging items (64 HS_NST canvas pixels together); when not even
//            one tile does (a tile would touch three images, or two strips are too wide), the block is the current image's next
//            32 pixels or its rest alone, padded: what the unpacked plan does with a tile.
// Blocks are ordered largest first over the whole layer, as in the unpacked plan.
#define HS_PACK_BINS 4096                                // (h, w) bins of a canvas the packed plan takes: up to 64 x 64
__host__ __device__ static inline bool hs_pack_fits(int wr, int Hd, int Wd, float inv, int m, int nA, int nB)
{
    const int yf = (int)(((float)m + 0.5f) * inv), yl = (int)(((float)(m + nA - 1) + 0.5f) * inv);
    const int cols_in = wr + 2 < Wd ? wr + 2 : Wd;
    int R = yl - yf + 3;
    int st = (R < Hd ? R : Hd) * cols_in;
    if (nB > 0) {
        const int RB = (int)(((float)(nB - 1) + 0.5f) * inv) + 3;
        R += RB;
        st += (RB < Hd ? RB : Hd) * cols_in;
    }
    return R * (wr + 2) <= HS_NPB_PK && st <= 64 * HS_NST;
}
// images per group of shape (hr, wr)
__host__ __device__ static inline int hs_pack_period(int S) { const int t = S | 32, P = 32 / (t & -t); return P < 8 ? P : 8; }
// emit(i, m, nA, nB, ntile): a block = pixels m .. m + nA - 1 of the group's image i, then pixels 0 .. nB - 1 of image i + 1
template <class F> __host__ __device__ static inline void hs_pack_walk(int hr, int wr, int Hd, int Wd, int q, F &&emit)
{
    const int S = hr * wr;
    if (q == 1) {                             // nothing to share tiles with: the unpacked plan's equal parts
        int tm;
        const int parts = hs_rect_parts(hr, wr, Hd, Wd, &tm), T = (S + 31) / 32, base = T / parts, rem = T % parts;
        for (int k = 0; k < parts; ++k) {
            const int tile0 = k * base + (k < rem ? k : rem), ntile = base + (k < rem ? 1 : 0);
            emit(0, 32 * tile0, 32 * (tile0 + ntile) < S ? 32 * ntile : S - 32 * tile0, 0, ntile);
        }
        return;
    }
    const float inv = 1.0f / (float)wr;
    int i = 0, m = 0;
    while (i < q) {
        const int left = (q - i) * S - m;
        const int rest = S - m;
        int nA = rest < 32 ? rest : 32, nB = 0;
        for (int n = 8; n >= 1; --n) {
            const int rows = 32 * n < left ? 32 * n : left;
            const int a_ = rows < rest ? rows : rest, b_ = rows - a_;
            if (b_ <= S && hs_pack_fits(wr, Hd, Wd, inv, m, a_, b_)) { nA = a_; nB = b_; break; }
        }
        emit(i, m, nA, nB, (nA + nB + 31) / 32);
        m += nA;
        if (m == S) { ++i; m = nB; if (m == S) { ++i; m = 0; } }
    }
}

// One workgroup per layer.  Images -> bins (shared-memory histogram, block scan, counting sort into d_order), then every group
// is walked twice by one thread: once to count the blocks of each size (the descriptor array is ordered by size), once to write
// them -- with the images still named by their place in d_order, which k_rect_pack_resolve (all layers, one thread per block)
// turns into image, rectangle and bounding box: the walk itself waits for no load.
__global__ __launch_bounds__(1024) void k_rect_plan_pack(const unsigned *__restrict__ bbox, int n, int Hd, int Wd, RectPlanArgs a,
                                                         int *__restrict__ order_all)
{
    __shared__ int cnt[HS_PACK_BINS], cur[HS_PACK_BINS], gb[HS_PACK_BINS + 1];
    __shared__ unsigned long long sc[1024];
    __shared__ int cls[9], clscur[9], tiles_sum;
    const int L = blockIdx.x, g = a.grow[L], tid = threadIdx.x, nb = Hd * Wd;
    int *order = order_all + (long)L * n;
    for (int b = tid; b < nb; b += 1024) cnt[b] = 0;
    if (tid < 9) cls[tid] = 0;
    if (tid == 0) tiles_sum = 0;
    __syncthreads();
#define HS_PACK_SHAPE(b_)                                                                       \
        const int y0 = max((int)((b_) & 255) - g, 0), x0 = max((int)(((b_) >> 8) & 255) - g, 0); \
        const int y1 = min((int)(((b_) >> 16) & 255) + g, Hd - 1), x1 = min((int)((b_) >> 24) + g, Wd - 1); \
        const int hr = y1 - y0 + 1, wr = x1 - x0 + 1, bin = (hr - 1) * Wd + wr - 1;
    for (int img = tid; img < n; img += 1024) {
        const unsigned b = bbox[img];
        HS_PACK_SHAPE(b)
        (void)y0; (void)x0;
        atomicAdd(&cnt[bin], 1);
    }
    __syncthreads();
    // exclusive scan over the bins of (images, groups): K consecutive bins per thread
    const int K = (nb + 1023) / 1024;
    unsigned long long mine = 0;
    for (int j = 0; j < K; ++j) {
        const int b = tid * K + j;
        if (b < nb && cnt[b] > 0) {
            const int P = hs_pack_period((b / Wd + 1) * (b % Wd + 1));
            mine += (unsigned long long)cnt[b] << 32 | (unsigned)((cnt[b] + P - 1) / P);
        }
    }
    sc[tid] = mine;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {
        const unsigned long long v = tid >= s ? sc[tid - s] : 0ull;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    {
        unsigned long long e = sc[tid] - mine;
        for (int j = 0; j < K; ++j) {
            const int b = tid * K + j;
            if (b < nb) {
                cur[b] = (int)(e >> 32); gb[b] = (int)(e & 0xFFFFFFFFu);
                if (cnt[b] > 0) {
                    const int P = hs_pack_period((b / Wd + 1) * (b % Wd + 1));
                    e += (unsigned long long)cnt[b] << 32 | (unsigned)((cnt[b] + P - 1) / P);
                }
            }
        }
    }
    const int n_groups = (int)(sc[1023] & 0xFFFFFFFFu);
    if (tid == 0) gb[nb] = n_groups;
    __syncthreads();
    for (int img = tid; img < n; img += 1024) {           // counting sort: the bin's images side by side (in the atomics' order)
        const unsigned b = bbox[img];
        HS_PACK_SHAPE(b)
        (void)y0; (void)x0;
        order[atomicAdd(&cur[bin], 1)] = img;
    }
#undef HS_PACK_SHAPE
    // group gi -> its bin (the last b with gb[b] <= gi: empty bins share the value of the bin after them), place and size
#define HS_PACK_GROUP(gi)                                                                       \
        int lo_ = 0, hi_ = nb;                /* first index whose gb exceeds gi */                \
        while (lo_ < hi_) { const int mid_ = (lo_ + hi_) >> 1; if (gb[mid_ + 1] > (gi)) hi_ = mid_; else lo_ = mid_ + 1; } \
        const int bin = lo_, hr = bin / Wd + 1, wr = bin % Wd + 1, P = hs_pack_period(hr * wr);  \
        const int rank0 = ((gi) - gb[bin]) * P, q = min(P, cnt[bin] - rank0);
    int tiles = 0;
    for (int gi = tid; gi < n_groups; gi += 1024) {
        HS_PACK_GROUP(gi)
        hs_pack_walk(hr, wr, Hd, Wd, q, [&](int, int, int, int, int nt) { atomicAdd(&cls[nt], 1); tiles += nt; });
    }
    atomicAdd(&tiles_sum, tiles);
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int nt = 8; nt >= 1; --nt) { clscur[nt] = o; o += cls[nt]; }
        a.counts[2 * L] = 2 * o;
        a.counts[2 * L + 1] = tiles_sum;
    }
    __syncthreads();
    uint4 *desc = a.desc + (long)L * a.max_blocks;
    for (int gi = tid; gi < n_groups; gi += 1024) {
        HS_PACK_GROUP(gi)
        const int first = cur[bin] - cnt[bin] + rank0;     // (the sort left cur at the bin's end)
        hs_pack_walk(hr, wr, Hd, Wd, q, [&](int i, int m, int nA, int nB, int nt) {
            const int slot = atomicAdd(&clscur[nt], 1);
            desc[2 * slot] = make_uint4((unsigned)(first + i), 0u, (unsigned)m | (unsigned)nA << 16, 0u);
            desc[2 * slot + 1] = make_uint4((unsigned)(first + i + (nB > 0 ? 1 : 0)), 0u, (unsigned)nB | (unsigned)nt << 16, 0u);
        });
    }
#undef HS_PACK_GROUP
}

// places in d_order -> image, rectangle, bounding box: one thread per 16-byte entry of every layer
__global__ __launch_bounds__(256) void k_rect_pack_resolve(const unsigned *__restrict__ bbox, int n, int Hd, int Wd, RectPlanArgs a,
                                                           const int *__restrict__ order_all)
{
    const int L = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x, g = a.grow[L];
    if (e >= a.counts[2 * L]) return;
    uint4 *d = a.desc + (long)L * a.max_blocks + e;
    const int img = order_all[(long)L * n + (int)d->x];
    const unsigned b = bbox[img];
    const int y0 = max((int)(b & 255) - g, 0), x0 = max((int)((b >> 8) & 255) - g, 0);
    const int y1 = min((int)((b >> 16) & 255) + g, Hd - 1), x1 = min((int)(b >> 24) + g, Wd - 1);
    d->x = (unsigned)img;
    d->y = (unsigned)y0 | (unsigned)x0 << 8 | (unsigned)(y1 - y0 + 1) << 16 | (unsigned)(x1 - x0 + 1) << 24;
    d->w = b;
}

// 16-byte descriptor entries per layer the packed plan may write for n_images observations: two per block, blocks per image at
// most the worst ratio over every shape and group size (each bin's groups are cut alike, its last group is one of the sizes)
static long rect_pack_max_desc(int n_images, int height, int width)
{
    if (n_images < 0 || height < 3 || width < 3 || height * width > HS_PACK_BINS) return -1;
    if (rect_max_parts(height, width, false) < 0) return -1;
    static int cache_h = 0, cache_w = 0;
    static double cache_r = 0.0;
    if (cache_h != height || cache_w != width) {
        double worst = 1.0;
        for (int hr = 1; hr <= height; ++hr)
            for (int wr = 1; wr <= width; ++wr) {
                const int P = hs_pack_period(hr * wr);
                int tm;
                const int alone = hs_rect_parts(hr, wr, height, width, &tm);       // a group of one image
                if ((double)alone > worst) worst = (double)alone;
                if (P == 1) continue;
                // a group of q images is cut like the first q of P images, except that its last block stops at the group's end
                // (a shorter second segment always fits): it has at most the blocks of the P-walk up to the one that ends image q - 1
                int blocks = 0, done = 0;
                const int S = hr * wr;
                hs_pack_walk(hr, wr, height, width, P, [&](int i, int m, int nA, int nB, int) {
                    ++blocks;
                    const int upto = m + nA == S ? i + (nB == S ? 1 : 0) : -1;      // the last image this block ends
                    for (; done <= upto && done < P; ++done) {       // a group of done + 1 >= 2 images has at most this many blocks
                        const double r = (double)blocks / (double)(done + 1);
                        if (r > worst) worst = r;
                    }
                });
            }
        cache_h = height; cache_w = width; cache_r = worst;
    }
    return 2 * ((long)((double)n_images * cache_r) + 1);
}

extern "C" long snk_conv_rect_pack_max_desc(int n_images, int height, int width) { return rect_pack_max_desc(n_images, height, width); }

extern "C" int snk_conv_rect_plan_pack(const float *d_planes, float b0, float b1, float b2, int n_images, int height, int width,
                                       int n_layers, const int *grow, void *d_bbox, void *d_desc, int *d_counts, void *d_order, void *stream)
{
    SNK_REQUIRE(d_planes && grow && d_bbox && d_desc && d_counts && d_order, "snk_conv_rect_plan_pack: NULL argument");
    SNK_REQUIRE(n_layers >= 1 && n_layers <= HS_RECT_MAX_LAYERS, "snk_conv_rect_plan_pack: %d layers (at most %d)", n_layers, HS_RECT_MAX_LAYERS);
    const long md = rect_pack_max_desc(n_images, height, width);
    SNK_REQUIRE(md >= 0 && md < (1l << 31), "snk_conv_rect_plan_pack: bad shape %d x %d x %d", n_images, height, width);
    if (n_images == 0) return 0;
    RectPlanArgs a;
    a.n_layers = n_layers;
    for (int i = 0; i < n_layers; ++i) {
        SNK_REQUIRE(grow[i] >= 0 && grow[i] < 128, "snk_conv_rect_plan_pack: grow[%d] = %d", i, grow[i]);
        a.grow[i] = grow[i];
    }
    a.desc = (uint4 *)d_desc; a.max_blocks = md; a.counts = d_counts;
    a.a16 = false;
    hipStream_t st = (hipStream_t)stream;
    k_obs_bbox<<<(n_images + 3) / 4, 256, 0, st>>>(d_planes, n_images, height, width, b0, b1, b2, (unsigned *)d_bbox);
    k_rect_plan_pack<<<n_layers, 1024, 0, st>>>((const unsigned *)d_bbox, n_images, height, width, a, (int *)d_order);
    k_rect_pack_resolve<<<dim3((unsigned)((md + 255) / 256), n_layers), 256, 0, st>>>((const unsigned *)d_bbox, n_images, height, width, a, (const int *)d_order);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

// The same rule on the host, one layer, from given bounding boxes (y0 | x0 << 8 | y1 << 16 | x1 << 24): descriptors in the
// device format (bins in shape order, a bin's images in index order; largest blocks first, otherwise in that order), h_counts =
// { 16-byte entries, M tiles }.  h_desc: snk_conv_rect_pack_max_desc(n_images, height, width) entries.  No GPU involved.
extern "C" int snk_conv_rect_plan_pack_host(const unsigned *h_bbox, int n_images, int height, int width, int grow,
                                            unsigned *h_desc, int *h_counts)
{
    SNK_REQUIRE(h_bbox && h_desc && h_counts, "snk_conv_rect_plan_pack_host: NULL argument");
    SNK_REQUIRE(grow >= 0 && grow < 128, "snk_conv_rect_plan_pack_host: grow = %d", grow);
    const long md = rect_pack_max_desc(n_images, height, width);
    SNK_REQUIRE(md >= 0 && md < (1l << 31), "snk_conv_rect_plan_pack_host: bad shape %d x %d x %d", n_images, height, width);
    const int nb = height * width;
    int *binof = (int *)malloc(sizeof(int) * (size_t)(n_images + 1)), *start = (int *)calloc((size_t)nb + 2, sizeof(int));
    int *order = (int *)malloc(sizeof(int) * (size_t)(n_images + 1));
    unsigned *rect = (unsigned *)malloc(sizeof(unsigned) * (size_t)(n_images + 1));
    unsigned *tmp = (unsigned *)malloc(16 * (size_t)(md + 2));
    long n_blk = 0, tiles = 0;
    bool ok = binof && start && order && rect && tmp;
    if (ok) {
        for (int i = 0; i < n_images; ++i) {
            const unsigned b = h_bbox[i];
            const int y0 = (int)(b & 255) - grow > 0 ? (int)(b & 255) - grow : 0, x0 = (int)((b >> 8) & 255) - grow > 0 ? (int)((b >> 8) & 255) - grow : 0;
            const int y1 = (int)((b >> 16) & 255) + grow < height - 1 ? (int)((b >> 16) & 255) + grow : height - 1;
            const int x1 = (int)(b >> 24) + grow < width - 1 ? (int)(b >> 24) + grow : width - 1;
            if (y1 < y0 || x1 < x0) { ok = false; break; }
            binof[i] = (y1 - y0) * width + x1 - x0;
            rect[i] = (unsigned)y0 | (unsigned)x0 << 8 | (unsigned)(y1 - y0 + 1) << 16 | (unsigned)(x1 - x0 + 1) << 24;
            ++start[binof[i] + 1];
        }
    }
    if (ok) {
        for (int b = 0; b < nb; ++b) start[b + 1] += start[b];
        for (int i = 0; i < n_images; ++i) order[start[binof[i]]++] = i;      // (start[b] is now the bin's end)
        int at = 0;
        for (int b = 0; b < nb && ok; ++b) {
            const int cntb = start[b] - at, hr = b / width + 1, wr = b % width + 1, P = hs_pack_period(hr * wr);
            for (int r0 = 0; r0 < cntb; r0 += P) {
                const int first = at + r0;
                hs_pack_walk(hr, wr, height, width, cntb - r0 < P ? cntb - r0 : P, [&](int i, int m, int nA, int nB, int nt) {
                    if (2 * (n_blk + 1) > md) { ok = false; return; }
                    const int ia = order[first + i], ib = order[first + i + (nB > 0 ? 1 : 0)];
                    unsigned *d = tmp + 8 * n_blk++;
                    d[0] = (unsigned)ia; d[1] = rect[ia]; d[2] = (unsigned)m | (unsigned)nA << 16; d[3] = h_bbox[ia];
                    d[4] = (unsigned)ib; d[5] = rect[ib]; d[6] = (unsigned)nB | (unsigned)nt << 16; d[7] = h_bbox[ib];
                    tiles += nt;
                });
            }
            at = start[b];
        }
    }
    if (ok) {
        long o = 0;
        for (int nt = 8; nt >= 1; --nt)
            for (long k = 0; k < n_blk; ++k)
                if ((int)((tmp[8 * k + 6] >> 16) & 15) == nt) { for (int j = 0; j < 8; ++j) h_desc[8 * o + j] = tmp[8 * k + j]; ++o; }
        h_counts[0] = (int)(2 * n_blk);
        h_counts[1] = (int)tiles;
    }
    free(binof); free(start); free(order); free(rect); free(tmp);
    SNK_REQUIRE(ok, "snk_conv_rect_plan_pack_host: bad bounding box, out of memory or more blocks than snk_conv_rect_pack_max_desc allows");
    return 0;
}

// the frames the sub-rectangle kernels are built in: the float32 tower (split) and the three 16-bit towers (16-bit in and out)
template <int MODE> static void hs_launch_rect(const ConvForm &f, const ConvHsArgs &a, bool pack, int grid)
{
    hipStream_t st = (hipStream_t)f.stream;
    if (pack) k_conv3x3_f16s_rectp<MODE><<<grid, 256, 0, st>>>(a);
    else if (f.mx) k_conv3x3_f16s_rect<MODE, false, 3, true, true><<<grid, 256, 0, st>>>(a);
    else if (f.bf) k_conv3x3_f16s_rect<MODE, false, 3, true, false><<<grid, 256, 0, st>>>(a);
    else if (f.io16) k_conv3x3_f16s_rect<MODE, false, 3, false, false><<<grid, 256, 0, st>>>(a);
    else k_conv3x3_f16s_rect<MODE, true, 0, false, false><<<grid, 256, 0, st>>>(a);
}

// The sub-rectangle forms: one block per descriptor of a.desc -- snk_conv_rect_plan's, or (pack) snk_conv_rect_plan_pack's.
static int conv_f16s_rect_launch(const ConvForm &f, bool pack = false)
{
    const char *who = f.who;
    const int n_images = f.n_images, height = f.a.Hd, width = f.a.Wd;
    SNK_REQUIRE(f.a.grow_in >= 0 && f.a.grow_in < 128 && f.a.grow_res >= 0 && f.a.grow_res < 128, "%s: grow_in %d, grow_res %d", who,
                f.a.grow_in, f.a.grow_res);
    SNK_REQUIRE(f.a.x && f.a.wS && f.a.scale && f.a.shift && f.a.out && f.a.desc && f.a.n_desc, "%s: NULL argument", who);
    SNK_REQUIRE(f.a.out != f.a.x, "%s: in-place convolution is not possible", who);
    // grid: the most blocks the plan can have written; (packed: a row's offset into the tensors carries its image: the whole
    // batch must stay below 2^31 elements)
    const long mb = pack ? rect_pack_max_desc(n_images, height, width) : rect_max_blocks(n_images, height, width, f.io16 != 0);
    SNK_REQUIRE(mb >= 0 && mb < (1l << 31) && (long)(pack ? n_images : 1) * height * width * HS_C < (1l << 31), "%s: bad shape %d x %d x %d",
                who, n_images, height, width);
    if (n_images == 0) return 0;
    SNK_REQUIRE(f.mode == (f.a.res ? HS_MODE_RES_RELU : HS_MODE_RELU) && (f.io16 ? f.io16 == 3 && !f.split && !pack : f.split && !f.bf) &&
                (!f.mx || f.bf), "%s: no sub-rectangle kernel is built for MODE %d, split %d, io16 %d", who, f.mode, f.split, f.io16);
    ConvHsArgs a = f.a;
    a.wscale_inv = (const float *)((const _Float16 *)a.wS + HS_WS_ELEMS);
    a.n_blk = 1; a.relu = 1;
    if (!a.res) a.bg_res = nullptr;
    const int grid = (int)(pack ? mb / 2 : mb);
    if (f.mode == HS_MODE_RES_RELU) hs_launch_rect<HS_MODE_RES_RELU>(f, a, pack, grid);
    else hs_launch_rect<HS_MODE_RELU>(f, a, pack, grid);
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

// the argument list the five sub-rectangle entry points share, by name
static ConvForm conv_rect_form(const char *who, const void *d_x, const void *d_wS, const float *d_scale, const float *d_shift,
                               const void *d_residual, void *d_out, const void *d_desc, const int *d_count, const void *d_bg_in,
                               int grow_in, const void *d_bg_res, int grow_res, const void *d_bg_out, int n_images, int height,
                               int width, void *stream)
{
    ConvForm f = conv_form(who, d_residual ? HS_MODE_RES_RELU : HS_MODE_RELU, d_x, d_wS, n_images, height, width, stream);
    f.a.scale = d_scale; f.a.shift = d_shift; f.a.res = (const float *)d_residual; f.a.out = (float *)d_out;
    f.a.desc = (const uint4 *)d_desc; f.a.n_desc = d_count;
    f.a.bg_in = (const float *)d_bg_in; f.a.grow_in = grow_in;
    f.a.bg_res = (const float *)d_bg_res; f.a.grow_res = grow_res;
    f.a.bg_out = (const float *)d_bg_out;
    return f;
}

extern "C" int snk_conv3x3_bn_f16s_rect(const float *d_x, const void *d_wS, const float *d_scale, const float *d_shift,
                                        const float *d_residual, float *d_out, const void *d_desc, const int *d_count,
                                        const float *d_bg_in, int grow_in, const float *d_bg_res, int grow_res,
                                        const float *d_bg_out, int n_images, int height, int width, void *stream)
{
    return conv_f16s_rect_launch(conv_rect_form("snk_conv3x3_bn_f16s_rect", d_x, d_wS, d_scale, d_shift, d_residual, d_out, d_desc, d_count,
                                                d_bg_in, grow_in, d_bg_res, grow_res, d_bg_out, n_images, height, width, stream));
}

// snk_conv3x3_bn_f16s_rect on the packed plan's descriptors (snk_conv_rect_plan_pack)
extern "C" int snk_conv3x3_bn_f16s_rect_pack(const float *d_x, const void *d_wS, const float *d_scale, const float *d_shift,
                                             const float *d_residual, float *d_out, const void *d_desc, const int *d_count,
                                             const float *d_bg_in, int grow_in, const float *d_bg_res, int grow_res,
                                             const float *d_bg_out, int n_images, int height, int width, void *stream)
{
    return conv_f16s_rect_launch(conv_rect_form("snk_conv3x3_bn_f16s_rect_pack", d_x, d_wS, d_scale, d_shift, d_residual, d_out, d_desc,
                                                d_count, d_bg_in, grow_in, d_bg_res, grow_res, d_bg_out, n_images, height, width, stream),
                                 true);
}

// the frame of the 16-bit towers' sub-rectangle layers: 16-bit activations in and out
static ConvForm conv_rect_form16(ConvForm f, bool bf, bool mx) { f.split = false; f.io16 = 3; f.bf = bf; f.mx = mx; return f; }

// the sub-rectangle form of snk_conv3x3_bn_f16_act16 (f16 activations in and out, relu = 1; the background images are f16
// [height][width][128])
extern "C" int snk_conv3x3_bn_f16_act16_rect(const void *d_x16, const void *d_wS, const float *d_scale, const float *d_shift,
                                             const void *d_residual16, void *d_out16, const void *d_desc, const int *d_count,
                                             const void *d_bg_in16, int grow_in, const void *d_bg_res16, int grow_res,
                                             const void *d_bg_out16, int n_images, int height, int width, void *stream)
{
    return conv_f16s_rect_launch(conv_rect_form16(conv_rect_form("snk_conv3x3_bn_f16_act16_rect", d_x16, d_wS, d_scale, d_shift, d_residual16,
                                                                 d_out16, d_desc, d_count, d_bg_in16, grow_in, d_bg_res16, grow_res, d_bg_out16,
                                                                 n_images, height, width, stream), false, false));
}

// the same for the bf16 tower (bf16 activations in and out, bf16 background images, weights = snk_conv3x3_prepare_weights_bf16)
extern "C" int snk_conv3x3_bn_bf16_act16_rect(const void *d_x16, const void *d_wS, const float *d_scale, const float *d_shift,
                                              const void *d_residual16, void *d_out16, const void *d_desc, const int *d_count,
                                              const void *d_bg_in16, int grow_in, const void *d_bg_res16, int grow_res,
                                              const void *d_bg_out16, int n_images, int height, int width, void *stream)
{
    return conv_f16s_rect_launch(conv_rect_form16(conv_rect_form("snk_conv3x3_bn_bf16_act16_rect", d_x16, d_wS, d_scale, d_shift, d_residual16,
                                                                 d_out16, d_desc, d_count, d_bg_in16, grow_in, d_bg_res16, grow_res, d_bg_out16,
                                                                 n_images, height, width, stream), true, false));
}

// the argument list the inference entry points of the full form share, by name (d_out: NULL where only the fused head's output is wanted)
static ConvForm conv_bn_form(const char *who, int mode, const void *d_x, const void *d_wS, const float *d_scale, const float *d_shift,
                             const void *d_residual, void *d_out, int relu, int n_images, int height, int width, void *stream)
{
    ConvForm f = conv_form(who, mode, d_x, d_wS, n_images, height, width, stream);
    f.a.scale = d_scale; f.a.shift = d_shift; f.a.res = (const float *)d_residual; f.a.out = (float *)d_out; f.a.relu = relu;
    return f;
}

// the head's 1x1 stage in the layer's epilogue
static void conv_form_head(ConvForm &f, const float *d_w1x1, float bn_scale, float bn_shift, float *d_h1)
{
    f.a.w1x1 = d_w1x1; f.a.s1 = bn_scale; f.a.b1 = bn_shift; f.a.h1 = d_h1;
}

// the frame of the 16-bit towers' full layers: 16-bit activations in; out16: 16-bit out as well
static void conv_form_a16(ConvForm &f, bool out16, bool bf, bool mx) { f.split = false; f.io16 = out16 ? 3 : 1; f.bf = bf; f.mx = mx; }

extern "C" int snk_conv3x3_bn_f16s(const float *d_x, const void *d_wS, const float *d_scale, const float *d_shift,
                                   const float *d_residual, float *d_out, int n_images, int height, int width, int relu,
                                   void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_scale && d_shift && d_out, "snk_conv3x3_bn_f16s: NULL argument");
    return conv_f16s_launch(conv_bn_form("snk_conv3x3_bn_f16s", hs_tower_mode(relu, d_residual), d_x, d_wS, d_scale, d_shift, d_residual,
                                         d_out, relu, n_images, height, width, stream));
}

// (single-pass f16 on float32 tensors: the generic epilogue is the only one built)
extern "C" int snk_conv3x3_bn_f16(const float *d_x, const void *d_wS, const float *d_scale, const float *d_shift,
                                  const float *d_residual, float *d_out, int n_images, int height, int width, int relu,
                                  void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_scale && d_shift && d_out, "snk_conv3x3_bn_f16: NULL argument");
    ConvForm f = conv_bn_form("snk_conv3x3_bn_f16", HS_MODE_ARGS, d_x, d_wS, d_scale, d_shift, d_residual, d_out, relu, n_images, height,
                              width, stream);
    f.split = false;
    return conv_f16s_launch(f);
}

// (the compile-time epilogue where the layer closes a residual block and writes no output of its own; the generic one otherwise)
extern "C" int snk_conv3x3_bn_f16s_head(const float *d_x, const void *d_wS, const float *d_scale, const float *d_shift,
                                        const float *d_residual, float *d_out, const float *d_w1x1, float bn_scale,
                                        float bn_shift, float *d_h1, int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_scale && d_shift && d_w1x1 && d_h1, "snk_conv3x3_bn_f16s_head: NULL argument");
    ConvForm f = conv_bn_form("snk_conv3x3_bn_f16s_head", d_residual && !d_out ? HS_MODE_HEAD : HS_MODE_ARGS, d_x, d_wS, d_scale, d_shift,
                              d_residual, d_out, 1, n_images, height, width, stream);
    conv_form_head(f, d_w1x1, bn_scale, bn_shift, d_h1);
    return conv_f16s_launch(f);
}

// The training step's forward convolution: d_out = conv3x3_same(d_x, w) (no batch norm, no ReLU) and, from the same values on
// their way out, d_sums[0..127] = sum over all pixels of (out - center), d_sums[128..255] = sum of (out - center)^2 (float64;
// d_center: 128 floats or NULL) -- what snk_bn_train_sums_f64 would compute from d_out in a pass of its own.
// d_partials: snk_conv3x3_stats_partials(n_images, height, width) floats.
#define HS_AMAX_STAGE 64                                 // rows the first of the two maximum folds leaves
extern "C" long snk_conv3x3_stats_partials(int n_images, int height, int width)
{
    if (n_images <= 0 || height < 1 || width < 3) return -1;
    const long T = ((long)height * width + 31) / 32;
    // at most one block per M tile: 2 x 128 sums + 128 maxima each; the two folds' scratch
    return (long)n_images * T * 384 + TF_SCRATCH_FLOATS(256) + HS_AMAX_STAGE * HS_C;
}

// per-channel maximum over the blocks' maxima: [n_rows][128] -> [gridDim.x][128] (whole 512-byte rows per eight-lane group, block b
// takes rows b, b + gridDim.x, ..); run twice: the blocks' maxima -> 64 rows -> 1
__global__ __launch_bounds__(256) void k_amax_fold128(const float *__restrict__ part, int n_rows, float *__restrict__ out)
{
    __shared__ float4 sh[8][32];
    const int cq = threadIdx.x & 31, rl = threadIdx.x >> 5;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = blockIdx.x * 8 + rl; r < n_rows; r += gridDim.x * 8) {
        const float4 v = *(const float4 *)(part + (size_t)r * HS_C + 4 * cq);
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
    sh[rl][cq] = m;
    __syncthreads();
    if (rl == 0) {
#pragma unroll
        for (int r = 1; r < 8; ++r) { const float4 v = sh[r][cq]; m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w); }
        *(float4 *)(out + (size_t)blockIdx.x * HS_C + 4 * cq) = m;
    }
}

// what the training entry points share, by name: bare convolutions on float32 tensors (d_center: the centre of the sums, or the
// mean of the layer below for the input-gradient forms); split = false: the single-pass f16 form
static ConvForm conv_train_form(const char *who, int mode, bool split, const float *d_x, const void *d_wS, const float *d_residual,
                                float *d_out, const float *d_center, int n_images, int height, int width, void *stream)
{
    ConvForm f = conv_form(who, mode, d_x, d_wS, n_images, height, width, stream);
    f.split = split;
    f.a.res = d_residual; f.a.out = d_out; f.a.center = d_center;
    return f;
}

// The launch of a training form, the fold of its blocks' sums into d_sums and, where d_amax is given, of their maxima into d_amax.
static int conv_train(ConvForm f, float *d_partials, double *d_sums, float *d_amax = nullptr)
{
    // the launch's grid is known only inside: the maxima sit behind the largest sums + fold scratch the buffer is sized for
    const long T = ((long)f.a.Hd * f.a.Wd + 31) / 32;
    f.a.stat_part = d_partials;
    f.a.amax_part = d_amax ? d_partials + (long)f.n_images * T * 256 + TF_SCRATCH_FLOATS(256) : nullptr;
    int grid = 0;
    const int rc = conv_f16s_launch(f, &grid);
    if (rc) return rc;
    tf_fold<double>(d_partials, grid, 256, 256, 1.0, d_sums, (double *)(d_partials + (long)grid * 256), (hipStream_t)f.stream);
    if (d_amax) {
        float *stage = d_partials + (long)f.n_images * T * 384 + TF_SCRATCH_FLOATS(256);
        k_amax_fold128<<<HS_AMAX_STAGE, 256, 0, (hipStream_t)f.stream>>>(f.a.amax_part, grid, stage);
        k_amax_fold128<<<1, 256, 0, (hipStream_t)f.stream>>>(stage, HS_AMAX_STAGE, d_amax);
    }
    SNK_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int snk_conv3x3_f16s_stats(const float *d_x, const void *d_wS, float *d_out, const float *d_center, float *d_partials,
                                      double *d_sums, int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_out && d_partials && d_sums && n_images > 0, "snk_conv3x3_f16s_stats: bad argument");
    return conv_train(conv_train_form("snk_conv3x3_f16s_stats", HS_MODE_STATS, true, d_x, d_wS, nullptr, d_out, d_center, n_images, height,
                                      width, stream), d_partials, d_sums);
}

// ---- the training step's single-pass f16 mode (TrainStep(conv="f16"), SNK_TRAIN_CONV=f16) -------------------------------------------
// The snk_conv3x3_f16_* entry points take the argument lists, weight images and scale tails of their snk_conv3x3_f16s_* namesakes
// and run the same block frames with SPLIT = false: one MFMA per product.  The arithmetic rule (include/snake_engine.h, DESIGN.md
// section 4, tests/test_train_f16_gpu.py state the same one): an operand v enters the MFMA as f16(v * s), round to nearest even, s
// the power of two the split form uses for that tensor (the image's tail); beyond +-65504 after scaling it is clamped and the
// layer's range flag raised, as in the split form; products are exact in float32, sums are float32, the result is multiplied by
// the inverse scales.  Nothing else is rounded to 16 bits: every tensor in HBM stays float32.  The weight image is the split
// image: its hi fragments are 1 KB runs of their own, so a wave that skips the lo runs streams exactly a hi-only image's bytes.
extern "C" int snk_conv3x3_f16_stats(const float *d_x, const void *d_wS, float *d_out, const float *d_center, float *d_partials,
                                     double *d_sums, int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_out && d_partials && d_sums && n_images > 0, "snk_conv3x3_f16_stats: bad argument");
    return conv_train(conv_train_form("snk_conv3x3_f16_stats", HS_MODE_STATS, false, d_x, d_wS, nullptr, d_out, d_center, n_images, height,
                                      width, stream), d_partials, d_sums);
}

// The same with the two options of the deferred batch norm (snake_engine/train_step.py: the activation between the two convolutions
// of a residual block is never written out):
//   d_in_scale / d_in_shift (both or neither): d_x is the PRE-batch-norm output of the layer below and every value is taken as
//     relu(x * in_scale[c] + in_shift[c]) on its way into the kernel -- bit for bit what snk_bn_train_apply(relu = 1, no residual)
//     would have written; the input scale in d_wS's tail must cover that range (snk_bn_train_finalize_range);
//   d_amax (or NULL; with either input form): 128 floats, the largest |out - center| per channel -- what snk_bn_train_finalize_range turns into the
//     range of this layer's own batch norm + ReLU output without a pass over it.
static int hs_stats_mode(const float *d_in_scale, const float *d_amax)
{
    return !d_in_scale ? HS_MODE_STATS : d_amax ? HS_MODE_STATS_AFF_AMAX : HS_MODE_STATS_AFF;
}

extern "C" int snk_conv3x3_f16s_stats_deferred(const float *d_x, const void *d_wS, float *d_out, const float *d_center,
                                               const float *d_in_scale, const float *d_in_shift, float *d_amax, float *d_partials,
                                               double *d_sums, int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_out && d_partials && d_sums && n_images > 0 && !d_in_scale == !d_in_shift,
                "snk_conv3x3_f16s_stats_deferred: bad argument");
    ConvForm f = conv_train_form("snk_conv3x3_f16s_stats_deferred", hs_stats_mode(d_in_scale, d_amax), true, d_x, d_wS, nullptr, d_out,
                                 d_center, n_images, height, width, stream);
    f.a.aff_scale = d_in_scale; f.a.aff_shift = d_in_shift;
    return conv_train(f, d_partials, d_sums, d_amax);
}

extern "C" int snk_conv3x3_f16_stats_deferred(const float *d_x, const void *d_wS, float *d_out, const float *d_center,
                                              const float *d_in_scale, const float *d_in_shift, float *d_amax, float *d_partials,
                                              double *d_sums, int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_out && d_partials && d_sums && n_images > 0 && !d_in_scale == !d_in_shift,
                "snk_conv3x3_f16_stats_deferred: bad argument");
    ConvForm f = conv_train_form("snk_conv3x3_f16_stats_deferred", hs_stats_mode(d_in_scale, d_amax), false, d_x, d_wS, nullptr, d_out,
                                 d_center, n_images, height, width, stream);
    f.a.aff_scale = d_in_scale; f.a.aff_shift = d_in_shift;
    return conv_train(f, d_partials, d_sums, d_amax);
}

// reduced precision with f16 activations in HBM (BASELINE configs[4]): d_x16 / d_residual16 are f16 [n][H][W][128]; the output
// is f16 (out_f16 != 0: every tower layer but the last) or float32 (the layer the head reads).  Weights: the image
// snk_conv3x3_prepare_weights_f16s makes with x_scale = 1.
extern "C" int snk_conv3x3_bn_f16_act16(const void *d_x16, const void *d_wS, const float *d_scale, const float *d_shift,
                                        const void *d_residual16, void *d_out, int out_f16, int n_images, int height, int width,
                                        int relu, void *stream)
{
    SNK_REQUIRE(d_x16 && d_wS && d_scale && d_shift && d_out, "snk_conv3x3_bn_f16_act16: NULL argument");
    ConvForm f = conv_bn_form("snk_conv3x3_bn_f16_act16", hs_tower_mode(relu, d_residual16), d_x16, d_wS, d_scale, d_shift, d_residual16,
                              d_out, relu, n_images, height, width, stream);
    conv_form_a16(f, out_f16 != 0, false, false);
    return conv_f16s_launch(f);
}

// BASELINE configs[4] as it is worded, "bf16 MFMA conv": bf16 activations in HBM (d_x16 / d_residual16: bf16 [n][H][W][128]; the
// output is bf16, or float32 for the layer the head reads), bf16 weights (snk_conv3x3_prepare_weights_bf16), products on
// v_mfma_f32_32x32x16_bf16, float32 accumulation, batch norm / shortcut / ReLU in float32.  The block body is hs_block: the same
// staging, LDS image, fragment pipeline and epilogue as the f16-activation tower.
extern "C" int snk_conv3x3_bn_bf16_act16(const void *d_x16, const void *d_wS, const float *d_scale, const float *d_shift,
                                         const void *d_residual16, void *d_out, int out_bf16, int n_images, int height, int width,
                                         int relu, void *stream)
{
    SNK_REQUIRE(d_x16 && d_wS && d_scale && d_shift && d_out, "snk_conv3x3_bn_bf16_act16: NULL argument");
    ConvForm f = conv_bn_form("snk_conv3x3_bn_bf16_act16", hs_tower_mode(relu, d_residual16), d_x16, d_wS, d_scale, d_shift, d_residual16,
                              d_out, relu, n_images, height, width, stream);
    conv_form_a16(f, out_bf16 != 0, true, false);
    return conv_f16s_launch(f);
}

// The last layer of the towers with 16-bit activations with the head's 1x1 stage in its epilogue (alpha_nnet.py:46-50), as
// snk_conv3x3_bn_f16s_head does for the float32 tower: d_h1[n][height * width] = relu(dot(relu(bn(conv) + shortcut)[pixel][:],
// w1x1) * bn_scale + bn_shift); the layer's own output never goes to HBM (in float32 it would be twice the bytes of every other
// activation of these towers).  snk_head_dense_f32 finishes AlphaNNet.v from d_h1.
extern "C" int snk_conv3x3_bn_f16_act16_head(const void *d_x16, const void *d_wS, const float *d_scale, const float *d_shift,
                                             const void *d_residual16, const float *d_w1x1, float bn_scale, float bn_shift,
                                             float *d_h1, int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x16 && d_wS && d_scale && d_shift && d_residual16 && d_w1x1 && d_h1, "snk_conv3x3_bn_f16_act16_head: NULL argument");
    ConvForm f = conv_bn_form("snk_conv3x3_bn_f16_act16_head", HS_MODE_HEAD, d_x16, d_wS, d_scale, d_shift, d_residual16, nullptr, 1,
                              n_images, height, width, stream);
    conv_form_head(f, d_w1x1, bn_scale, bn_shift, d_h1);
    conv_form_a16(f, false, false, false);
    return conv_f16s_launch(f);
}

extern "C" int snk_conv3x3_bn_bf16_act16_head(const void *d_x16, const void *d_wS, const float *d_scale, const float *d_shift,
                                              const void *d_residual16, const float *d_w1x1, float bn_scale, float bn_shift,
                                              float *d_h1, int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x16 && d_wS && d_scale && d_shift && d_residual16 && d_w1x1 && d_h1, "snk_conv3x3_bn_bf16_act16_head: NULL argument");
    ConvForm f = conv_bn_form("snk_conv3x3_bn_bf16_act16_head", HS_MODE_HEAD, d_x16, d_wS, d_scale, d_shift, d_residual16, nullptr, 1,
                              n_images, height, width, stream);
    conv_form_head(f, d_w1x1, bn_scale, bn_shift, d_h1);
    conv_form_a16(f, false, true, false);
    return conv_f16s_launch(f);
}

// The mxfp8 tower (SNK_CONV_ALGO=mxfp8): the bf16 tower's arguments, activations and epilogue; the MFMA operands are MX-FP8 (the
// rule above mx_scale_byte): every 32-channel block of a staged pixel is quantized on its way into LDS, the weights once by
// snk_conv3x3_prepare_weights_mxfp8, and each tap's 128 input channels go through two v_mfma_scale_f32_32x32x64_f8f6f4.
extern "C" int snk_conv3x3_bn_mxfp8_act16(const void *d_x16, const void *d_wS, const float *d_scale, const float *d_shift,
                                          const void *d_residual16, void *d_out, int out_bf16, int n_images, int height, int width,
                                          int relu, void *stream)
{
    SNK_REQUIRE(d_x16 && d_wS && d_scale && d_shift && d_out, "snk_conv3x3_bn_mxfp8_act16: NULL argument");
    SNK_REQUIRE(n_images > 0, "snk_conv3x3_bn_mxfp8_act16: %d images", n_images);
    ConvForm f = conv_bn_form("snk_conv3x3_bn_mxfp8_act16", hs_tower_mode(relu, d_residual16), d_x16, d_wS, d_scale, d_shift, d_residual16,
                              d_out, relu, n_images, height, width, stream);
    conv_form_a16(f, out_bf16 != 0, true, true);
    return conv_f16s_launch(f);
}

extern "C" int snk_conv3x3_bn_mxfp8_act16_rect(const void *d_x16, const void *d_wS, const float *d_scale, const float *d_shift,
                                               const void *d_residual16, void *d_out16, const void *d_desc, const int *d_count,
                                               const void *d_bg_in16, int grow_in, const void *d_bg_res16, int grow_res,
                                               const void *d_bg_out16, int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(n_images > 0, "snk_conv3x3_bn_mxfp8_act16_rect: %d images", n_images);
    return conv_f16s_rect_launch(conv_rect_form16(conv_rect_form("snk_conv3x3_bn_mxfp8_act16_rect", d_x16, d_wS, d_scale, d_shift, d_residual16,
                                                                 d_out16, d_desc, d_count, d_bg_in16, grow_in, d_bg_res16, grow_res, d_bg_out16,
                                                                 n_images, height, width, stream), true, true));
}

extern "C" int snk_conv3x3_bn_mxfp8_act16_head(const void *d_x16, const void *d_wS, const float *d_scale, const float *d_shift,
                                               const void *d_residual16, const float *d_w1x1, float bn_scale, float bn_shift,
                                               float *d_h1, int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x16 && d_wS && d_scale && d_shift && d_residual16 && d_w1x1 && d_h1, "snk_conv3x3_bn_mxfp8_act16_head: NULL argument");
    SNK_REQUIRE(n_images > 0, "snk_conv3x3_bn_mxfp8_act16_head: %d images", n_images);
    ConvForm f = conv_bn_form("snk_conv3x3_bn_mxfp8_act16_head", HS_MODE_HEAD, d_x16, d_wS, d_scale, d_shift, d_residual16, nullptr, 1,
                              n_images, height, width, stream);
    conv_form_head(f, d_w1x1, bn_scale, bn_shift, d_h1);
    conv_form_a16(f, false, true, true);
    return conv_f16s_launch(f);
}

// The training step's INPUT-GRADIENT convolution with the next batch-norm backward's sums in its epilogue: d_out = conv3x3_same(d_x,
// mirrored kernel) (+ d_residual, the shortcut's gradient) is the gradient at the output of the layer below; from the same values
// on their way out d_sums[0..127] = sum(g), d_sums[128..255] = sum(g * (y - mean) * inv) with g = d_out where that layer's ReLU bit
// is set (d_mask: one byte per quad of channels, as snk_bn_train_apply writes them; d_y: its pre-batch-norm output) -- what
// snk_bn_train_grad_sums_f64 computes from d_out in a pass of its own.  d_partials: snk_conv3x3_stats_partials floats.
extern "C" int snk_conv3x3_f16s_igrad_stats(const float *d_x, const void *d_wS, const float *d_residual, float *d_out,
                                            const float *d_y, const uint8_t *d_mask, const float *d_mean, const float *d_inv, float *d_partials,
                                            double *d_sums, int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_out && d_y && d_mask && d_mean && d_inv && d_partials && d_sums && n_images > 0,
                "snk_conv3x3_f16s_igrad_stats: bad argument");
    ConvForm f = conv_train_form("snk_conv3x3_f16s_igrad_stats", HS_MODE_IGRAD, true, d_x, d_wS, d_residual, d_out, d_mean, n_images, height,
                                 width, stream);
    f.a.g_y = d_y; f.a.g_mask = d_mask; f.a.g_inv = d_inv;
    return conv_train(f, d_partials, d_sums);
}

extern "C" int snk_conv3x3_f16_igrad_stats(const float *d_x, const void *d_wS, const float *d_residual, float *d_out,
                                           const float *d_y, const uint8_t *d_mask, const float *d_mean, const float *d_inv, float *d_partials,
                                           double *d_sums, int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_out && d_y && d_mask && d_mean && d_inv && d_partials && d_sums && n_images > 0,
                "snk_conv3x3_f16_igrad_stats: bad argument");
    ConvForm f = conv_train_form("snk_conv3x3_f16_igrad_stats", HS_MODE_IGRAD, false, d_x, d_wS, d_residual, d_out, d_mean, n_images, height,
                                 width, stream);
    f.a.g_y = d_y; f.a.g_mask = d_mask; f.a.g_inv = d_inv;
    return conv_train(f, d_partials, d_sums);
}

// The same for a layer below whose batch norm + ReLU output was never written (deferred): its ReLU decision is
// d_y * d_scale[c] + d_shift[c] > 0 -- the sign of what snk_bn_train_apply would have written -- instead of mask bytes.
extern "C" int snk_conv3x3_f16s_igrad_stats_deferred(const float *d_x, const void *d_wS, const float *d_residual, float *d_out,
                                                     const float *d_y, const float *d_scale, const float *d_shift,
                                                     const float *d_mean, const float *d_inv, float *d_partials, double *d_sums, int n_images,
                                                     int height, int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_out && d_y && d_scale && d_shift && d_mean && d_inv && d_partials && d_sums && n_images > 0,
                "snk_conv3x3_f16s_igrad_stats_deferred: bad argument");
    ConvForm f = conv_train_form("snk_conv3x3_f16s_igrad_stats_deferred", HS_MODE_IGRAD_AFF, true, d_x, d_wS, d_residual, d_out, d_mean,
                                 n_images, height, width, stream);
    f.a.g_y = d_y; f.a.g_inv = d_inv; f.a.aff_scale = d_scale; f.a.aff_shift = d_shift;
    return conv_train(f, d_partials, d_sums);
}

extern "C" int snk_conv3x3_f16_igrad_stats_deferred(const float *d_x, const void *d_wS, const float *d_residual, float *d_out,
                                                    const float *d_y, const float *d_scale, const float *d_shift, const float *d_mean,
                                                    const float *d_inv, float *d_partials, double *d_sums, int n_images, int height,
                                                    int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_out && d_y && d_scale && d_shift && d_mean && d_inv && d_partials && d_sums && n_images > 0,
                "snk_conv3x3_f16_igrad_stats_deferred: bad argument");
    ConvForm f = conv_train_form("snk_conv3x3_f16_igrad_stats_deferred", HS_MODE_IGRAD_AFF, false, d_x, d_wS, d_residual, d_out, d_mean,
                                 n_images, height, width, stream);
    f.a.g_y = d_y; f.a.g_inv = d_inv; f.a.aff_scale = d_scale; f.a.aff_shift = d_shift;
    return conv_train(f, d_partials, d_sums);
}

// snk_conv3x3_f16s_igrad_stats whose shortcut gradient is d_residual WHERE d_residual_mask's bit is set: d_residual = the gradient
// at the residual block's output (before that output's ReLU), d_residual_mask = that output's ReLU bits (snk_bn_train_apply's
// bytes) -- the masked copy snk_bn_train_grad_apply(d_g) writes is not needed.  d_out may be d_residual (in place).
extern "C" int snk_conv3x3_f16s_igrad_stats_masked_res(const float *d_x, const void *d_wS, const float *d_residual,
                                                       const uint8_t *d_residual_mask, float *d_out, const float *d_y, const uint8_t *d_mask,
                                                       const float *d_mean, const float *d_inv, float *d_partials, double *d_sums,
                                                       int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_residual && d_residual_mask && d_out && d_y && d_mask && d_mean && d_inv && d_partials && d_sums &&
                n_images > 0, "snk_conv3x3_f16s_igrad_stats_masked_res: bad argument");
    ConvForm f = conv_train_form("snk_conv3x3_f16s_igrad_stats_masked_res", HS_MODE_IGRAD_MRES, true, d_x, d_wS, d_residual, d_out, d_mean,
                                 n_images, height, width, stream);
    f.a.g_y = d_y; f.a.g_mask = d_mask; f.a.g_inv = d_inv; f.a.res_mask = d_residual_mask;
    return conv_train(f, d_partials, d_sums);
}

extern "C" int snk_conv3x3_f16_igrad_stats_masked_res(const float *d_x, const void *d_wS, const float *d_residual,
                                                      const uint8_t *d_residual_mask, float *d_out, const float *d_y, const uint8_t *d_mask,
                                                      const float *d_mean, const float *d_inv, float *d_partials, double *d_sums,
                                                      int n_images, int height, int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_residual && d_residual_mask && d_out && d_y && d_mask && d_mean && d_inv && d_partials && d_sums &&
                n_images > 0, "snk_conv3x3_f16_igrad_stats_masked_res: bad argument");
    ConvForm f = conv_train_form("snk_conv3x3_f16_igrad_stats_masked_res", HS_MODE_IGRAD_MRES, false, d_x, d_wS, d_residual, d_out, d_mean,
                                 n_images, height, width, stream);
    f.a.g_y = d_y; f.a.g_mask = d_mask; f.a.g_inv = d_inv; f.a.res_mask = d_residual_mask;
    return conv_train(f, d_partials, d_sums);
}

// snk_conv3x3_f16s_igrad_stats_masked_res for a layer below whose batch norm + ReLU output was never written (the deferred stem):
// the ReLU decision of the SUMS is d_y * d_scale[c] + d_shift[c] > 0 instead of mask bytes
extern "C" int snk_conv3x3_f16s_igrad_stats_masked_res_deferred(const float *d_x, const void *d_wS, const float *d_residual,
                                                                const uint8_t *d_residual_mask, float *d_out, const float *d_y,
                                                                const float *d_scale, const float *d_shift, const float *d_mean,
                                                                const float *d_inv, float *d_partials, double *d_sums, int n_images,
                                                                int height, int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_residual && d_residual_mask && d_out && d_y && d_scale && d_shift && d_mean && d_inv && d_partials &&
                d_sums && n_images > 0, "snk_conv3x3_f16s_igrad_stats_masked_res_deferred: bad argument");
    ConvForm f = conv_train_form("snk_conv3x3_f16s_igrad_stats_masked_res_deferred", HS_MODE_IGRAD_MRES_AFF, true, d_x, d_wS, d_residual,
                                 d_out, d_mean, n_images, height, width, stream);
    f.a.g_y = d_y; f.a.g_inv = d_inv; f.a.aff_scale = d_scale; f.a.aff_shift = d_shift; f.a.res_mask = d_residual_mask;
    return conv_train(f, d_partials, d_sums);
}

extern "C" int snk_conv3x3_f16_igrad_stats_masked_res_deferred(const float *d_x, const void *d_wS, const float *d_residual,
                                                               const uint8_t *d_residual_mask, float *d_out, const float *d_y,
                                                               const float *d_scale, const float *d_shift, const float *d_mean,
                                                               const float *d_inv, float *d_partials, double *d_sums, int n_images, int height,
                                                               int width, void *stream)
{
    SNK_REQUIRE(d_x && d_wS && d_residual && d_residual_mask && d_out && d_y && d_scale && d_shift && d_mean && d_inv && d_partials &&
                d_sums && n_images > 0, "snk_conv3x3_f16_igrad_stats_masked_res_deferred: bad argument");
    ConvForm f = conv_train_form("snk_conv3x3_f16_igrad_stats_masked_res_deferred", HS_MODE_IGRAD_MRES_AFF, false, d_x, d_wS, d_residual,
                                 d_out, d_mean, n_images, height, width, stream);
    f.a.g_y = d_y; f.a.g_inv = d_inv; f.a.aff_scale = d_scale; f.a.aff_shift = d_shift; f.a.res_mask = d_residual_mask;
    return conv_train(f, d_partials, d_sums);
}
