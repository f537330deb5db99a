/* sjpeg_hip.h -- C-ABI of the MI355X (gfx950) scan engine.
 *
 * This is the one device boundary of the library: the host encoder (include/sjpeg.h,
 * sjpeg_amd/csrc/host_*.cc) prepares quantizers, Huffman codes and JFIF headers exactly
 * as the reference does, then hands whole frames (or a batch of frames) to
 * sjpeg_hip_encode_scan(), which replaces the reference's per-MCU hot loop
 *
 *     Encoder::SinglePassScan()            /root/reference/src/enc.cc:276-307
 *       -> GetSamples()                    src/encoders.cc:170-182,206-215,239-248
 *       -> fDCT_()                         src/fdct.cc:596-609
 *       -> quantize_block_()               src/quantize.cc:288-320
 *       -> GenerateDCDiffCode()/CodeBlock  src/entropy.cc:133-198
 *       -> BitWriter::PutBits/FlushBits    src/bit_writer.h:172-209, bit_writer.cc:107-116
 *
 * with hand-written HIP kernels.  Plain pointers and sizes only: no C++ types, no torch
 * types.  A binding for any host language (cgo, JNI, ctypes, N-API) binds exactly these
 * symbols; see INTEGRATION.md.
 *
 * All functions return 0 on success or a negative SJPEG_HIP_E* code; the message of the
 * last failure on the calling thread is available from sjpeg_hip_last_error().
 * Nothing here ever falls back to a CPU implementation: without a usable gfx950 device
 * the calls fail.
 */
#ifndef SJPEG_HIP_H_
#define SJPEG_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SJPEG_HIP_ABI_VERSION 18

enum {
  SJPEG_HIP_OK = 0,
  SJPEG_HIP_EINVAL = -1,      /* bad argument (null pointer, size, mode, ...)        */
  SJPEG_HIP_ENODEV = -2,      /* no usable HIP device / runtime                      */
  SJPEG_HIP_ENOMEM = -3,      /* device or host allocation failed                    */
  SJPEG_HIP_ERUNTIME = -4,    /* a HIP call or kernel failed                         */
  SJPEG_HIP_ECAPACITY = -5    /* caller's output slots are smaller than required     */
};

/* Values of SjpegYUVMode (include/sjpeg.h) that the scan engine codes directly. */
enum { SJPEG_HIP_YUV420 = 1, SJPEG_HIP_YUV444 = 3, SJPEG_HIP_YUV400 = 4 };

/* Everything the scan needs besides pixels, in the reference's own units.
 * Index 0 = luma tables, 1 = chroma tables (reference quant_idx_, src/encoders.cc:37-39).
 * iquant/bias are the reference Quantizer fields (src/sjpegi.h:228-235) in NATURAL order
 * as produced by Encoder::FinalizeQuantMatrix (src/quantize.cc:123-148); qthresh is not
 * needed: by construction (src/quantize.cc:144-145) a >= qthresh <=> QUANTIZE(a) > 0.
 * dc_codes/ac_codes are the packed (code << 16) | length words of
 * BuildHuffmanTable (src/entropy.cc:98-112). */
typedef struct sjpeg_hip_scan_tables {
  uint16_t iquant[2][64];
  uint16_t bias[2][64];
  uint32_t dc_codes[2][12];
  uint32_t ac_codes[2][256];
  uint8_t quant[2][64];        /* the (final, clamped) quantizer steps; read by the quantization-
                                  error pass (src/quantize.cc:553-565) and the trellis */
  uint8_t trellis_len[2][256]; /* SJPEG_HIP_QUANT_TRELLIS: AC code LENGTHS the rate term is priced
                                  with (what Quantizer::codes_ points at, src/quantize.cc:151,396):
                                  the standard tables in the reference's single-pass flow */
  uint32_t flags;              /* SJPEG_HIP_QUANT_* */
} sjpeg_hip_scan_tables;

/* flags: quantize with the trellis search of the reference's methods 7 / 8
 * (Encoder::TrellisQuantizeBlock, src/quantize.cc:325-457) instead of plain rounding.  Applies to
 * the encode and symbol-statistics passes. */
#define SJPEG_HIP_QUANT_TRELLIS 1u
/* Two-pass flows quantize every block twice (statistics pass, then encode pass with the tables
 * compiled from it).  KEEP: the statistics pass leaves its quantized blocks in the engine (144 B per
 * block); REPLAY: the encode pass entropy-codes those instead of converting, transforming and
 * quantizing the pixels again -- what the reference's stored run/levels do (reuse_run_levels_,
 * src/enc.cc:121-129).  REPLAY needs a KEEP statistics pass of the same geometry right before it on
 * the same engine, and ignores iquant / bias / quant / trellis_len / the pixel source.  Worth it
 * where quantization is expensive: the host API uses it for the trellis methods. */
#define SJPEG_HIP_QUANT_KEEP 2u
#define SJPEG_HIP_QUANT_REPLAY 4u
/* OPTIONAL restart-marker mode (encode calls).  NOT the reference's bytes -- it never writes DRI / RSTn
 * (src/sjpegi.h:68-74) -- but the same picture: same tables, same coefficients, identical pixels
 * after decoding.  Every segment of the engine (sjpeg_hip_restart_interval() MCUs) becomes a restart
 * interval: its bits padded to a byte with 1-bits, RSTn (FF D0+(n & 7)) behind it, DC predictors
 * reset (ITU-T T.81 B.2.4.4 / F.1.2.3).  The header passed to the call must carry the DRI segment:
 * sjpeg_hip_header_add_restart().  What it is for: intervals are independently decodable and byte
 * aligned, so a frame's intervals can be produced on different devices and concatenated by the host
 * with no bit-level stitch. */
#define SJPEG_HIP_RESTART_MARKERS 8u

/* Pixel sources.  Packed colour and gray use plane[0]; planar YUV uses Y, U, V; NV12/NV21 use
 * Y and the interleaved chroma plane in plane[1].  Chroma planes of the 4:2:0 layouts are
 * (width+1)/2 x (height+1)/2 samples.  These replace the reference's input adapters
 * Encoder420/444/400 (src/encoders.cc:157-253, packed RGB/BGRA/RGBA), Encoder400G (:256-276),
 * EncoderNV12 (:281-344), EncoderYUV444 (:384-419) and EncoderYUV420 (:442-490). */
enum {
  SJPEG_HIP_SRC_RGB = 0,       /* 3 bytes/pixel R,G,B     -> any of 420 / 444 / 400 */
  SJPEG_HIP_SRC_BGRA = 1,      /* 4 bytes/pixel B,G,R,A   -> any of 420 / 444 / 400 */
  SJPEG_HIP_SRC_RGBA = 2,      /* 4 bytes/pixel R,G,B,A   -> any of 420 / 444 / 400 */
  SJPEG_HIP_SRC_GRAY = 3,      /* 1 plane                 -> 400 */
  SJPEG_HIP_SRC_YUV444 = 4,    /* 3 full-size planes      -> 444 */
  SJPEG_HIP_SRC_YUV420 = 5,    /* Y + subsampled U, V     -> 420 */
  SJPEG_HIP_SRC_NV12 = 6,      /* Y + interleaved U,V     -> 420 */
  SJPEG_HIP_SRC_NV21 = 7,      /* Y + interleaved V,U     -> 420 */
  SJPEG_HIP_SRC_RGB_PLANAR = 8, /* 3 full-size planes R,G,B -> any of 420 / 444 / 400 */
  SJPEG_HIP_SRC_RGB_PLANAR_F32 = 9,   /* the same planes of float elements (below): fp32 ... */
  SJPEG_HIP_SRC_RGB_PLANAR_F16 = 10,  /* ... IEEE half ... */
  SJPEG_HIP_SRC_RGB_PLANAR_BF16 = 11, /* ... bfloat16 */
  /* one plane of interleaved float pixels (below): 3 elements a pixel, R, G, B -> any of 420 / 444 / 400 */
  SJPEG_HIP_SRC_RGB_F32 = 12, SJPEG_HIP_SRC_RGB_F16 = 13, SJPEG_HIP_SRC_RGB_BF16 = 14,
  /* ... 4 elements a pixel, R, G, B and a fourth that is never read */
  SJPEG_HIP_SRC_RGBA_F32 = 15, SJPEG_HIP_SRC_RGBA_F16 = 16, SJPEG_HIP_SRC_RGBA_BF16 = 17,
  /* one plane, 1 float element a pixel -> 400 */
  SJPEG_HIP_SRC_GRAY_F32 = 18, SJPEG_HIP_SRC_GRAY_F16 = 19, SJPEG_HIP_SRC_GRAY_BF16 = 20
};
/* SJPEG_HIP_SRC_RGB_PLANAR (channel-first pictures: a [3, H, W] or [N, 3, H, W] array, or any crop of one):
 * plane[0..2] are R, G, B, each width x height bytes; the bytes produced are those of the same pixels handed over
 * as SJPEG_HIP_SRC_RGB.  ONE PITCH, THREE BASES: row_stride[1] and row_stride[2] must equal row_stride[0] (and, in a
 * sjpeg_hip_source, frame_stride[1] and frame_stride[2] must equal frame_stride[0]); |row_stride| >= width; negative
 * strides work as for every other layout.  A mismatch is SJPEG_HIP_EINVAL -- the message names the stride and, in
 * ragged calls, the frame.  The rule lets the three planes share one per-thread offset: the kernels address
 * G and B as R's address plus a uniform 64-bit distance, plane[1] - plane[0] and plane[2] - plane[0].
 * Taken by every entry point that takes a `format` or a sjpeg_hip_source, SJPEG_YUV_AUTO / SJPEG_YUV_SHARP, the
 * riskiness and the sharp conversion included (there it counts as an RGB source beside RGB, BGRA and RGBA).
 *
 * SJPEG_HIP_SRC_RGB_PLANAR_F32 / _F16 / _BF16 (what a network puts out: channel-first float tensors, values in 0..1
 * or -1..1): the layout and the one-pitch rule of SJPEG_HIP_SRC_RGB_PLANAR with elements of 4 or 2 bytes.  Strides
 * stay in BYTES and may be negative; |row_stride| >= width * element size; plane pointers, row strides and frame
 * strides must be multiples of the element size -- the only alignment the kernels assume, so a crop of a wider
 * tensor at an odd column works.  A violation is SJPEG_HIP_EINVAL before any device work; the message names the
 * stride or plane and, in ragged calls, the frame.  A sample x becomes the byte the encoder sees by
 *     t  = fmaf((float)x, scale, bias)           ONE fp32 rounding; (float)x is exact for half and bfloat16
 *     u8 = isnan(t) ? 0 : (uint8) rint(min(max(t, 0), 255))       round half to even; +-inf saturate
 * with the engine's pixel transform (scale, bias) of the sample's channel -- sjpeg_hip_engine_set_pixel_transform() /
 * _transform3(), 255 and 0 by default --
 * and the JPEG bytes are exactly those of the uint8 picture so defined handed over as SJPEG_HIP_SRC_RGB_PLANAR.
 * (It is the fused multiply-add: a host-side restatement must use fmaf, not a product rounded before the sum.)  The
 * conversion happens in the kernels' loader: no uint8 copy of the batch is made.
 * Taken by every entry point that has an engine and takes a `format` or a sjpeg_hip_source, in all three samplings,
 * SJPEG_YUV_AUTO / SJPEG_YUV_SHARP, sjpeg_hip_riskiness_ragged_src and sjpeg_hip_sharp_yuv_ragged included.  The two
 * calls without an engine, sjpeg_hip_riskiness_sums and sjpeg_hip_sharp_yuv, have no transform to read and refuse the
 * three formats (SJPEG_HIP_EINVAL; the message names the ragged call to use).
 *
 * SJPEG_HIP_SRC_RGB_F32 / _F16 / _BF16, SJPEG_HIP_SRC_RGBA_F32 / _F16 / _BF16 (channels-last tensors, a renderer's
 * RGBA16F, any [H, W, 3] or [H, W, 4] float array) and SJPEG_HIP_SRC_GRAY_F32 / _F16 / _BF16 (depth maps, masks,
 * [H, W] floats): ONE plane, plane[0], of float elements; a pixel is `step` = 3, 4 or 1 elements from the next and its
 * first `channels` = 3, 3 or 1 elements are read -- R, G, B, or the gray value.  plane[1] and plane[2] are ignored, as
 * for SJPEG_HIP_SRC_RGB.  Strides are in BYTES and may be negative; plane[0], row strides and frame strides are
 * multiples of the element size, the only alignment assumed; |row_stride| >= ((width - 1) * step + channels) * element
 * size.  The kernels never read an element that is not a used sample of a pixel of the picture: in particular not the
 * fourth element of a row's last pixel, so x[..., 1:4] of an ARGB tensor is a legal RGBA source although its last
 * "alpha" lies outside the allocation.  A violation is SJPEG_HIP_EINVAL before any device work; the message names the
 * stride or plane and, in ragged calls, the frame.  Samples become bytes as above, channel c = 0, 1, 2 for R, G, B
 * through scale[c] and bias[c], gray through channel 0; the JPEG bytes are exactly those of the uint8 picture so
 * defined handed over as SJPEG_HIP_SRC_RGB (the gray formats: as SJPEG_HIP_SRC_GRAY, yuv_mode 4:0:0 only).
 * Taken where the planar float formats are; the gray ones are refused where SJPEG_HIP_SRC_GRAY is (SJPEG_YUV_AUTO /
 * SJPEG_YUV_SHARP, the riskiness, the sharp conversion), and the two calls without an engine refuse all nine. */
typedef struct sjpeg_hip_source {
  int32_t format;              /* SJPEG_HIP_SRC_* */
  int32_t reserved;            /* 0 */
  const void* plane[3];        /* DEVICE pointers */
  int64_t row_stride[3];       /* bytes between rows of each plane; may be negative */
  int64_t frame_stride[3];     /* bytes between consecutive frames of a batch, per plane */
} sjpeg_hip_source;

/* A Huffman table in DHT form: BITS (number of codes of each length 1..16) and HUFFVAL
 * (symbols by increasing code length), reference struct HuffmanTable (src/sjpegi.h:221-225). */
typedef struct sjpeg_hip_huffman_spec {
  uint8_t bits[16];
  uint8_t syms[256];
  int32_t nsyms;
} sjpeg_hip_huffman_spec;

/* Opaque engine: one HIP device, cached device scratch.  Not thread-safe; use one engine
 * per host thread (they may share a device).  Every call is asynchronous on the stream it is
 * given; the scratch is shared by all calls, so a call on another stream than the previous one
 * first waits (on the device) for that one's work -- use one engine per stream to overlap.
 * A stream handed to a call must stay alive until the engine's NEXT call has been issued (that call
 * orders itself behind it with an event); if it was destroyed earlier the engine falls back to a
 * device-wide synchronisation instead of failing.
 * The scratch of an encode is sized from the bytes the caller gives every frame (out_stride), per frame of the
 * batch; a batch that would take more than SJPEG_HIP_SCRATCH_LIMIT_BYTES of it (environment, read when the engine
 * is created; default 16 GiB) is coded as several launches of as many frames as fit, in order, on the same
 * stream -- the caller sees one call. */
typedef struct sjpeg_hip_engine sjpeg_hip_engine;

int sjpeg_hip_abi_version(void);
int sjpeg_hip_device_count(void);                 /* 0 when no device/runtime */
const char* sjpeg_hip_last_error(void);

int sjpeg_hip_engine_create(int device, sjpeg_hip_engine** engine);
void sjpeg_hip_engine_destroy(sjpeg_hip_engine* engine);

/* Worst-case size in bytes of ONE coded frame (header + stuffed entropy data + EOI):
 * the minimum legal out_stride for sjpeg_hip_encode_scan().  Follows the reference's
 * own bound of 2560 bytes per MCU (src/enc.cc:206-209).  0 on invalid arguments. */
size_t sjpeg_hip_frame_bound(int width, int height, int yuv_mode, size_t header_size);

/* Codes `nframes` frames that are RESIDENT IN DEVICE MEMORY, all with the same geometry
 * and tables, each into its own complete JPEG byte stream:
 *
 *   d_out + f*out_stride : [ header bytes | entropy-coded segment | FF D9 ]
 *   d_sizes[f]           : number of bytes written for frame f
 *
 *   d_rgb         packed 8-bit R,G,B; pixel (x,y) of frame f at
 *                 d_rgb + f*frame_stride + y*row_stride + 3*x.  row_stride may be negative
 *                 (bottom-up images, as the reference allows: src/api.cc:35-36).
 *   header        HOST pointer to the bytes that precede the entropy segment (SOI..SOS,
 *                 written by the host exactly like src/headers.cc); may be NULL/0, in which
 *                 case each stream starts directly with entropy data.
 *   append_eoi    non-zero: terminate each stream with FF D9 (src/headers.cc:262-268).
 *   d_out         device buffer, nframes*out_stride bytes.  out_stride >= frame_bound always
 *                 suffices; a smaller slot is legal (the engine's scratch is sized from it, about
 *                 3.5 x out_stride per frame instead of the worst case of the geometry): a frame
 *                 whose stream does not fit its slot reports d_sizes[f] = 0 and is not written,
 *                 the other frames of the batch are unaffected.
 *   d_sizes       device array of nframes uint64.
 *   stream        hipStream_t (as void*) on which everything is enqueued; NULL = default
 *                 stream.  The call is asynchronous: results are valid once the stream
 *                 has drained.
 *
 * The output is bit-identical to what the reference writes between (and including) the
 * same header and EOI for the same pixels and tables. */
int sjpeg_hip_encode_scan(sjpeg_hip_engine* engine,
                          const void* d_rgb, int64_t row_stride, int64_t frame_stride,
                          int width, int height, int yuv_mode, int nframes,
                          const sjpeg_hip_scan_tables* tables,
                          const void* header, size_t header_size, int append_eoi,
                          void* d_out, size_t out_stride, uint64_t* d_sizes,
                          void* stream);

/* Stage taps for tests and profiling (same arguments as above where named alike).
 * d_coeffs receives the quantized coefficients of every block in stream order,
 * 64 int16 per block in zig-zag order, element 0 = quantized DC *value*
 * (blocks per frame = mcu count * {6,3,1}).  Pure function of pixels + tables. */
int sjpeg_hip_scan_coeffs(sjpeg_hip_engine* engine,
                          const void* d_rgb, int64_t row_stride, int64_t frame_stride,
                          int width, int height, int yuv_mode, int nframes,
                          const sjpeg_hip_scan_tables* tables,
                          int16_t* d_coeffs, void* stream);

/* Statistics passes for the reference's methods 1..6 (same pixel arguments as above).
 *
 * sjpeg_hip_scan_histogram: replaces Encoder::CollectHistograms (src/histogram.cc:317-339 with
 * StoreHisto :56-108).  d_hist receives, per frame, uint32 [2][64][128]: for quantizer table
 * t (0 luma, 1 chroma) and NATURAL coefficient position p, the number of blocks whose
 * un-quantized coefficient c has |c| >> 2 == bin (bin < 128).
 *
 * sjpeg_hip_scan_symbol_stats: replaces the statistics half of SinglePassScanOptimized
 * (src/enc.cc:323-372, AddEntropyStats src/entropy.cc:208-227).  Needs tables->iquant/bias.
 * d_freq receives, per frame, uint32 [2][272]: [t][0..255] AC symbol counts (run << 4 | size,
 * 0xF0 = ZRL, 0x00 = EOB), [t][256 + n] DC size-category counts. */
int sjpeg_hip_scan_histogram(sjpeg_hip_engine* engine,
                             const void* d_rgb, int64_t row_stride, int64_t frame_stride,
                             int width, int height, int yuv_mode, int nframes,
                             uint32_t* d_hist, void* stream);
int sjpeg_hip_scan_symbol_stats(sjpeg_hip_engine* engine,
                                const void* d_rgb, int64_t row_stride, int64_t frame_stride,
                                int width, int height, int yuv_mode, int nframes,
                                const sjpeg_hip_scan_tables* tables,
                                uint32_t* d_freq, void* stream);

/* Replaces Encoder::ComputePSNR's inner sum (src/dichotomy.cc:302-323 with QuantizeError,
 * src/quantize.cc:553-565): d_err receives, per frame, the uint64 sum over all blocks and
 * coefficients of ((|c| >> 4) - quant * level)^2 (each block's sum wrapped to 32 bits like the
 * reference).  Needs tables->iquant / bias / quant. */
int sjpeg_hip_scan_quant_error_src(sjpeg_hip_engine* engine, const struct sjpeg_hip_source* src,
                                   int width, int height, int yuv_mode, int nframes,
                                   const sjpeg_hip_scan_tables* tables, uint64_t* d_err,
                                   void* stream);

/* Number of entropy-coded bits (before byte stuffing and padding) of each frame of the most
 * recent sjpeg_hip_encode_scan*() call on this engine, copied to HOST memory `bits[nframes]`.
 * Synchronises the device.  With the coded size this gives what the reference's BitCounter
 * reports (src/bit_writer.h:292-365).  (Not defined behind sjpeg_hip_encode_batch_src, whose
 * jobs may run on the engine's child engines.) */
int sjpeg_hip_engine_entropy_bits(sjpeg_hip_engine* engine, uint64_t* bits, int nframes);

/* ---- SJPEG_YUV_SHARP: the iterative sharp RGB -> YUV 4:2:0 conversion -----------------------------
 * Replaces sjpeg::ApplySharpYUVConversion (src/yuv_convert.cc:674-697; the pre-pass of
 * EncoderSharp420, src/encoders.cc:512-541).  `src` is packed RGB / BGRA / RGBA or planar RGB in device memory;
 * the result is three tightly packed 8-bit planes per frame: Y width x height, U and V
 * ((width+1)/2) x ((height+1)/2), frames y_frame_stride / uv_frame_stride bytes apart -- exactly
 * what a SJPEG_HIP_SRC_YUV420 source of sjpeg_hip_encode_scan_src() then takes.  The row pairs of
 * a sweep are sequential by construction (a row pair reads the row above as this sweep left it); the
 * columns of a row pair, the up to four sweeps of a picture (a pipeline a few row pairs apart) and
 * the pictures of a batch run in parallel.  Any width.  d_workspace: sjpeg_hip_sharp_workspace()
 * bytes of device memory.  (Environment, read once, for A/B runs only: SJPEG_HIP_SHARP_STRIPS=0 takes
 * the kernel with one workgroup per picture and sweep, SJPEG_HIP_SHARP_INPLACE=1 the in-place sweeps;
 * same planes.) */
size_t sjpeg_hip_sharp_workspace(int width, int height, int nframes);
int sjpeg_hip_sharp_yuv(const sjpeg_hip_source* src, int width, int height, int nframes,
                        uint8_t* d_y, uint8_t* d_u, uint8_t* d_v, int64_t y_frame_stride,
                        int64_t uv_frame_stride, void* d_workspace, size_t workspace_size,
                        void* stream);

/* ---- SJPEG_YUV_AUTO / SjpegRiskiness (src/jpeg_tools.cc:170-236) -------------------------------
 * The decision between 4:2:0 / sharp / 4:4:4 / 4:0:0 is made of three sums of a stencil over the
 * picture; the stencil looks pairs of 7x7x7 YUV cells up in a 343 x 343 byte table.  That table
 * is trained data of the reference (src/score_7.cc, `sjpeg::kSharpnessScore`): it ships beside the
 * library as riskiness.bin (the reference's bytes, Apache-2.0: riskiness.NOTICE) and is found there;
 * another copy goes in with sjpeg_hip_set_riskiness_table() (117649 bytes, host memory; copied) or
 * through the environment variable SJPEG_HIP_RISKINESS_TABLE (a file holding those bytes).  A
 * library installed without any: SJPEG_YUV_AUTO, SjpegCompress() and SjpegRiskiness() fail.
 * sjpeg_hip_riskiness_sums: device part; d_sums[nframes][3] = sum of the scores above the noise
 * level, their count, the count of neutral-chroma samples. */
#define SJPEG_HIP_RISKINESS_TABLE_SIZE 117649
int sjpeg_hip_set_riskiness_table(const uint8_t* table, size_t size);
int sjpeg_hip_has_riskiness_table(void);
int sjpeg_hip_riskiness_sums(const sjpeg_hip_source* src, int width, int height, int nframes,
                             const uint8_t* d_table, uint64_t* d_sums, void* stream);

/* ---- one frame over several GPUs ------------------------------------------
 * The reference codes a frame as ONE entropy segment (src/enc.cc:276-307; no restart markers,
 * src/sjpegi.h:68-74), so a frame can only be shared between devices at BIT granularity.  The
 * engine's unit of independent work is the segment (a fixed number of consecutive MCUs in scan
 * order); sjpeg_hip_segment_count() says how many a frame has.  Rank r of P codes the band of
 * segments [r*n/P, (r+1)*n/P): it needs the pixel rows of those MCUs plus the one MCU in front of
 * the band (DC predictors; `src` is addressed as the whole frame, rows outside are not read).
 * It gets the band's un-stuffed bit string (MSB-first 32-bit words) and its length in bits.  The
 * root gathers strings and lengths (RCCL gather / send-recv), and sjpeg_hip_stitch_bands() shifts
 * every band to its bit offset, pads with 1-bits, stuffs 0xFF bytes, adds header and EOI: the
 * bytes of sjpeg_hip_encode_scan_src() on one device, i.e. of the reference. */
int sjpeg_hip_segment_count(int width, int height, int yuv_mode);
/* capacity in 32-bit words a band buffer must have (0 on bad arguments) */
size_t sjpeg_hip_band_bound(int width, int height, int yuv_mode, int seg_begin, int seg_end);
int sjpeg_hip_encode_band_src(sjpeg_hip_engine* engine, const sjpeg_hip_source* src,
                              int width, int height, int yuv_mode,
                              const sjpeg_hip_scan_tables* tables, int seg_begin, int seg_end,
                              uint32_t* d_words, size_t cap_words, uint64_t* d_nbits, void* stream);
/* d_words: nbands buffers of band_stride_words words each, in band order (device memory of
 * `engine`'s device); d_nbits[nbands]; the rest as sjpeg_hip_encode_scan() for one frame. */
int sjpeg_hip_stitch_bands(sjpeg_hip_engine* engine, int nbands, const uint32_t* d_words,
                           size_t band_stride_words, const uint64_t* d_nbits,
                           const void* header, size_t header_size, int append_eoi,
                           void* d_out, size_t out_cap, uint64_t* d_size, void* stream);

/* The same four operations for any pixel source (the functions above are these with
 * format = SJPEG_HIP_SRC_RGB).  yuv_mode must match the source where it is implied. */
int sjpeg_hip_encode_scan_src(sjpeg_hip_engine* engine, const sjpeg_hip_source* src,
                              int width, int height, int yuv_mode, int nframes,
                              const sjpeg_hip_scan_tables* tables,
                              const void* header, size_t header_size, int append_eoi,
                              void* d_out, size_t out_stride, uint64_t* d_sizes, void* stream);
/* The same call with PACKED output: frame f is written at d_out + d_offsets[f], the frames back to back, every
 * one at a multiple of 16 with zero padding behind it; d_offsets[nframes] = the bytes the batch takes.
 * out_stride (a multiple of 16, as d_out) stays what ONE frame may take -- a frame that needs more reports
 * size 0 and takes no room --, so d_out needs nframes * out_stride bytes at most.  This is what
 * sjpeg_hip_compact_streams() makes of a strided batch, without the extra pass over the bytes: the block
 * d_out[0 .. d_offsets[nframes]) is ready for sjpeg_hip_gather_rows / _bytes (multi-device batch path).
 * Reference: none (src/enc.cc:391-448 codes one picture into one sink); config #4 of BASELINE.json. */
int sjpeg_hip_encode_scan_packed_src(sjpeg_hip_engine* engine, const sjpeg_hip_source* src,
                                     int width, int height, int yuv_mode, int nframes,
                                     const sjpeg_hip_scan_tables* tables,
                                     const void* header, size_t header_size, int append_eoi,
                                     void* d_out, size_t out_stride, uint64_t* d_sizes,
                                     uint64_t* d_offsets, void* stream);
int sjpeg_hip_scan_coeffs_src(sjpeg_hip_engine* engine, const sjpeg_hip_source* src,
                              int width, int height, int yuv_mode, int nframes,
                              const sjpeg_hip_scan_tables* tables, int16_t* d_coeffs, void* stream);
int sjpeg_hip_scan_histogram_src(sjpeg_hip_engine* engine, const sjpeg_hip_source* src,
                                 int width, int height, int yuv_mode, int nframes,
                                 uint32_t* d_hist, void* stream);
int sjpeg_hip_scan_symbol_stats_src(sjpeg_hip_engine* engine, const sjpeg_hip_source* src,
                                    int width, int height, int yuv_mode, int nframes,
                                    const sjpeg_hip_scan_tables* tables, uint32_t* d_freq,
                                    void* stream);

/* A whole batch the way the reference codes ONE picture with its default parameters
 * (Encoder::Encode, src/enc.cc:391-448): per-picture adapted quantizer (method >= 3:
 * CollectHistograms + AnalyseHisto) and per-picture optimised Huffman codes (method not 0 / 3:
 * the statistics half of SinglePassScanOptimized), then headers and the scan -- one launch per
 * device pass for all frames (histograms, analysis sums, symbol statistics, encode), the float
 * regression and BuildOptimalTable per frame on the host in between (two synchronisations of
 * `stream`).  quant = the two starting matrices (natural order, e.g. sjpeg_hip_quality_matrices),
 * min_quant NULL = ones, q_bias / qdelta_max_* as EncoderParam (0x78, 12, 1).  method 0..6 as
 * SjpegEncode (trellis methods: host API).  Output as sjpeg_hip_encode_scan_src (complete JPEGs,
 * EOI included).  A batch of 90 Mpixels or more is coded as TWO JOBS -- halves of the batch, each a complete
 * sequence of passes -- side by side: one on `stream`, one on a stream (and a child engine, with its own scratch)
 * the ENGINE owns; the call's host thread drives both, and `stream` ends behind both (the usual asynchronous
 * contract: outputs are complete when `stream` is).  The three passes have different bottlenecks, side by side they
 * fill each other's gaps: 32 4K frames 1.12 -> 1.00 ms.  Make the engine early in the life of the
 * process -- a stream made late shares a hardware queue with an older one, the caller's as a rule, and nothing overlaps. */
int sjpeg_hip_encode_batch_src(sjpeg_hip_engine* engine, const sjpeg_hip_source* src,
                               int width, int height, int yuv_mode, int nframes,
                               const uint8_t quant[2][64], const uint8_t* min_quant /*[2][64]*/, int q_bias,
                               int method, int qdelta_max_luma, int qdelta_max_chroma,
                               void* d_out, size_t out_stride, uint64_t* d_sizes, void* stream);

/* Pipelined mode, for back-to-back encode calls on one engine (a service coding batch after
 * batch): K1 of a call runs on the caller's stream, the stitch kernels K2..K5 on a stream of the
 * engine, over two sets of segment buffers, so the stitch of call i (HBM-bound) runs under the
 * K1 of call i + 1 (ALU-bound).  In this mode d_out / d_sizes of an encode call are complete
 * only after sjpeg_hip_engine_wait(engine, stream) -- which makes `stream` wait for everything
 * the engine has in flight -- or a device synchronisation; do not touch them in between.
 * Results are the same bytes.  The other entry points stay ordered on the caller's stream (they
 * wait for the engine's stream first).  Off by default; switching it off drains the engine.  (The
 * engine's stream is made by the first call that switches the mode on: do that early too.) */
int sjpeg_hip_engine_set_pipelined(sjpeg_hip_engine* engine, int on);

/* The pixel transform of the float source formats (SJPEG_HIP_SRC_RGB_PLANAR_F32 / _F16 / _BF16, above): a sample x is
 * coded as the byte rint(clamp(fmaf(x, scale, bias), 0, 255)).  255 and 0 when the engine is made (values in 0..1);
 * 127.5 and 127.5 take values in -1..1.  Engine state: sticky until set again, inherited by everything a call runs on
 * the engine's behalf, ignored by every other format.  A non-finite scale or bias is SJPEG_HIP_EINVAL and changes
 * nothing.  Not ordered on any stream: it holds for the calls made after it. */
int sjpeg_hip_engine_set_pixel_transform(sjpeg_hip_engine* engine, float scale, float bias);
int sjpeg_hip_engine_get_pixel_transform(const sjpeg_hip_engine* engine, float* scale, float* bias);
/* The same transform per channel: a sample x of channel c (0, 1, 2 = R, G, B; gray: 0) is coded as the byte
 * rint(clamp(fmaf(x, scale[c], bias[c]), 0, 255)) -- pictures normalised with a per-channel mean and std go in with
 * scale[c] = 255 * std[c], bias[c] = 255 * mean[c].  Read by every float source format.  The call above sets the three
 * channels alike and its getter reports channel 0.  A non-finite entry is SJPEG_HIP_EINVAL and changes nothing. */
int sjpeg_hip_engine_set_pixel_transform3(sjpeg_hip_engine* engine, const float scale[3], const float bias[3]);
int sjpeg_hip_engine_get_pixel_transform3(const sjpeg_hip_engine* engine, float scale[3], float bias[3]);
int sjpeg_hip_engine_wait(sjpeg_hip_engine* engine, void* stream);

/* A batch whose frames each carry their OWN tables and header -- what a batch of the reference's
 * default encodes is (method 4: per-image adapted quantizer and per-image optimised Huffman
 * codes, src/enc.cc:801-812 + 323-372, one Encoder per image there, one launch here).
 * tables[nframes] (host); headers = the frames' header bytes back to back (host), frame f owns
 * [header_offsets[f], header_offsets[f+1]); flags must agree between the frames.  The rest as
 * sjpeg_hip_encode_scan_src() / sjpeg_hip_scan_symbol_stats_src(). */
int sjpeg_hip_encode_scan_multi(sjpeg_hip_engine* engine, const sjpeg_hip_source* src,
                                int width, int height, int yuv_mode, int nframes,
                                const sjpeg_hip_scan_tables* tables /*[nframes]*/,
                                const void* headers, const size_t* header_offsets /*[nframes+1]*/,
                                int append_eoi, void* d_out, size_t out_stride, uint64_t* d_sizes,
                                void* stream);
int sjpeg_hip_scan_symbol_stats_multi(sjpeg_hip_engine* engine, const sjpeg_hip_source* src,
                                      int width, int height, int yuv_mode, int nframes,
                                      const sjpeg_hip_scan_tables* tables /*[nframes]*/,
                                      uint32_t* d_freq, void* stream);

/* A RAGGED batch: pictures of different sizes in one call -- a gallery's thumbnails, an upload queue, a dataset being
 * re-encoded.  Frame f has its own planes, row strides, width and height (1..65535 each) and its own place in d_out:
 * [out_offset, out_offset + out_capacity).  The frames share the source format, the yuv_mode and method 0 (fixed
 * quantizer, default Huffman codes; the other methods: sjpeg_hip_encode_ragged_batch_src below); tables_per_frame = 0: tables[0] codes every frame, 1: frame f is coded with
 * tables[f] (per-frame quality).  headers / header_offsets[nframes + 1] as sjpeg_hip_encode_scan_multi() (both NULL:
 * no headers).  The bytes of frame f are what sjpeg_hip_encode_scan_src() makes of that picture alone.
 *   d_sizes[f] = frame f's size, or 0 when it does not fit its out_capacity (every other frame is still exact; nothing
 *   is written outside any frame's range).  sjpeg_hip_frame_bound() gives a capacity every frame fits.
 *   Asynchronous on `stream`.  In pipelined mode the call runs ordered, behind the engine's stitch stream.  A batch
 *   whose scratch would pass SJPEG_HIP_SCRATCH_LIMIT_BYTES goes in several launches of consecutive frames.
 *   SJPEG_HIP_EINVAL (the message names the frame) for: nframes outside 1..65535, a format that does not match
 *   yuv_mode, a null plane, |row_stride| below a row of the plane, bad dimensions, header offsets that do not ascend,
 *   out_offset + out_capacity past 2^64, and tables with SJPEG_HIP_QUANT_TRELLIS, _KEEP, _REPLAY or
 *   SJPEG_HIP_RESTART_MARKERS (not taken here).
 * The scratch is laid out frame after frame by prefix sums -- sized by each frame's own capacity, not nframes times
 * the largest -- and every kernel runs a flat grid over the batch's total work. */
typedef struct sjpeg_hip_ragged_frame {
  const void* plane[3];        /* DEVICE pointers, laid out as `format` says (as sjpeg_hip_source) */
  int64_t row_stride[3];       /* bytes between rows of each plane; may be negative */
  int32_t width, height;       /* 1..65535 each */
  uint64_t out_offset;         /* where this frame's JPEG starts in d_out */
  uint64_t out_capacity;       /* bytes it may take, e.g. sjpeg_hip_frame_bound(width, height, yuv_mode, header bytes) */
} sjpeg_hip_ragged_frame;

int sjpeg_hip_encode_ragged_src(sjpeg_hip_engine* engine, int format, int yuv_mode, int nframes,
                                const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                const sjpeg_hip_scan_tables* tables, int tables_per_frame,
                                const void* headers, const size_t* header_offsets /*[nframes+1]*/,
                                int append_eoi, void* d_out, uint64_t* d_sizes, void* stream);

/* The two analysis passes over a ragged batch (frames[] as above; out_offset / out_capacity are ignored).
 *   sjpeg_hip_scan_histogram_ragged_src: d_hist[nframes][2][64][128] (uint32), frame f's what
 *   sjpeg_hip_scan_histogram_src() makes of that picture alone.  sjpeg_hip_scan_symbol_stats_ragged_src:
 *   d_freq[nframes][2][272] (uint32), frame f's what sjpeg_hip_scan_symbol_stats_src() makes of that picture alone with
 *   tables[f] (tables_per_frame = 1) or tables[0] (0).  Asynchronous on `stream`; in pipelined mode they run ordered.
 *   The partials of a batch that would pass SJPEG_HIP_SCRATCH_LIMIT_BYTES go in several launches of consecutive frames.
 *   SJPEG_HIP_EINVAL (the message names the frame) as sjpeg_hip_encode_ragged_src(). */
int sjpeg_hip_scan_histogram_ragged_src(sjpeg_hip_engine* engine, int format, int yuv_mode, int nframes,
                                        const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, uint32_t* d_hist,
                                        void* stream);
int sjpeg_hip_scan_symbol_stats_ragged_src(sjpeg_hip_engine* engine, int format, int yuv_mode, int nframes,
                                           const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                           const sjpeg_hip_scan_tables* tables, int tables_per_frame,
                                           uint32_t* d_freq, void* stream);

/* A RAGGED batch with the reference's per-picture analysis, methods 0..6: the defaults (method 4) of SjpegCompress()
 * over pictures of different sizes.  Complete JPEGs, EOI included: frame f's bytes are what
 * sjpeg_hip_encode_batch_src() makes of that picture alone with the starting matrix quant[f] (quant_per_frame = 1:
 * per-frame quality) or quant[0] (0), and the same min_quant, q_bias, method and qdelta limits.  Frame f goes to
 * [out_offset, out_offset + out_capacity) of d_out; d_sizes[f] = 0 when it does not fit (nothing written, the others
 * exact) -- sjpeg_hip_frame_bound(w, h, yuv_mode, 2048) is always enough.  The engine builds every frame's header from
 * its own size, adapted matrices and optimised codes.  Method 0 is one sjpeg_hip_encode_ragged_src() call.
 *   The host waits where sjpeg_hip_encode_batch_src() does -- for the adapted matrices (methods 3..6), for the symbol
 *   counts (1, 2, 4, 5, 6) --; the encode is asynchronous on `stream`.  In pipelined mode the call runs ordered.
 *   SJPEG_HIP_EINVAL: every check of sjpeg_hip_encode_ragged_src(), a NULL quant, a method outside 0..6 (the trellis
 *   methods go through sjpeg_hip_encode_ragged_trellis_src() or the host API) and qdelta_max outside -12..12. */
int sjpeg_hip_encode_ragged_batch_src(sjpeg_hip_engine* engine, int format, int yuv_mode, int nframes,
                                      const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                      const uint8_t (*quant)[2][64], int quant_per_frame,
                                      const uint8_t* min_quant /*[2][64] or NULL*/, int q_bias, int method,
                                      int qdelta_max_luma, int qdelta_max_chroma,
                                      void* d_out, uint64_t* d_sizes, void* stream);

/* ---- ragged batches with the reference's SJPEG_YUV_AUTO decision and the sharp conversion ----
 * sjpeg_hip_riskiness_ragged_src: d_sums[nframes][3] (device), frame f's what sjpeg_hip_riskiness_sums() makes of that
 *   picture alone (all zero for a 1 x N or N x 1 frame).  format: RGB, BGRA, RGBA or planar RGB; frames[] as above, out_offset /
 *   out_capacity ignored; any row stride, negative ones too.  d_table: the 117649-byte table in device memory, or NULL:
 *   the table SjpegRiskiness() uses (installed, SJPEG_HIP_RISKINESS_TABLE, riskiness.bin beside the library; the
 *   engine keeps a device copy).  Asynchronous on `stream`.
 * sjpeg_hip_riskiness_verdict: SjpegRiskiness' arithmetic (src/jpeg_tools.cc:212-236) on one frame's three sums, host
 *   only: the SjpegYUVMode it decides; *risk (if not NULL) the score 0..100.
 * sjpeg_hip_sharp_yuv_ragged: the sharp conversion of every frame into its own tightly packed planes d_y[f] (width x
 *   height), d_u[f], d_v[f] (((width+1)/2) x ((height+1)/2)) -- host arrays of device pointers --, each frame's bytes
 *   those of sjpeg_hip_sharp_yuv() for that picture alone.  d_workspace: sjpeg_hip_sharp_ragged_workspace() bytes of
 *   device memory.  Asynchronous on `stream` only; the sweeps' launches never hold more workgroups than the device holds
 *   at once.
 * sjpeg_hip_encode_ragged_auto_src: sjpeg_hip_encode_ragged_batch_src() with the SjpegYUVMode of EncoderParam:
 *   SJPEG_YUV_AUTO (0): the riskiness of every frame decides its mode (420, sharp 420, 444 or 400), as
 *   SjpegEncode(..., SJPEG_YUV_AUTO) decides it for that picture alone; SJPEG_YUV_SHARP (2): every frame goes through
 *   the sharp conversion; 1, 3, 4 (= SJPEG_HIP_YUV420 / 444 / 400): exactly sjpeg_hip_encode_ragged_batch_src().
 *   AUTO and SHARP take RGB, BGRA, RGBA or planar RGB sources.  modes[f] (host, or NULL): the SjpegYUVMode frame f was coded with.
 *   Frame f's bytes are what SjpegEncode(picture, q, method, yuv_mode) makes of it alone; d_sizes[f] and the output
 *   ranges are in the caller's frame order; sjpeg_hip_frame_bound(w, h, SJPEG_HIP_YUV444, 2048) is always enough.
 *   Host waits: the riskiness sums (AUTO only), then those of sjpeg_hip_encode_ragged_batch_src() once over all modes.
 *   The sharp planes and workspace count against SJPEG_HIP_SCRATCH_LIMIT_BYTES: past it, the call goes in parts of
 *   consecutive frames.  SJPEG_HIP_EINVAL for every check of sjpeg_hip_encode_ragged_batch_src(), yuv_mode outside
 *   0..4, AUTO or SHARP with another source format, methods outside 0..6. */
int sjpeg_hip_riskiness_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                                   const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                   const uint8_t* d_table /*or NULL*/, uint64_t* d_sums /*[nframes][3]*/,
                                   void* stream);
int sjpeg_hip_riskiness_verdict(const uint64_t sums[3], int width, int height, float* risk);
size_t sjpeg_hip_sharp_ragged_workspace(int nframes, const sjpeg_hip_ragged_frame* frames);
int sjpeg_hip_sharp_yuv_ragged(sjpeg_hip_engine* engine, int format, int nframes,
                               const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                               uint8_t* const* d_y, uint8_t* const* d_u, uint8_t* const* d_v,
                               void* d_workspace, size_t workspace_size, void* stream);
int sjpeg_hip_encode_ragged_auto_src(sjpeg_hip_engine* engine, int format, int yuv_mode, int nframes,
                                     const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                     const uint8_t (*quant)[2][64], int quant_per_frame,
                                     const uint8_t* min_quant /*[2][64] or NULL*/, int q_bias, int method,
                                     int qdelta_max_luma, int qdelta_max_chroma,
                                     void* d_out, uint64_t* d_sizes, int* modes /*[nframes], host, or NULL*/,
                                     void* stream);

/* ---- ragged batches with trellis quantization: the reference's methods 7 (= 4 + trellis) and 8 (= 6 + trellis) ----
 * sjpeg_hip_encode_ragged_trellis_src: the arguments, output contract and host waits of
 *   sjpeg_hip_encode_ragged_auto_src(); frame f's bytes are what SjpegEncode(picture, q, method, yuv_mode) makes of it
 *   alone.  yuv_mode 1 / 3 / 4 with any source layout; 0 (SJPEG_YUV_AUTO) and 2 (SJPEG_YUV_SHARP) with RGB, BGRA or RGBA
 *   (packed) or planar RGB.
 *   The flow per picture is Encoder::Encode's (src/enc.cc:121-129, 323-372): histogram and adapted matrices, then ONE
 *   trellis quantization (src/quantize.cc:325-457) in the statistics pass, its rate priced with the standard AC code
 *   lengths, then the optimised codes and an encode pass that REPLAYS the quantized blocks the statistics pass kept --
 *   no pixel read, no second trellis.  The kept blocks are engine scratch, 36 864 bytes a segment
 *   (sjpeg_hip_segment_count()), laid out by the frames' prefix sums; together with the sharp planes they count against
 *   SJPEG_HIP_SCRATCH_LIMIT_BYTES: past it the call goes in parts of consecutive frames, each a complete flow with its
 *   own waits.  sjpeg_hip_engine_trim() gives them back.  Asynchronous encode on `stream`, ordered in pipelined mode.
 *   SJPEG_HIP_EINVAL (the frame named): every check of sjpeg_hip_encode_ragged_auto_src(), and a method other than 7
 *   or 8 (methods 0..6 are that call's). */
int sjpeg_hip_encode_ragged_trellis_src(sjpeg_hip_engine* engine, int format, int yuv_mode, int nframes,
                                        const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                        const uint8_t (*quant)[2][64], int quant_per_frame,
                                        const uint8_t* min_quant /*[2][64] or NULL*/, int q_bias, int method /*7 or 8*/,
                                        int qdelta_max_luma, int qdelta_max_chroma,
                                        void* d_out, uint64_t* d_sizes, int* modes /*[nframes], host, or NULL*/,
                                        void* stream);

/* ---- ragged batches searched to a per-picture target size or PSNR ----
 * The two measurements of the reference's multi-pass search (Encoder::LoopScan, src/dichotomy.cc:113-205) over a ragged
 * batch (frames[] as above, out_offset / out_capacity ignored; tables[f] with tables_per_frame = 1, else tables[0]):
 * sjpeg_hip_scan_quant_error_ragged_src: d_err[nframes] (device), frame f's what sjpeg_hip_scan_quant_error_src() makes
 *   of that picture alone (QuantizeError summed as Encoder::ComputePSNR does).  Asynchronous on `stream`.
 * sjpeg_hip_scan_counted_bits_ragged_src: d_bits[nframes] (device), what the reference's BitCounter reports for frame f's
 *   scan with its tables (src/bit_writer.h:292-365): the entropy bits plus 8 for every 0xFF among the COMPLETED bytes
 *   (the 1-padded last byte does not count).  The ragged encode without its output: the segment scratch is planned
 *   from the host API's first capacity; a frame whose segments overflow that plan is counted again with its
 *   sjpeg_hip_frame_bound() plan in a second launch of only those frames.  One host wait (which frames overflowed), and
 *   one more after a recount; a frame past even its worst-case plan is SJPEG_HIP_ERUNTIME, naming it.
 * Both refuse trellis, keep / replay and restart flags, split into several launches under
 * SJPEG_HIP_SCRATCH_LIMIT_BYTES, run ordered in pipelined mode and name the offending frame in sjpeg_hip_last_error().
 *
 * sjpeg_hip_encode_ragged_search_src: sjpeg_hip_encode_ragged_batch_src() with the search.  Frame f's bytes are what
 *   the reference's sjpeg::Encode() makes of that picture alone with its starting matrices quant[f] (quant[0] when
 *   quant_per_frame = 0), min_quant, q_bias, the qdelta limits, Huffman_compress = (method not in {0, 3}),
 *   adaptive_quantization = (method >= 3) and search[f] (search[0] when search_per_frame = 0).  q_out[f] / value_out[f]
 *   (host, or NULL): the SearchHook's best_q and best_result after the call, -1 for a frame that was not searched
 *   (passes <= 1).  A call in which no frame is searched is sjpeg_hip_encode_ragged_batch_src().
 *   Every pass is one launch over the frames still searching: the adaptation of their kept histograms to the pass's
 *   matrices (methods 3..6), then one measurement -- symbol statistics (size, optimised codes), counted bits (size,
 *   methods 0 and 3) or the quantization error (PSNR).  Host waits per pass: two for methods 3..6 (matrices back,
 *   measurements back), one otherwise; a count that overflowed its first plan adds one.  These are per SEARCH: the
 *   frames with size targets and those with PSNR targets are searched one after the other, and so are the parts
 *   below, so a call with both kinds of target, or in P parts, waits up to twice, or P times, as often.  A frame leaves
 *   the search when its SearchHook is done.  The frames are then coded with their best matrices, without further adaptation, by
 *   the method 1 (optimised codes) or 0 flow of sjpeg_hip_encode_ragged_batch_src().  The kept histograms and the
 *   partials count against SJPEG_HIP_SCRATCH_LIMIT_BYTES: past it the call goes in parts of consecutive frames, each a
 *   complete search.  yuv_mode: 1, 3 or 4.  SJPEG_HIP_EINVAL for every check of sjpeg_hip_encode_ragged_batch_src(), a
 *   NULL search, target_mode other than 1 or 2 and a non-finite target_value. */
typedef struct sjpeg_hip_search {
  int32_t target_mode;   /* 1 = size in bytes (EncoderParam::TARGET_SIZE), 2 = PSNR in dB (TARGET_PSNR) */
  float target_value;
  int32_t passes;        /* clamped to 1..20 (src/api.cc:169); a frame with passes <= 1 is not searched */
  float tolerance;       /* percent, as EncoderParam::tolerance (default 1) */
  float qmin, qmax;      /* as EncoderParam (defaults 0, 100) */
} sjpeg_hip_search;

int sjpeg_hip_scan_quant_error_ragged_src(sjpeg_hip_engine* engine, int format, int yuv_mode, int nframes,
                                          const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                          const sjpeg_hip_scan_tables* tables, int tables_per_frame,
                                          uint64_t* d_err /*[nframes]*/, void* stream);
int sjpeg_hip_scan_counted_bits_ragged_src(sjpeg_hip_engine* engine, int format, int yuv_mode, int nframes,
                                           const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                           const sjpeg_hip_scan_tables* tables, int tables_per_frame,
                                           uint64_t* d_bits /*[nframes]*/, void* stream);
int sjpeg_hip_encode_ragged_search_src(sjpeg_hip_engine* engine, int format, int yuv_mode, int nframes,
                                       const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                       const uint8_t (*quant)[2][64], int quant_per_frame,
                                       const uint8_t* min_quant /*[2][64] or NULL*/, int q_bias, int method,
                                       int qdelta_max_luma, int qdelta_max_chroma,
                                       const sjpeg_hip_search* search, int search_per_frame,
                                       float* q_out /*[nframes], host, or NULL*/, float* value_out /*[nframes], host, or NULL*/,
                                       void* d_out, uint64_t* d_sizes, void* stream);

/* ---- ragged batches into ONE packed buffer: the frames back to back ---------------------
 * sjpeg_hip_encode_ragged_packed_src: any of the ragged encodes above, with the frames written back to back into
 * d_packed instead of each into a slot [out_offset, out_offset + out_capacity) sized before it is coded.  It goes where
 * the same arguments go in the unpacked calls and refuses what those refuse, with their messages:
 *   params->search != NULL          sjpeg_hip_encode_ragged_search_src (yuv_mode 1 / 3 / 4, methods 0..6)
 *   method 7 or 8                   sjpeg_hip_encode_ragged_trellis_src
 *   otherwise                       sjpeg_hip_encode_ragged_auto_src (yuv_mode 1 / 3 / 4: ..._batch_src)
 * Frame f's bytes are exactly those of that call.  frames[f].out_offset is ignored; frames[f].out_capacity is the most
 * frame f may take and still plans its segment scratch.  modes / q_out / value_out (host, each may be NULL): as in the
 * unpacked calls; a flow that has no modes reports yuv_mode, one without a search -1 for q and value.
 * Also SJPEG_HIP_EINVAL: a NULL engine, params, frames, d_packed, d_offsets or d_sizes; d_packed not a multiple of 16.
 * Layout:
 *   - d_sizes[f] and d_offsets[f] are indexed by the caller's frame number.  Frame f lies at d_packed + d_offsets[f],
 *     a multiple of 16; the bytes between its end and the next multiple of 16 are zero.
 *   - The frames lie back to back in the order the flow codes them.  That IS the caller's order (offsets ascending: the
 *     format sjpeg_hip_gather_streams takes) whenever the call codes its frames as one group: yuv_mode 1 / 3 / 4 or
 *     SJPEG_YUV_SHARP, and either no frame searched or every frame searched (whatever their targets: the searches run
 *     per kind of target, the final encode over all of them).  With SJPEG_YUV_AUTO the frames lie grouped by the mode
 *     each was given (4:2:0, 4:4:4, 4:0:0, sharp), and in a search of only some frames the ones that are not searched
 *     (passes <= 1) come first, then the searched ones; the caller's order inside each group.  Launches over
 *     SJPEG_HIP_SCRATCH_LIMIT_BYTES do not change this; a call cut into parts is grouped inside each part, so a
 *     one-group call keeps the caller's order there too.
 *   - A frame that did not fit its own out_capacity has size 0 and takes no room.  A frame whose padded end would pass
 *     packed_capacity has size 0 and is not written, bit 63 of d_offsets[nframes] (SJPEG_HIP_PACKED_OVERFLOW) is set,
 *     and every frame coded after it is dropped as well; the low 63 bits then hold the capacity that would have been
 *     enough.  Without overflow d_offsets[nframes] is the number of bytes used.  Nothing is written outside
 *     [d_packed, d_packed + packed_capacity).
 *   - d_offsets[f] of a frame with size 0 is not a place in the buffer: a frame dropped for lack of room holds the start
 *     it would have had, which can lie past packed_capacity, and a frame that failed its own out_capacity holds the
 *     start of the frame coded after it.  Use d_offsets[f] only where d_sizes[f] != 0.
 * Placement is device work on the caller's stream (a cursor in engine memory that the call zeroes and every launch,
 * group and part of it advances): no host wait is added, and in pipelined mode the call runs ordered. */
typedef struct sjpeg_hip_ragged_params {
  int32_t yuv_mode;                 /* SjpegYUVMode 0..4 */
  int32_t method;                   /* 0..8 */
  const uint8_t (*quant)[2][64];    /* starting matrices */
  int32_t quant_per_frame;
  const uint8_t* min_quant;         /* [2][64] or NULL */
  int32_t q_bias, qdelta_max_luma, qdelta_max_chroma;
  const sjpeg_hip_search* search;   /* NULL: no search */
  int32_t search_per_frame;
} sjpeg_hip_ragged_params;

int sjpeg_hip_encode_ragged_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                       const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                       const sjpeg_hip_ragged_params* params,
                                       void* d_packed, size_t packed_capacity,
                                       uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                       int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                       void* stream);

/* ---- ragged batches with EVERY combination of sjpeg_hip_ragged_params: the search with any sampling and the trellis ----
 * sjpeg_hip_encode_ragged_full_src: yuv_mode 0..4, method 0..8, search NULL or not (per frame or shared), in one call.
 *   Frame f's bytes are what the reference's sjpeg::Encode() makes of that picture alone with yuv_mode as given,
 *   Huffman_compress = (method not in {0, 3}), adaptive_quantization = (method >= 3), use_trellis = (method >= 7) and
 *   search[f].  Frame f goes to [out_offset, out_offset + out_capacity) of d_out; modes / q_out / value_out (host, each
 *   may be NULL) as in sjpeg_hip_encode_ragged_packed_src.  A frame with passes <= 1 is coded by the unsearched flow of
 *   the same method and mode and reports -1 in q_out / value_out.
 *   What an older entry point takes is handed to its flow and gives its bytes: no frame searched --
 *   sjpeg_hip_encode_ragged_auto_src / _trellis_src; a search with yuv_mode 1 / 3 / 4 and methods 0..6 --
 *   sjpeg_hip_encode_ragged_search_src.  The flow of this call covers a search (some frame with passes > 1) with
 *   SJPEG_YUV_AUTO or SJPEG_YUV_SHARP, with method 7 or 8, or both -- Encoder::LoopScan (src/dichotomy.cc:113-205) with
 *   the mode decision of src/encoders.cc:549-551 in front and, for the trellis, StoreRunLevels (src/dichotomy.cc:80-111):
 *   - SJPEG_YUV_AUTO: one ragged riskiness and one wait, then the verdicts: the frames stand in mode groups (4:2:0, 4:4:4,
 *     4:0:0 of the caller's format, sharp).  The sharp frames (all frames under SJPEG_YUV_SHARP) are converted ONCE into
 *     planar 4:2:0 planes in engine scratch and searched as a SJPEG_HIP_SRC_YUV420 group.
 *   - Every pass launches over ALL groups, then waits: the host waits per pass are those of
 *     sjpeg_hip_encode_ragged_search_src (two for methods 3..8, one otherwise, one more after a recount), per kind of
 *     target and per part, whatever the number of groups.
 *   - Methods 7 and 8 with a size target: each pass's statistics launch quantizes with the trellis and keeps its blocks;
 *     frame f is priced with ITS accumulated rate table -- the standard AC lengths, and after every pass the lengths of the
 *     symbols that pass's optimised AC tables have (InitCodes(true), src/dichotomy.cc:86,152, src/entropy.cc:116-128).
 *     With a PSNR target the passes measure the plain quantization error (ComputePSNR does not use the trellis).
 *   - The end (src/dichotomy.cc:178-201): a size-searched trellis frame whose last pass was its best is NOT quantized
 *     again -- its stream replays the blocks that pass kept, with the codes that pass compiled.  Every other trellis frame
 *     gets one more trellis statistics pass with its best matrices (no adaptation) and its rate table as it stands, then
 *     the replay.  Frames of methods 0..6 end as in sjpeg_hip_encode_ragged_search_src: method 1 or 0 with the best
 *     matrices, over all groups at once.
 *   - A frame's kept blocks (36 864 bytes a segment) lie at ONE place for the whole part, whichever frames a launch
 *     covers; the replay covers all trellis frames of a group in one launch.  The kept histograms, the sharp planes and
 *     workspace and the kept blocks count against SJPEG_HIP_SCRATCH_LIMIT_BYTES: past it the call goes in parts of
 *     consecutive searched frames, each a complete search.
 *   AUTO and SHARP take RGB, BGRA or RGBA (packed) or planar RGB sources.
 *   SJPEG_HIP_EINVAL (the message names the argument or the frame): a
 *   NULL engine, params, frames, d_out, d_sizes or params->quant; nframes outside 1..65535; yuv_mode outside 0..4; method
 *   outside 0..8; qdelta_max outside -12..12; a target_mode other than 1 or 2 or a non-finite target_value in any search
 *   entry; and every frame check of sjpeg_hip_encode_ragged_src.  No restart markers.  Per-picture metadata:
 *   sjpeg_hip_encode_ragged_full_meta_src, below.
 * sjpeg_hip_encode_ragged_full_packed_src: the same call into ONE packed buffer -- the arguments and the layout contract
 *   of sjpeg_hip_encode_ragged_packed_src.  A searched SJPEG_YUV_AUTO call lays its frames out as that contract says:
 *   the frames that are not searched first, then (per part) the searched ones grouped by the mode each was given.
 * sjpeg_hip_engine_search_stats: counters of the engine's most recent _full_ call that took the flow above (all zero
 *   after a call that was handed to an older flow).  Host values; the call does not synchronise.
 *   [0] most passes any frame ran, [1] measurement launches (one per group and pass; recounts too), [2] host waits of the
 *   call (those of the unsearched frames' flow and of the method 1 ending counted as documented for one part), [3] frames
 *   whose stream replays the blocks their own last search pass kept, [4] frames quantized once more after the search,
 *   [5] trellis statistics launches. */
int sjpeg_hip_encode_ragged_full_src(sjpeg_hip_engine* engine, int format, int nframes,
                                     const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                     const sjpeg_hip_ragged_params* params, void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                     int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_full_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                            const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                            const sjpeg_hip_ragged_params* params,
                                            void* d_packed, size_t packed_capacity,
                                            uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                            int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                            void* stream);
int sjpeg_hip_engine_search_stats(sjpeg_hip_engine* engine, uint64_t stats[6]);

/* ---- ragged batches whose pictures carry metadata: EXIF, ICC profile, XMP, raw APP markers ----
 * sjpeg_hip_metadata_size (host only): *size = the bytes sjpeg_hip_make_header_meta() puts between SOI + APP0 (20 bytes)
 *   and the DQT segment for this metadata; 0 for NULL or all-empty metadata.  SJPEG_HIP_EINVAL, sjpeg_hip_last_error()
 *   naming the member, for what the reference refuses (src/headers.cc:72-180) -- EXIF whose APP1 segment would pass
 *   0xFFFF bytes, an ICC profile of 256 chunks or more, an XMP packet too long for one APP1 segment (above 65 504
 *   bytes) without a well-formed xmpNote:HasExtendedXMP=" note in front of the split point, or above 2^31 bytes -- and
 *   for a NULL pointer with a non-zero size.
 * sjpeg_hip_encode_ragged_full_meta_src / _full_meta_packed_src: sjpeg_hip_encode_ragged_full_src / _full_packed_src with
 *   `meta`, a HOST array (sjpeg_hip_metadata, with sjpeg_hip_make_header_meta below): frame f carries meta[f]
 *   (meta_per_frame = 1) or meta[0] (0).  meta == NULL is exactly the call without metadata.
 *   Frame f's bytes are what the reference's sjpeg::Encode() makes of that picture alone with the EncoderParam the _full_
 *   call describes plus app_markers, exif, iccp, xmp and xmp_split_point of its metadata.  Without a size target those
 *   are the bytes of the same call without metadata with the metadata segments inserted behind byte 20.  A size search
 *   counts the metadata into the size it aims at, as Encoder::HeaderSize() does (src/dichotomy.cc:210-241), and may so
 *   choose another quality; a PSNR search is not affected.  modes, q_out, value_out, d_sizes, the frame order of a packed
 *   buffer, the host waits and sjpeg_hip_engine_search_stats keep their meaning.
 *   Invalid metadata in any frame is SJPEG_HIP_EINVAL before any device work; the message names the entry, the frame and
 *   the member.  sjpeg_hip_frame_bound(w, h, SJPEG_HIP_YUV444, 2048 + sjpeg_hip_metadata_size()) is always enough for a
 *   frame; one that does not fit its out_capacity reports size 0, nothing is written outside any frame's range and the
 *   others stay exact.  The headers of one launch are staged in engine scratch (sjpeg_hip_engine_scratch_bytes,
 *   sjpeg_hip_engine_trim): they count against SJPEG_HIP_SCRATCH_LIMIT_BYTES and stay below 4 GiB, a larger batch goes
 *   in more launches.  A header above 2048 bytes is placed with 16-byte stores. */
struct sjpeg_hip_metadata;
int sjpeg_hip_metadata_size(const struct sjpeg_hip_metadata* meta, size_t* size);
int sjpeg_hip_encode_ragged_full_meta_src(sjpeg_hip_engine* engine, int format, int nframes,
                                          const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                          const sjpeg_hip_ragged_params* params,
                                          const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                          void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                          int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_full_meta_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                 const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                                 const sjpeg_hip_ragged_params* params,
                                                 const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                                 void* d_packed, size_t packed_capacity,
                                                 uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                                 int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                                 void* stream);

/* ---- pictures reduced inside the ragged call: thumbnails and pyramid levels ----
 * A thumbnail service, a srcset or DeepZoom pyramid, a dataset preview: each picture at 1/2, 1/4 or 1/8 of its size.
 * Frame f has a factor s = factors[f] in 1..SJPEG_HIP_REDUCE_MAX.  Its reduced picture is w' = (W + s - 1) / s by
 * h' = (H + s - 1) / s; sample (x', y', c) is
 *     sum = the sum over dy < s, dx < s of b(min(x' * s + dx, W - 1), min(y' * s + dy, H - 1), c)
 *     out = (sum + s * s / 2) / (s * s)                        integer arithmetic, exact: round half up
 * where b is the byte the encoder sees at that source pixel today: R, G, B of the packed and planar byte formats (alpha
 * is not part of it), the float formats through the engine's pixel transform (above), the gray value of the gray
 * formats.  Edges replicate the last column and row: a 17-wide picture at s = 8 gives 3 columns, the last made of one
 * source column.  s = 1 is the identity.  THE CONTRACT: the JPEG of a reduced frame is byte for byte what the same call
 * makes of the uint8 picture so defined handed over as SJPEG_HIP_SRC_RGB (the gray formats: SJPEG_HIP_SRC_GRAY, yuv_mode
 * 4:0:0 only).  Formats: every RGB-like one (RGB, BGRA, RGBA, planar RGB, all their float forms) and the four gray ones;
 * strides of either sign, element-only alignment, and no element read that is not a used sample of a pixel of the
 * picture, as everywhere.  The planar and semi-planar YUV formats (YUV444, YUV420, NV12, NV21) are not reduced: with a
 * factor above 1 they are SJPEG_HIP_EINVAL, the message names the format.
 * A pyramid is the same picture listed several times, with factors 1, 2, 4, 8 (every level reads the source again).
 *
 * sjpeg_hip_reduced_size (host only): w' and h'.  SJPEG_HIP_EINVAL for a factor outside 1..8 or dimensions outside
 *   1..65535.
 * sjpeg_hip_reduce_ragged_bytes (host only): the bytes the reduced pictures of a batch take, 0 on bad arguments
 *   (factors NULL: all 1).  THE LAYOUT: interleaved uint8 R, G, B (one gray plane for the gray formats); a picture's rows
 *   are its row bytes rounded up to a multiple of 4 apart, every picture starts at a multiple of 16 from the buffer's
 *   start, frame after frame in the caller's order.  The padding behind a row and behind a picture may hold anything
 *   and lies inside the buffer.  (So the kernel stores whole dwords; beside the sources it is their size divided by
 *   s * s, plus that padding.)
 * sjpeg_hip_reduce_ragged_src: ONE launch over the batch's tiles into d_reduced (a multiple of 16, reduced_bytes
 *   behind it), asynchronous on `stream` and ordered as every engine call is, pipelined mode included.  It fills
 *   reduced_frames[f] (host) with plane[0], row_stride[0], w' and h' -- out_offset / out_capacity are copied from
 *   frames[f] -- and sets *reduced_format to SJPEG_HIP_SRC_RGB or SJPEG_HIP_SRC_GRAY: the pair goes to any ragged entry.
 *   It takes an engine because the float formats read its pixel transform.  SJPEG_HIP_EINVAL before any device work, the
 *   frame named as the ragged entries name it: a factor outside 1..8, a YUV-plane format, reduced_bytes below
 *   sjpeg_hip_reduce_ragged_bytes(), and every frame check of sjpeg_hip_encode_ragged_src.
 * sjpeg_hip_encode_ragged_reduced_src / _reduced_packed_src: the arguments and the output contract of
 *   sjpeg_hip_encode_ragged_full_meta_src / _full_meta_packed_src, plus `factors` (host, uint8[nframes]).
 *   factors == NULL or every factor 1: exactly that call on the caller's frames, any format; no copy, no kernel.
 *   Otherwise every frame goes through the reduce kernel into engine memory -- the frames with s = 1 too: they are
 *   copied or converted, which the formats' own contracts make byte-exact, so that ONE inner call codes the batch as one
 *   group of one format: frame order, packed layout, modes, q_out, value_out, the host waits and
 *   sjpeg_hip_engine_search_stats are those of that call on the reduced pictures (SJPEG_YUV_AUTO decides on the REDUCED
 *   picture).  out_capacity is the caller's: sjpeg_hip_frame_bound(w', h', SJPEG_HIP_YUV444, 2048 + metadata) is always
 *   enough.  The reduced pictures live in engine memory of their own, one allocation (not the arena of the sharp planes),
 *   counted by sjpeg_hip_engine_scratch_bytes and released by sjpeg_hip_engine_trim; a failure to get it is
 *   SJPEG_HIP_ENOMEM naming the bytes.  A later call on the engine writes them behind everything the earlier one queued
 *   (the engine's ordering between streams; two calls on one stream are ordered by it).  SJPEG_HIP_EINVAL before any
 *   device work: the checks above, gray with a yuv_mode other than 4:0:0, and every check of the inner call. */
#define SJPEG_HIP_REDUCE_MAX 8
int sjpeg_hip_reduced_size(int width, int height, int factor, int* reduced_width, int* reduced_height);
size_t sjpeg_hip_reduce_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                     const uint8_t* factors /*host uint8[nframes], or NULL*/);
int sjpeg_hip_reduce_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                                const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                const uint8_t* factors /*host uint8[nframes]*/, void* d_reduced, size_t reduced_bytes,
                                sjpeg_hip_ragged_frame* reduced_frames /*host out [nframes]*/, int* reduced_format,
                                void* stream);
int sjpeg_hip_encode_ragged_reduced_src(sjpeg_hip_engine* engine, int format, int nframes,
                                        const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                        const sjpeg_hip_ragged_params* params, const uint8_t* factors /*host uint8[nframes], or NULL*/,
                                        const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                        void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                        int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_reduced_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                               const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                               const sjpeg_hip_ragged_params* params, const uint8_t* factors /*host uint8[nframes], or NULL*/,
                                               const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                               void* d_packed, size_t packed_capacity,
                                               uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                               int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                               void* stream);

/* ---- pictures resized inside the ragged call: thumbnails that fit a box ----
 * What a thumbnail service, a srcset or a dataset preview asks for is a fixed box -- "fit in 256 x 256", "320 wide" --,
 * which the integer factors above do not give.  Frame f of W x H is resized to w' x h' = sizes[f], 1 <= w' <= W and
 * 1 <= h' <= H: smaller or equal on each axis, never larger.  The result is the EXACT area average, in integers.  Along
 * x both pictures lie on a grid of W * w' units: source column x covers [x * w', (x + 1) * w'), output column x' covers
 * [x' * W, (x' + 1) * W), and
 *     wx(x', x) = max(0, min((x + 1) * w', (x' + 1) * W) - max(x * w', x' * W))        (over x it sums to W)
 *     wy(y', y)   the same with H and h'                                                (over y it sums to H)
 *     S   = the sum over y of wy(y', y) * the sum over x of wx(x', x) * b(x, y, c)      (64 bits: S <= 255 W H < 2^40)
 *     out = (2 S + W H) / (2 W H)                       integer division, exact: round half up
 * where b is the byte the encoder sees at that source pixel today, as for the reduced pictures above: R, G, B of the
 * byte formats, the float formats through the engine's pixel transform, the gray value of the gray formats.  The weights
 * cover the source exactly, so no edge is replicated; an output sample reads at most ceil(W / w') + 1 columns of
 * ceil(H / h') + 1 rows.  w' = W and h' = H is the identity; W = s w' and H = s h' is the reduction by s above, byte
 * for byte.  THE CONTRACT: the JPEG of a resized frame is byte for byte what the same call makes of the uint8 picture so
 * defined handed over as SJPEG_HIP_SRC_RGB (the gray formats: SJPEG_HIP_SRC_GRAY, yuv_mode 4:0:0 only).  Formats, strides,
 * alignment and the elements read: as for the reduced pictures; the YUV-plane formats are not resized (SJPEG_HIP_EINVAL,
 * the message names the format).
 *
 * sjpeg_hip_fit_size (host only, integers): the size of a W x H picture fitted into a box bw x bh (each 1..65535),
 *   keeping its shape: (W, H) when W <= bw and H <= bh -- never larger --; else, when W * bh >= H * bw, w' = bw and
 *   h' = max(1, (H * bw + W / 2) / W); else h' = bh and w' = max(1, (W * bh + H / 2) / H).  SJPEG_HIP_EINVAL for
 *   dimensions or a box outside 1..65535.
 * sjpeg_hip_resize_ragged_bytes (host only): the bytes the resized pictures of a batch take, 0 on bad arguments
 *   (sizes: host int32[nframes][2] = (w', h'); NULL: every frame at its own size).  THE LAYOUT is that of the reduced
 *   pictures: rows padded to whole dwords, every picture at a multiple of 16, frame after frame.
 * sjpeg_hip_resize_ragged_src: ONE launch over the batch's tiles into d_resized (a multiple of 16, resized_bytes behind
 *   it), with the arguments, the ordering, the pipelined-mode behaviour and the outputs of sjpeg_hip_reduce_ragged_src.
 *   SJPEG_HIP_EINVAL before any device work, the frame named: a size below 1 or above the source's, a YUV-plane format,
 *   resized_bytes below sjpeg_hip_resize_ragged_bytes(), and every frame check of sjpeg_hip_encode_ragged_src.
 * sjpeg_hip_encode_ragged_resized_src / _resized_packed_src: the arguments and the output contract of
 *   sjpeg_hip_encode_ragged_full_meta_src / _full_meta_packed_src, plus `sizes`.  sizes == NULL or every size its
 *   frame's own: exactly that call on the caller's frames, any format; no copy, no kernel.  Otherwise every frame goes
 *   through the resize kernel into engine memory -- the memory of the reduced pictures: counted by
 *   sjpeg_hip_engine_scratch_bytes, released by sjpeg_hip_engine_trim, SJPEG_HIP_ENOMEM naming the bytes when it cannot
 *   be had -- and ONE inner call codes the batch, as for the reduced calls (SJPEG_YUV_AUTO decides on the RESIZED
 *   picture).  out_capacity is the caller's: sjpeg_hip_frame_bound(w', h', SJPEG_HIP_YUV444, 2048 + metadata) is always
 *   enough.  SJPEG_HIP_EINVAL before any device work: the checks above, gray with a yuv_mode other than 4:0:0, NULL
 *   arguments, and every check of the inner call. */
int sjpeg_hip_fit_size(int width, int height, int box_width, int box_height, int* fitted_width, int* fitted_height);
size_t sjpeg_hip_resize_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                     const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/);
int sjpeg_hip_resize_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                                const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                const int32_t (*sizes)[2] /*host int32[nframes][2]*/, void* d_resized, size_t resized_bytes,
                                sjpeg_hip_ragged_frame* resized_frames /*host out [nframes]*/, int* resized_format,
                                void* stream);
int sjpeg_hip_encode_ragged_resized_src(sjpeg_hip_engine* engine, int format, int nframes,
                                        const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                        const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                        const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                        void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                        int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_resized_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                               const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                               const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                               const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                               void* d_packed, size_t packed_capacity,
                                               uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                               int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                               void* stream);

/* ---- pictures turned upright inside the ragged call: EXIF orientation ----
 * A phone stores the sensor's rows as they come and records the rotation in EXIF tag 0x0112, Orientation, 1..8 (6: the
 * usual portrait photo); a thumbnail that ignores the tag lies on its side.  Let R be frame f's resized picture, w x h:
 * exactly what sjpeg_hip_resize_ragged_src defines above for sizes[f] = (w, h) -- `sizes` stay in the STORED orientation,
 * sizes == NULL: every frame at its own size.  For orientations[f] = o the upright picture U is w x h for o in 1..4 and
 * h x w for o in 5..8, and U(x, y) = R(sx, sy):
 *     o  meaning                                  sx         sy
 *     1  as stored                                x          y
 *     2  mirrored left-right                      w - 1 - x  y
 *     3  rotated 180                              w - 1 - x  h - 1 - y
 *     4  mirrored top-bottom                      x          h - 1 - y
 *     5  transposed                               y          x
 *     6  rotated 90 clockwise to show             y          h - 1 - x
 *     7  transverse                               w - 1 - y  h - 1 - x
 *     8  rotated 90 counter-clockwise to show     w - 1 - y  x
 * Exact area averaging commutes with the eight symmetries, so "resize, then turn" has one right answer; it costs the
 * stores of the small picture (the resize kernel stores every finished tile where it lands in U), not a pass over the
 * source.  THE CONTRACT: the JPEG of an oriented frame is byte for byte what the same call makes of the uint8 picture U
 * handed over as SJPEG_HIP_SRC_RGB (the gray formats: SJPEG_HIP_SRC_GRAY, 4:0:0 only); SJPEG_YUV_AUTO decides on U.
 * Formats, strides of either sign and the elements read: those of the resize.  The YUV-plane formats are not oriented:
 * an orientation other than 1 on one of them is SJPEG_HIP_EINVAL, the message names the format.
 *
 * sjpeg_hip_oriented_size (host only): (*ow, *oh) = the size of U for a stored width x height (1..65535 each) and an
 *   orientation 1..8; SJPEG_HIP_EINVAL otherwise.
 * sjpeg_hip_orient_ragged_bytes (host only): the bytes the upright pictures of a batch take, 0 on bad arguments (sizes
 *   and orientations: each may be NULL -- own sizes, all 1).  THE LAYOUT is that of the resized pictures with U's size:
 *   rows of align4(width of U * channels) bytes, every picture at a multiple of 16, frame after frame.  Row and picture
 *   padding may hold anything.  orientations == NULL: the value of sjpeg_hip_resize_ragged_bytes.
 * sjpeg_hip_orient_ragged_src: ONE launch, resize and orientation together, into d_out (a multiple of 16, `bytes` behind
 *   it) with the arguments, the ordering and the pipelined-mode behaviour of sjpeg_hip_resize_ragged_src; out_frames
 *   are U's (width, height, row stride), *out_format SJPEG_HIP_SRC_RGB or _GRAY.  SJPEG_HIP_EINVAL before any device
 *   work, the frame named: the resize's checks, and an orientation outside 1..8.
 * sjpeg_hip_encode_ragged_oriented_src / _oriented_packed_src: the resized entries plus `orientations` (host
 *   uint8[nframes], or NULL).  NULL or all 1: exactly the resized call on the same arguments -- so NV12 at its own sizes
 *   still passes through to the _full_meta_ call.  Otherwise the kernel runs into the engine memory of the reduced and
 *   resized pictures (counted by sjpeg_hip_engine_scratch_bytes, released by sjpeg_hip_engine_trim), then ONE inner call.
 *   out_capacity: sjpeg_hip_frame_bound of U's size, SJPEG_HIP_YUV444, 2048 + metadata is always enough.
 * sjpeg_hip_exif_orientation (host only): 1..8 from IFD0 tag 0x0112 of an EXIF payload as sjpeg_hip_metadata.exif takes
 *   it (the TIFF header first; a leading "Exif\0\0" is skipped), both byte orders; the tag must be one SHORT.  0 for
 *   anything else: no tag, a value outside 1..8, truncated or malformed bytes.  Never reads outside [exif, exif + size).
 * sjpeg_hip_exif_reset_orientation (host only): sets that value to 1 in place and returns the old value, or 0 with
 *   nothing changed -- for a service that bakes the rotation in and keeps the EXIF: a viewer would turn the picture a
 *   second time. */
int sjpeg_hip_oriented_size(int width, int height, int orientation, int* ow, int* oh);
size_t sjpeg_hip_orient_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                     const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                     const uint8_t* orientations /*host [nframes], or NULL*/);
int sjpeg_hip_orient_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                                const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                const uint8_t* orientations /*host [nframes], or NULL*/, void* d_out, size_t bytes,
                                sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/, int* out_format, void* stream);
int sjpeg_hip_encode_ragged_oriented_src(sjpeg_hip_engine* engine, int format, int nframes,
                                         const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                         const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                         const uint8_t* orientations /*host [nframes], or NULL*/,
                                         const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                         void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                         int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_oriented_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                                const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                const uint8_t* orientations /*host [nframes], or NULL*/,
                                                const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                                void* d_packed, size_t packed_capacity,
                                                uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                                int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                                void* stream);
int sjpeg_hip_exif_orientation(const uint8_t* exif, size_t size);
int sjpeg_hip_exif_reset_orientation(uint8_t* exif, size_t size);

/* ---- decoded video resized and turned inside the ragged call: NV12, NV21 and planar YUV ----
 * NV12 is what a GPU video decoder writes, so the pictures most likely to lie in device memory in front of this encoder
 * are decoded frames: poster frames, contact sheets, scrubbing previews.  The entries above make ONE interleaved plane
 * and refuse the four YUV-plane formats (SJPEG_HIP_SRC_YUV444, _YUV420, _NV12, _NV21); the ones below take exactly those
 * four and make THREE planes.  Frame f of W x H has a luma plane W x H and chroma planes CW x CH: CW = W, CH = H for
 * SJPEG_HIP_SRC_YUV444, else CW = (W + 1) / 2, CH = (H + 1) / 2, as the encoder reads them; U and V of NV12 / NV21 are
 * the even and odd bytes of plane 1 (NV21: V first).  sizes[f] = (w', h'), 1 <= w' <= W and 1 <= h' <= H, in the STORED
 * orientation; the resized chroma size is cw' = w', ch' = h' for 4:4:4, else cw' = (w' + 1) / 2, ch' = (h' + 1) / 2 --
 * never above the source's.
 *   Resize.  Every plane is resized as a gray picture of its own by the exact area average defined for
 *     sjpeg_hip_resize_ragged_src above: Y from W x H to w' x h', U and V from CW x CH to cw' x ch'.
 *   Orientation.  orientations[f] = o in 1..8 turns every plane as a picture of its own by the table above.  The upright
 *     picture is w' x h' for 1..4 and h' x w' for 5..8; its chroma planes are the turned cw' x ch' planes, whose size is
 *     the one the upright luma's implies.
 *   Odd sizes.  For even W, H, w', h' the chroma grid covers exactly the luma's extent before and after the resize and
 *     the turn.  For an odd one the last chroma sample stands for a half-covered pair, and a per-plane average or
 *     mirror then displaces chroma by less than one chroma sample -- at a picture's edge, which every decoder
 *     tolerates.  The bytes still have one right answer: the per-plane definition above.
 *   Output.  Always planar: SJPEG_HIP_SRC_YUV420 for SJPEG_HIP_SRC_YUV420, _NV12 and _NV21 (U and V de-interleaved,
 *     NV21's order put right), SJPEG_HIP_SRC_YUV444 for SJPEG_HIP_SRC_YUV444.  THE LAYOUT: for frame after frame Y,
 *     then U, then V; every plane at a multiple of 16 from the buffer's start, its rows align4(plane width) bytes
 *     apart -- the layout of the reduced pictures, per plane.  Padding may hold anything and lies inside the buffer.
 * THE CONTRACT: the JPEG of a frame is byte for byte what sjpeg_hip_encode_ragged_full_meta_src makes of the three
 * planes so defined handed over in the output format.  yuv_mode is the format's own, 4:2:0 or 4:4:4; anything else is
 * the inner call's "yuv_mode does not match the source format".  The samples are coded as they are, no colour
 * conversion: right for full-range BT.601 frames, which is what a JFIF file holds.  BT.709 and limited-range frames:
 * the _yuv_converted_ and _yuv_colour entries further down ("video colour converted inside the ragged call").
 *
 * sjpeg_hip_yuv_plane_size (host only): the size of plane 0..2 (Y, U, V) of a width x height picture (1..65535 each)
 *   in one of the four formats; SJPEG_HIP_EINVAL for any other format, the message names it.
 * sjpeg_hip_resize_ragged_yuv_bytes (host only): the bytes the made planes of a batch take, 0 on bad arguments (the
 *   last error says which); sizes and orientations: each may be NULL -- own sizes, all 1.
 * sjpeg_hip_resize_ragged_yuv_src: ONE launch over the tiles of every plane of every frame, resize and turn together,
 *   into d_out (a multiple of 16, `bytes` behind it), with the argument checks, the ordering and the pipelined-mode
 *   behaviour of sjpeg_hip_orient_ragged_src.  out_frames[f]: the three planes, their row strides and the upright width
 *   and height; *out_format as above.  The UV plane of NV12 / NV21 is read once.
 * sjpeg_hip_encode_ragged_yuv_resized_src / _yuv_resized_packed_src: the arguments and the output contract of
 *   sjpeg_hip_encode_ragged_oriented_src / _oriented_packed_src.  Every size its frame's own and every orientation 1
 *   (or both NULL): exactly the _full_meta_ call on the caller's frames, no kernel, no copy.  Otherwise the kernel
 *   writes into the engine memory of the reduced and resized pictures (counted by sjpeg_hip_engine_scratch_bytes,
 *   released by sjpeg_hip_engine_trim, SJPEG_HIP_ENOMEM naming the bytes when it cannot be had), then ONE inner call.
 *   out_capacity is the caller's: sjpeg_hip_frame_bound of the upright size with the format's mode, 2048 + metadata,
 *   is always enough.
 * SJPEG_HIP_EINVAL before any device work, the frame named as the ragged entries do: an RGB-like or gray format (the
 *   message names it and points at sjpeg_hip_orient_ragged_src), a size below 1 or above the source's, an orientation
 *   outside 1..8, `bytes` below sjpeg_hip_resize_ragged_yuv_bytes, a d_out that is not a multiple of 16, NULL
 *   arguments, and every frame check of sjpeg_hip_encode_ragged_src for the format. */
int sjpeg_hip_yuv_plane_size(int format, int width, int height, int plane, int* plane_width, int* plane_height);
size_t sjpeg_hip_resize_ragged_yuv_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                         const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                         const uint8_t* orientations /*host [nframes], or NULL*/);
int sjpeg_hip_resize_ragged_yuv_src(sjpeg_hip_engine* engine, int format, int nframes,
                                    const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                    const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                    const uint8_t* orientations /*host [nframes], or NULL*/, void* d_out, size_t bytes,
                                    sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/, int* out_format, void* stream);
int sjpeg_hip_encode_ragged_yuv_resized_src(sjpeg_hip_engine* engine, int format, int nframes,
                                            const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                            const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                            const uint8_t* orientations /*host [nframes], or NULL*/,
                                            const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                            void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                            int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_yuv_resized_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                   const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                                   const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                   const uint8_t* orientations /*host [nframes], or NULL*/,
                                                   const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                                   void* d_packed, size_t packed_capacity,
                                                   uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                                   int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                                   void* stream);

/* ---- contact sheets: a batch resized, turned and placed into grid pictures ----
 * A storyboard sprite sheet behind a video scrub bar, a contact sheet, a grid of a network's outputs: ONE JPEG of N
 * thumbnails in a grid, plus the rectangle of each.  The entries below make the thumbnails of the sections above and
 * store each straight into its rectangle of a sheet -- no thumbnail exists a second time.
 *   Sheet size.  SW = 2 * margin + cols * cell_width + (cols - 1) * gutter, SH the same down the rows; both 1..65535.
 *   Cells and sheets.  Frame f goes to sheet f / (cols * rows), there to cell k = f % (cols * rows): column
 *     i = k % cols, row j = k / cols, the cell's origin cx = margin + i * (cell_width + gutter), cy the same with j and
 *     cell_height.  nsheets = ceil(nframes / (cols * rows)), at most 65535; all sheets of a call have one size; the
 *     unused cells of the last sheet are background.
 *   The thumbnail of frame f is exactly the picture that exists already: for the RGB-like and gray formats that of
 *     sjpeg_hip_orient_ragged_src, for the four YUV-plane formats the three planes of sjpeg_hip_resize_ragged_yuv_src,
 *     made for sizes[f] (the STORED orientation) and orientations[f].  sizes == NULL: the frame is fitted into its
 *     cell, sizes[f] = sjpeg_hip_fit_size(W, H, box) with box = (cell_width, cell_height) for the orientations 1..4 and
 *     (cell_height, cell_width) for 5..8 -- never larger: a picture smaller than its cell stays as it is.
 *   Placement.  uw x uh, the thumbnail's UPRIGHT size, must not exceed the cell; x0 = cx + (cell_width - uw) / 2,
 *     y0 = cy + (cell_height - uh) / 2 (integer division: the spare sample is on the right and at the bottom).
 *   4:2:0 (SJPEG_HIP_SRC_YUV420, _NV12, _NV21).  margin, gutter, cell_width and cell_height must be even, and the
 *     centring offset is rounded down to even: x0 = cx + (((cell_width - uw) / 2) & ~1), y0 likewise.  The chroma planes
 *     of the thumbnail land at (x0 / 2, y0 / 2) in a chroma sheet of SW / 2 x SH / 2.  They always fit their half
 *     cell: with e = x0 - cx <= (cell_width - uw) / 2 and cell_width even, e / 2 + ceil(uw / 2) <=
 *     floor((cell_width - uw) / 2) + ceil(uw / 2) = cell_width / 2.  SJPEG_HIP_SRC_YUV444 has no evenness rule: all
 *     three planes land at (x0, y0).
 *   Bytes.  A sheet is `background` everywhere except in those rectangles, which hold the thumbnails' bytes.
 *     background is given in the bytes the encoder sees (R, G, B; the gray formats: [0]; the YUV-plane formats: Y, U, V)
 *     and does not pass through the engine's pixel transform.
 *   THE LAYOUT is that of the resized pictures, per sheet: one interleaved SJPEG_HIP_SRC_RGB / _GRAY plane, or the Y, U,
 *     V planes of SJPEG_HIP_SRC_YUV420 / _YUV444; rows align4 bytes apart, every plane at a multiple of 16, the sheets
 *     one after another.  Row padding holds background or anything, plane padding anything.
 * THE CONTRACT: the JPEG of a sheet is byte for byte what sjpeg_hip_encode_ragged_full_meta_src makes of the sheet so
 * defined, handed over in the output format.  SJPEG_YUV_AUTO decides on the sheet; the gray formats take 4:0:0 only,
 * the YUV-plane formats their own mode.
 *
 * sjpeg_hip_sheet_size (host only): checks the sheet for the format and gives its size.  SJPEG_HIP_EINVAL, the field
 *   named: a value out of range, reserved != 0, a sheet size above 65535, an odd value with a 4:2:0 format.
 * sjpeg_hip_sheet_places (host only; reads no device memory): places[f] = (sheet, x0, y0, uw, uh) -- the #xywh=
 *   numbers of a storyboard.
 * sjpeg_hip_sheet_ragged_bytes (host only): the bytes the sheets of a call take, 0 on bad arguments (the last error
 *   says which).
 * sjpeg_hip_sheet_ragged_src: the uint8 sheets into d_out (a multiple of 16, `bytes` behind it): a background fill in
 *   whole dwords, then ONE launch of the resize kernel over every thumbnail's tiles, both on `stream` -- stream order is
 *   the only ordering relied on.  sheet_frames[s]: sheet s as a frame of *out_format (planes, row strides, SW x SH).
 *   Ordering and pipelined-mode behaviour: those of sjpeg_hip_orient_ragged_src.
 * sjpeg_hip_encode_ragged_sheet_src / _sheet_packed_src: the arguments of the _oriented_ / _yuv_resized_ entries plus
 *   `sheet`; ONE set of entries serves both families of formats.  The frames' out_offset and out_capacity are ignored:
 *   sheet s is written at d_out + s * out_stride with capacity out_stride (sjpeg_hip_frame_bound of SW x SH is always
 *   enough); the packed entry has the packed contract of sjpeg_hip_encode_ragged_packed_src over nsheets pictures.
 *   Both fill d_sizes[nsheets].  params, meta, modes, q_out and value_out count SHEETS where the other entries count
 *   frames: quant_per_frame and search_per_frame mean per sheet, meta is [nsheets], [1] or NULL.  The sheets go into
 *   the engine memory of the reduced and resized pictures (counted by sjpeg_hip_engine_scratch_bytes, released by
 *   sjpeg_hip_engine_trim, SJPEG_HIP_ENOMEM naming the bytes); ONE inner call then codes all sheets.
 * SJPEG_HIP_EINVAL before any device work: the sheet checks above; every check of the orient / yuv-resize plans, the
 *   frame named; a thumbnail larger than its cell (the frame, both sizes and the orientation named); `bytes` below
 *   sjpeg_hip_sheet_ragged_bytes; a d_out that is not a multiple of 16; NULL arguments; out_stride below 1; every check
 *   of the inner call. */
typedef struct sjpeg_hip_sheet {
  int32_t cols, rows;               /* cells a sheet: each >= 1 */
  int32_t cell_width, cell_height;  /* each 1..65535 */
  int32_t gutter, margin;           /* between cells / around them: each 0..65535 */
  uint8_t background[3];            /* R, G, B; gray formats: [0]; YUV-plane formats: Y, U, V */
  uint8_t reserved;                 /* 0 */
} sjpeg_hip_sheet;
int sjpeg_hip_sheet_size(const sjpeg_hip_sheet* sheet, int format, int* width, int* height);
int sjpeg_hip_sheet_places(int format, int nframes, const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                           const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                           const uint8_t* orientations /*host [nframes], or NULL*/, int32_t (*places)[5] /*host out [nframes]*/);
size_t sjpeg_hip_sheet_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                    const sjpeg_hip_sheet* sheet, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                    const uint8_t* orientations /*host [nframes], or NULL*/);
int sjpeg_hip_sheet_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                               const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_sheet* sheet,
                               const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                               const uint8_t* orientations /*host [nframes], or NULL*/, void* d_out, size_t bytes,
                               sjpeg_hip_ragged_frame* sheet_frames /*host out [nsheets]*/, int* nsheets, int* out_format,
                               void* stream);
int sjpeg_hip_encode_ragged_sheet_src(sjpeg_hip_engine* engine, int format, int nframes,
                                      const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset, out_capacity ignored*/,
                                      const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                      const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                      const uint8_t* orientations /*host [nframes], or NULL*/,
                                      const struct sjpeg_hip_metadata* meta /*host: [nsheets], [1] or NULL*/, int meta_per_frame,
                                      void* d_out, size_t out_stride, uint64_t* d_sizes /*[nsheets]*/,
                                      int* modes, float* q_out, float* value_out /*host [nsheets], each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_sheet_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                             const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset, out_capacity ignored*/,
                                             const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                             const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                             const uint8_t* orientations /*host [nframes], or NULL*/,
                                             const struct sjpeg_hip_metadata* meta /*host: [nsheets], [1] or NULL*/, int meta_per_frame,
                                             void* d_packed, size_t packed_capacity,
                                             uint64_t* d_offsets /*[nsheets + 1]*/, uint64_t* d_sizes /*[nsheets]*/,
                                             int* modes, float* q_out, float* value_out /*host [nsheets], each may be NULL*/,
                                             void* stream);

/* ---- alpha flattened inside the ragged call: RGBA pictures over a background ----
 * PNG and WebP uploads, logos, product cut-outs, a renderer's [H, W, 4] RGBA16F, a matting network's colour plus
 * matte: pictures with an alpha channel, which JPEG has not.  The entries above drop the fourth sample and code
 * whatever colour lies under transparent pixels.  The entries below lay every pixel over a background first -- in the
 * resize kernel's loader, so no flattened copy of the source exists -- and then do what the oriented and sheet entries
 * do.
 *   Alpha formats: SJPEG_HIP_SRC_BGRA, _RGBA, _RGBA_F32, _RGBA_F16, _RGBA_BF16; the fourth byte or element of a pixel
 *     is its alpha.
 *   For a pixel of such a frame, s_c is the byte the encoder sees there today in channel c (the float formats: through
 *     the engine's pixel transform of channel c) and a its alpha byte: the stored byte, or for the float formats
 *     rint(clamp(fmaf(x, alpha_scale, alpha_bias), 0, 255)), NaN -> 0 -- the element rule of the float formats with
 *     the flatten's own scale and bias (255, 0 for alpha in 0..1).  alpha_scale and alpha_bias are ignored for the
 *     byte formats; for the float formats they must be finite.
 *   Straight alpha (premultiplied = 0):  b_c = (a * s_c + (255 - a) * bg_c + 127) / 255, integer division: round to
 *     nearest, and 255 is odd, so there are no ties; a = 255 gives s_c and a = 0 gives bg_c exactly.
 *   Premultiplied alpha (premultiplied = 1):  b_c = min(255, s_c + ((255 - a) * bg_c + 127) / 255).
 *   background is given in the bytes the encoder sees (R, G, B) and does not pass through the pixel transform.
 * THE CONTRACT: the flattened picture F of a frame is the uint8 RGB picture of the b_c, W x H.  A flattened call makes,
 * byte for byte, what the corresponding call above makes of F handed over as SJPEG_HIP_SRC_RGB: same sizes, same
 * orientations, same sheet, same params.  Flatten comes first; the exact area average, the turn and the placement
 * follow on bytes as they are defined above -- "composite the picture, then thumbnail it", two roundings on purpose.
 * Elements read: under flatten the fourth element of every pixel IS read, so a row of the float RGBA formats must hold
 * it: |row_stride| >= width * 4 * element size.  The x[..., 1:4]-of-ARGB view that the unflattened float RGBA formats
 * allow (its last pixel's fourth element lies outside the tensor) is therefore not a legal flattened source.  Nothing
 * else about strides and alignment changes: either sign, element-only alignment.
 *
 * sjpeg_hip_flatten_ragged_src: sjpeg_hip_orient_ragged_src plus `flatten` (not NULL): its arguments, ordering,
 *   pipelined-mode behaviour, output layout and size (sjpeg_hip_orient_ragged_bytes), ONE launch.  sizes == NULL and
 *   orientations == NULL is the flatten alone: F itself.  *out_format is always SJPEG_HIP_SRC_RGB.
 * sjpeg_hip_encode_ragged_flattened_src / _flattened_packed_src: the _oriented_ / _oriented_packed_ entries plus
 *   `flatten`.  flatten == NULL: exactly the oriented call on the same arguments, any format.  Otherwise EVERY frame
 *   goes through the kernel, also at its own size with orientation 1 -- there is no pass-through: the inner call never
 *   sees the alpha format -- into the engine memory of the reduced and resized pictures (counted by
 *   sjpeg_hip_engine_scratch_bytes, released by sjpeg_hip_engine_trim, SJPEG_HIP_ENOMEM naming the bytes), then ONE
 *   inner _full_meta_ call as SJPEG_HIP_SRC_RGB: SJPEG_YUV_AUTO, the search and the metadata act on the flattened,
 *   resized, upright picture.
 * sjpeg_hip_sheet_ragged_flat_src (flatten not NULL), sjpeg_hip_encode_ragged_sheet_flat_src / _sheet_flat_packed_src
 *   (flatten == NULL: exactly the sheet call): the three sheet entries plus `flatten`.  The flatten's background and
 *   the sheet's are independent fields.  sjpeg_hip_sheet_places and sjpeg_hip_sheet_ragged_bytes serve as they are: a
 *   flattened sheet has the places and the bytes of the same call on SJPEG_HIP_SRC_RGB frames.
 * SJPEG_HIP_EINVAL before any device work, the frame named as the ragged entries name it: a flatten with a format that
 *   has no alpha (the message names the format: the YUV-plane, gray, RGB and planar formats all fall here);
 *   premultiplied above 1; a float format's alpha_scale or alpha_bias that is not finite; a float row too short for its
 *   alpha (the message says "alpha"); and every check the corresponding unflattened entry makes. */
typedef struct sjpeg_hip_flatten {
  uint8_t background[3];          /* R, G, B in the bytes the encoder sees; not passed through the pixel transform */
  uint8_t premultiplied;          /* 0: straight alpha; 1: the colour samples are already multiplied by alpha; else EINVAL */
  float alpha_scale, alpha_bias;  /* float formats: the alpha sample's transform; 255, 0 for alpha in 0..1 */
} sjpeg_hip_flatten;
int sjpeg_hip_flatten_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                                 const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_flatten* flatten,
                                 const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                 const uint8_t* orientations /*host [nframes], or NULL*/, void* d_out, size_t bytes,
                                 sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/, int* out_format, void* stream);
int sjpeg_hip_encode_ragged_flattened_src(sjpeg_hip_engine* engine, int format, int nframes,
                                          const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                          const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                          const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                          const uint8_t* orientations /*host [nframes], or NULL*/,
                                          const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                          void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                          int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_flattened_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                 const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                                 const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                                 const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                 const uint8_t* orientations /*host [nframes], or NULL*/,
                                                 const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                                 void* d_packed, size_t packed_capacity,
                                                 uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                                 int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                                 void* stream);
int sjpeg_hip_sheet_ragged_flat_src(sjpeg_hip_engine* engine, int format, int nframes,
                                    const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_sheet* sheet,
                                    const sjpeg_hip_flatten* flatten, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                    const uint8_t* orientations /*host [nframes], or NULL*/, void* d_out, size_t bytes,
                                    sjpeg_hip_ragged_frame* sheet_frames /*host out [nsheets]*/, int* nsheets, int* out_format,
                                    void* stream);
int sjpeg_hip_encode_ragged_sheet_flat_src(sjpeg_hip_engine* engine, int format, int nframes,
                                           const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset, out_capacity ignored*/,
                                           const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                           const sjpeg_hip_flatten* flatten /*or NULL*/,
                                           const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                           const uint8_t* orientations /*host [nframes], or NULL*/,
                                           const struct sjpeg_hip_metadata* meta /*host: [nsheets], [1] or NULL*/, int meta_per_frame,
                                           void* d_out, size_t out_stride, uint64_t* d_sizes /*[nsheets]*/,
                                           int* modes, float* q_out, float* value_out /*host [nsheets], each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_sheet_flat_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                  const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset, out_capacity ignored*/,
                                                  const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                  const sjpeg_hip_flatten* flatten /*or NULL*/,
                                                  const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                  const uint8_t* orientations /*host [nframes], or NULL*/,
                                                  const struct sjpeg_hip_metadata* meta /*host: [nsheets], [1] or NULL*/, int meta_per_frame,
                                                  void* d_packed, size_t packed_capacity,
                                                  uint64_t* d_offsets /*[nsheets + 1]*/, uint64_t* d_sizes /*[nsheets]*/,
                                                  int* modes, float* q_out, float* value_out /*host [nsheets], each may be NULL*/,
                                                  void* stream);

/* ---- video colour converted inside the ragged call: BT.709 and studio range ----
 * A JFIF file is full-range BT.601 YCbCr.  Decoded video mostly is not: HD content is BT.709, and nearly all video is
 * studio range (Y 16..235, chroma 16..240).  The YUV entries above code the samples as they are -- right for full-range
 * BT.601 frames only; a thumbnail of anything else is displayed washed out, its saturated colours shifted in hue.  The
 * entries below convert the MADE planes -- the thumbnails, not the sources -- to JFIF's colour: ONE more launch behind
 * the resize launch on the call's stream, in place.  The source is described per call or per frame by its matrix
 * (SJPEG_HIP_MATRIX_BT601 / _BT709) and its range (SJPEG_HIP_RANGE_FULL / _LIMITED).
 * THE CONTRACT, exact and in integers.  P is what sjpeg_hip_resize_ragged_yuv_src makes of a frame: upright planar Y
 * (uw x uh), U and V (cw x ch).  The converted picture P' is defined from P alone; floor is a true floor, clamp8 clamps
 * to 0..255, u = U[j][i] - 128, v = V[j][i] - 128:
 *   chroma sample (i, j):  U' = clamp8(128 + floor((k11 * u + k12 * v + 8192) / 16384))
 *                          V' = clamp8(128 + floor((k21 * u + k22 * v + 8192) / 16384))
 *   luma sample (x, y):    Y' = clamp8(floor((k00 * (Y - y0) + k01 * u + k02 * v + 8192) / 16384)), u and v the
 *     UNCONVERTED chroma at (x / s, y / s), s = 2 for the 4:2:0 formats and 1 for SJPEG_HIP_SRC_YUV444: the nearest
 *     chroma sample, the one whose block the luma sample lies in (cw = (uw + 1) / 2: always inside the plane, after a
 *     transposing orientation too).  Every sum fits 32 bits.
 *   The tables, Q14: rows Y, U, V of the output, columns Y, U, V of the source; the chroma rows never read luma.
 *     BT.601 full:     y0 0,  the identity: no pass, the bytes of P
 *     BT.601 limited:  y0 16, {19077, 0, 0}, {0, 18651, 0}, {0, 0, 18651}
 *     BT.709 limited:  y0 16, {19077, 1895, 3657}, {0, 18462, -2064}, {0, -1351, 18342}
 *     BT.709 full:     y0 0,  {16384, 1664, 3213}, {0, 16218, -1813}, {0, -1187, 16112}
 *   They are rint(M * 16384), M = source Y'CbCr -> R'G'B' with the source's Kr, Kb (BT.601: 0.299, 0.114; BT.709:
 *   0.2126, 0.0722), then R'G'B' -> full-range BT.601 YCbCr, the columns scaled by 255/219 (Y) and 255/224 (chroma) for
 *   a limited-range source.  Against the exactly rounded real result the integer formula is off by at most 1.
 * The JPEG of a frame is byte for byte what sjpeg_hip_encode_ragged_full_meta_src makes of P' handed over as
 * SJPEG_HIP_SRC_YUV420 (SJPEG_HIP_SRC_YUV444 for a 4:4:4 source).  In a sheet only the thumbnails' rectangles are
 * converted: `background` stays as given, (Y, U, V) in the output's colour.
 *
 * colour, colour_per_frame: used as meta / meta_per_frame are -- [1] for all frames, or [nframes].  colour == NULL, or
 *   BT.601 full range for every frame: the entry IS its counterpart above -- the same bytes, no extra device work, its
 *   messages.  Otherwise every size and orientation goes through the resize kernel, ratio 1 included (the caller's
 *   planes are never written), then the colour launch over the frames that need it, then ONE inner call.
 * sjpeg_hip_yuv_colour_samples (host only): the formula as code, for bindings and tests: yuv_out[k] = P' of the one-
 *   sample picture yuv_in[k] = (Y, U, V); yuv_out may be yuv_in.
 * sjpeg_hip_convert_ragged_yuv_src: the arguments of sjpeg_hip_resize_ragged_yuv_src plus the colour; P' in the same
 *   layout, sized by sjpeg_hip_resize_ragged_yuv_bytes.
 * sjpeg_hip_encode_ragged_yuv_converted_src / _yuv_converted_packed_src: the _yuv_resized_ entries plus the colour.
 * sjpeg_hip_sheet_ragged_yuv_colour_src, sjpeg_hip_encode_ragged_sheet_yuv_colour_src / _sheet_yuv_colour_packed_src:
 *   the three sheet entries, for the four YUV-plane formats, plus the colour; places and bytes: sjpeg_hip_sheet_places
 *   and sjpeg_hip_sheet_ragged_bytes as they are.
 * SJPEG_HIP_EINVAL before any device work, the frame named as the ragged entries name it: a matrix or a range above 1,
 *   a reserved byte that is not 0, an RGB-like or gray format (the message names it), samples == NULL, and every check
 *   the counterpart entry makes. */
enum { SJPEG_HIP_MATRIX_BT601 = 0, SJPEG_HIP_MATRIX_BT709 = 1 };
enum { SJPEG_HIP_RANGE_FULL = 0, SJPEG_HIP_RANGE_LIMITED = 1 };
typedef struct sjpeg_hip_yuv_colour {
  uint8_t matrix;                 /* SJPEG_HIP_MATRIX_* of the SOURCE */
  uint8_t range;                  /* SJPEG_HIP_RANGE_* of the SOURCE */
  uint8_t reserved[2];            /* 0 */
} sjpeg_hip_yuv_colour;           /* 4 bytes */
int sjpeg_hip_yuv_colour_samples(const sjpeg_hip_yuv_colour* colour, size_t n, const uint8_t (*yuv_in)[3] /*[n]*/,
                                 uint8_t (*yuv_out)[3] /*[n]*/);
int sjpeg_hip_convert_ragged_yuv_src(sjpeg_hip_engine* engine, int format, int nframes,
                                     const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                     const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                     const uint8_t* orientations /*host [nframes], or NULL*/,
                                     const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                     void* d_out, size_t bytes, sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/,
                                     int* out_format, void* stream);
int sjpeg_hip_encode_ragged_yuv_converted_src(sjpeg_hip_engine* engine, int format, int nframes,
                                              const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                              const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                              const uint8_t* orientations /*host [nframes], or NULL*/,
                                              const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                              const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                              void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                              int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_yuv_converted_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                     const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                                     const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                     const uint8_t* orientations /*host [nframes], or NULL*/,
                                                     const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                                     const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                                     void* d_packed, size_t packed_capacity,
                                                     uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                                     int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                                     void* stream);
int sjpeg_hip_sheet_ragged_yuv_colour_src(sjpeg_hip_engine* engine, int format, int nframes,
                                          const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_sheet* sheet,
                                          const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                          const uint8_t* orientations /*host [nframes], or NULL*/,
                                          const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                          void* d_out, size_t bytes, sjpeg_hip_ragged_frame* sheet_frames /*host out [nsheets]*/,
                                          int* nsheets, int* out_format, void* stream);
int sjpeg_hip_encode_ragged_sheet_yuv_colour_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                 const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset, out_capacity ignored*/,
                                                 const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                 const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                 const uint8_t* orientations /*host [nframes], or NULL*/,
                                                 const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                                 const struct sjpeg_hip_metadata* meta /*host: [nsheets], [1] or NULL*/, int meta_per_frame,
                                                 void* d_out, size_t out_stride, uint64_t* d_sizes /*[nsheets]*/,
                                                 int* modes, float* q_out, float* value_out /*host [nsheets], each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_sheet_yuv_colour_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                        const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset, out_capacity ignored*/,
                                                        const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                        const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                        const uint8_t* orientations /*host [nframes], or NULL*/,
                                                        const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                                        const struct sjpeg_hip_metadata* meta /*host: [nsheets], [1] or NULL*/, int meta_per_frame,
                                                        void* d_packed, size_t packed_capacity,
                                                        uint64_t* d_offsets /*[nsheets + 1]*/, uint64_t* d_sizes /*[nsheets]*/,
                                                        int* modes, float* q_out, float* value_out /*host [nsheets], each may be NULL*/,
                                                        void* stream);

/* ---- 10-bit video: P010 and 16-bit YUV planes in the ragged call ----
 * GPU decoders write HEVC Main10, AV1 10-bit and VP9 profile 2 as P010 -- NV12's plane layout with little-endian 16-bit
 * words, the sample in the high bits --, software decoders yuv420p10le / yuv420p12le -- planar, the sample in the low
 * bits.  The entries below take such frames as the decoder wrote them: the resize kernel stages the 16-bit words, sums
 * them exactly and rounds ONCE into the made 8-bit planes; there is no narrowing pass over the full-size planes.
 * A DEEP source is one of the four YUV-plane formats (SJPEG_HIP_SRC_NV12, _NV21, _YUV420, _YUV444: the format says
 * where the samples lie, in samples) whose every sample is a little-endian 16-bit word x.  The depth is a second axis
 * beside the format, one per call: bytes = 2, and shift = how many low bits of a word lie below the byte.
 *   P010, P012, P016:  SJPEG_HIP_SRC_NV12,   shift 8        yuv420p10le:  SJPEG_HIP_SRC_YUV420, shift 2
 *   yuv444p10le:       SJPEG_HIP_SRC_YUV444, shift 2        yuv420p12le:  SJPEG_HIP_SRC_YUV420, shift 4
 * THE CONTRACT, exact and in integers.  A sample of a made plane comes from its cell's weighted sum S of source WORDS,
 * the cells and weights those of the resize above on the W w' x H h' grid; the weights sum to A = W H.  With s = shift:
 *   byte = min(255, floor((2 S + A 2^s) / (A 2^(s+1))))
 * -- the exact area average of the words, divided by 2^s, rounded half up once, then clamped.  The clamp is needed: a
 * full-scale P010 picture gives 256 before it.  At the frame's own size this is min(255, (x + 2^(s-1)) >> s); for s = 0
 * it is min(255, x).  Bits above the nominal depth of a low-aligned source are no error: they take part as they are
 * and the clamp bounds the result.  Bounds: a row's horizontal sum is at most 65535 * 65535 < 2^32, a cell's sum is
 * below 2^48, the numerator below 2^50.
 * Everything behind that is the contracts above applied to the made 8-bit planes: the orientation, the placed store
 * into sheets, the Q14 colour conversion (a 10-bit limited-range sample 64..940 lands on 16..235, so BT.709 / limited
 * works as it does for bytes).  There is no BT.2020 matrix and no PQ / HLG tone mapping: HDR frames are coded by their
 * code values.  The JPEG of a frame is byte for byte what the _yuv_converted_ entry makes of the made planes' bytes.
 *
 * depth: host, one per call.  colour, colour_per_frame: as above; colour == NULL: none.  There is NO pass-through: the
 *   inner flow cannot read words, so every frame goes through the kernel, at its own size and orientation 1 too.
 * sjpeg_hip_yuv16_samples (host only): the own-size formula as code: out[k] = min(255, (in[k] + 2^(s-1)) >> s).
 * sjpeg_hip_convert_ragged_yuv16_src: sjpeg_hip_convert_ragged_yuv_src plus the depth; the made planes are bytes, in
 *   the same layout, so sjpeg_hip_resize_ragged_yuv_bytes sizes the buffer for this entry too.
 * sjpeg_hip_encode_ragged_yuv16_src / _yuv16_packed_src: the _yuv_converted_ entries plus the depth.
 * sjpeg_hip_sheet_ragged_yuv16_src, sjpeg_hip_encode_ragged_sheet_yuv16_src / _sheet_yuv16_packed_src: the three
 *   _yuv_colour sheet entries plus the depth; places and bytes by sjpeg_hip_sheet_places / sjpeg_hip_sheet_ragged_bytes.
 * A frame's planes: row_stride in BYTES as ever, |row_stride| at least twice the 8-bit row; every plane pointer and
 *   row stride a multiple of 2.
 * SJPEG_HIP_EINVAL before any device work: depth == NULL, bytes other than 2, a shift above 8, a reserved byte that is
 *   not 0 (the field is named); an RGB-like or gray format (named); a NULL plane, a short row, a plane or row stride
 *   that is not a multiple of the element size (2 bytes) -- frame and plane named; and every check the counterpart
 *   entry makes. */
typedef struct sjpeg_hip_yuv_depth {
  uint8_t bytes;                  /* 2 (the only value taken; 1 and others are refused by name) */
  uint8_t shift;                  /* 0..8: how many low bits of a word lie below the byte */
  uint8_t reserved[2];            /* 0 */
} sjpeg_hip_yuv_depth;            /* 4 bytes */
int sjpeg_hip_yuv16_samples(const sjpeg_hip_yuv_depth* depth, size_t n, const uint16_t* in /*[n]*/, uint8_t* out /*[n]*/);
int sjpeg_hip_convert_ragged_yuv16_src(sjpeg_hip_engine* engine, int format, int nframes,
                                       const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                       const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                       const uint8_t* orientations /*host [nframes], or NULL*/,
                                       const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                       const sjpeg_hip_yuv_depth* depth,
                                       void* d_out, size_t bytes, sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/,
                                       int* out_format, void* stream);
int sjpeg_hip_encode_ragged_yuv16_src(sjpeg_hip_engine* engine, int format, int nframes,
                                      const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                      const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                      const uint8_t* orientations /*host [nframes], or NULL*/,
                                      const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                      const sjpeg_hip_yuv_depth* depth,
                                      const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                      void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                      int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_yuv16_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                             const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                             const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                             const uint8_t* orientations /*host [nframes], or NULL*/,
                                             const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                             const sjpeg_hip_yuv_depth* depth,
                                             const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                             void* d_packed, size_t packed_capacity,
                                             uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                             int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                             void* stream);
int sjpeg_hip_sheet_ragged_yuv16_src(sjpeg_hip_engine* engine, int format, int nframes,
                                     const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_sheet* sheet,
                                     const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                     const uint8_t* orientations /*host [nframes], or NULL*/,
                                     const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                     const sjpeg_hip_yuv_depth* depth,
                                     void* d_out, size_t bytes, sjpeg_hip_ragged_frame* sheet_frames /*host out [nsheets]*/,
                                     int* nsheets, int* out_format, void* stream);
int sjpeg_hip_encode_ragged_sheet_yuv16_src(sjpeg_hip_engine* engine, int format, int nframes,
                                            const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset, out_capacity ignored*/,
                                            const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                            const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                            const uint8_t* orientations /*host [nframes], or NULL*/,
                                            const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                            const sjpeg_hip_yuv_depth* depth,
                                            const struct sjpeg_hip_metadata* meta /*host: [nsheets], [1] or NULL*/, int meta_per_frame,
                                            void* d_out, size_t out_stride, uint64_t* d_sizes /*[nsheets]*/,
                                            int* modes, float* q_out, float* value_out /*host [nsheets], each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_sheet_yuv16_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                   const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset, out_capacity ignored*/,
                                                   const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                   const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                   const uint8_t* orientations /*host [nframes], or NULL*/,
                                                   const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                                   const sjpeg_hip_yuv_depth* depth,
                                                   const struct sjpeg_hip_metadata* meta /*host: [nsheets], [1] or NULL*/, int meta_per_frame,
                                                   void* d_packed, size_t packed_capacity,
                                                   uint64_t* d_offsets /*[nsheets + 1]*/, uint64_t* d_sizes /*[nsheets]*/,
                                                   int* modes, float* q_out, float* value_out /*host [nsheets], each may be NULL*/,
                                                   void* stream);

/* ---- resize in linear light: gamma-correct thumbnails in the ragged call ----
 * A downscaler that averages gamma-encoded values darkens fine detail: a 0/255 checkerboard reduced 2:1 comes out as
 * 128, and the light it emitted corresponds to byte 188.  Every entry above averages the stored bytes -- exact, but in
 * coded light.  The entries below average the LIGHT the bytes stand for, as libvips' `thumbnail --linear` and
 * ImageMagick's `-colorspace RGB -resize` do, still in ONE launch and still with one right answer in integers.
 * `light` is an int:
 *   SJPEG_HIP_LIGHT_CODED (0): average the bytes as they are.  This is every entry above.
 *   SJPEG_HIP_LIGHT_LINEAR_SRGB (1): the definition below.
 *   Anything else is SJPEG_HIP_EINVAL.
 * THE TABLE.  L[b], for b = 0..255, is floor(65535 * f(b / 255) + 1/2).  f is the sRGB decoding function of
 * IEC 61966-2-1:
 *   f(c) = c / 12.92 for c <= 0.04045
 *   f(c) = ((c + 0.055) / 1.055) ^ 2.4 otherwise
 * The table is 256 literal uint16_t constants (sjpeg_amd/csrc/light_math.h) that host and kernel share; there is no
 * pow at run time, on either side.  Check values: L[0..5] = 0, 20, 40, 60, 80, 99; L[252..255] = 63795, 64372, 64952,
 * 65535; strictly increasing, smallest step 19; sum 5217863; SHA-256 of the 256 values as little-endian uint16
 * fdb7af3c01815a2118db8e50aac3c2304205ccc3f381f8976c588642c1aa60b6.  No entry lies closer than 0.0016 to a rounding
 * tie, so a double-precision evaluation gives the same table.
 * THE AVERAGE.  The resize's own wx, wy, W, H, w', h', unchanged.  b(x, y, c) is the byte the resize sees there
 * today; for a flattened call that is the flattened byte.
 *   A = W * H
 *   S = sum over y of wy(y', y) * sum over x of wx(x', x) * L[b(x, y, c)]
 *     (a row's inner sum is at most 65535 W < 2^32 and S <= 65535 A < 2^48: the bounds of the 16-bit video path)
 *   out = the number of k in 1..255 with 2 S >= (L[k-1] + L[k]) * A
 * So out is the byte whose linear value is nearest the exact average; a tie goes to the larger byte.  The compare is
 * on exact 64-bit products: (L[k-1] + L[k]) < 2^17 and A < 2^32, so both sides stay below 2^49.  Consequences:
 *   A picture at its own size is itself (S = L[b] A).
 *   A constant picture is itself at any size.
 *   out is monotone in S.
 *   The eight orientations still commute with the average.
 *   A linear resize by a whole number is NOT the Reduced picture (sjpeg_hip_reduce_ragged_src): that averages bytes.
 * Known answers (the byte average in brackets): 0 and 255 in equal parts 188 [128]; 0 and 255 at 3:1 137 [64]; 100
 * and 200 in equal parts 160 [150].
 * ORDER OF STEPS: 1. the pixel transform of the float formats; 2. flatten, on bytes in coded light exactly as above
 * (browsers and PNG viewers composite this way; a flattened linear call makes what the linear call makes of the
 * flattened picture F); 3. L[]; 4. the average; 5. the inverse; 6. the turn; 7. the placement.  A sheet's background
 * and gutters are bytes, as given, and are never converted.
 * FORMATS: every format the resize takes goes through the same curve -- RGB, BGRA, RGBA, planar RGB, the float kinds
 * in both layouts, gray.  The YUV-plane formats are refused with SJPEG_HIP_EINVAL, naming the format: their samples
 * are not RGB light.
 * JPEG CONTRACT, the family's usual one: the JPEG is byte for byte what the same call makes of the uint8 picture so
 * defined, handed over as SJPEG_HIP_SRC_RGB (the gray formats: SJPEG_HIP_SRC_GRAY, 4:0:0 only).  SJPEG_YUV_AUTO, the
 * search and the metadata act on the made picture.
 *
 * sjpeg_hip_linear_ragged_src: sjpeg_hip_flatten_ragged_src's arguments, with `flatten` allowed to be NULL, plus
 *   `light` behind it.  Same output layout, same size (sjpeg_hip_orient_ragged_bytes), ONE launch.
 * sjpeg_hip_encode_ragged_linear_src / _linear_packed_src: the _flattened_ entries plus `light`.
 * sjpeg_hip_sheet_ragged_linear_src, sjpeg_hip_encode_ragged_sheet_linear_src / _sheet_linear_packed_src: the
 *   _sheet_flat_ entries plus `light` (flatten may be NULL).
 * light == SJPEG_HIP_LIGHT_CODED is a pass-through: exactly the flattened, oriented or sheet call on the same
 *   arguments, with that entry's name in the messages.  With SJPEG_HIP_LIGHT_LINEAR_SRGB EVERY frame goes through the
 *   kernel, also at its own size with orientation 1; that case is a copy, because the inverse is exact.
 * SJPEG_HIP_EINVAL before any device work: a light that is neither value; a YUV-plane format (named); gray with a
 *   yuv_mode other than 4:0:0; and every check the corresponding coded-light entry makes.
 * Host only, for bindings and tests:
 *   sjpeg_hip_light_table: the 256 table values of `light` (SJPEG_HIP_LIGHT_CODED: the bytes themselves, L[b] = b).
 *   sjpeg_hip_light_round: *byte = out for a cell sum S of a W x H picture (SJPEG_HIP_LIGHT_CODED: the byte average
 *     rounded half up, as the entries above round); S above L[255] W H, W or H outside 1..65535 or a NULL pointer is
 *     SJPEG_HIP_EINVAL. */
#define SJPEG_HIP_LIGHT_CODED 0
#define SJPEG_HIP_LIGHT_LINEAR_SRGB 1
int sjpeg_hip_light_table(int light, uint16_t table[256]);
int sjpeg_hip_light_round(int light, uint64_t S, uint32_t W, uint32_t H, uint32_t* byte);
int sjpeg_hip_linear_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                                const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                int light, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                const uint8_t* orientations /*host [nframes], or NULL*/, void* d_out, size_t bytes,
                                sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/, int* out_format, void* stream);
int sjpeg_hip_encode_ragged_linear_src(sjpeg_hip_engine* engine, int format, int nframes,
                                       const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                       const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/, int light,
                                       const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                       const uint8_t* orientations /*host [nframes], or NULL*/,
                                       const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                       void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                       int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_linear_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                              const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                              const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                              int light, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                              const uint8_t* orientations /*host [nframes], or NULL*/,
                                              const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                              void* d_packed, size_t packed_capacity,
                                              uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                              int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                              void* stream);
int sjpeg_hip_sheet_ragged_linear_src(sjpeg_hip_engine* engine, int format, int nframes,
                                      const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_sheet* sheet,
                                      const sjpeg_hip_flatten* flatten /*or NULL*/, int light,
                                      const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                      const uint8_t* orientations /*host [nframes], or NULL*/, void* d_out, size_t bytes,
                                      sjpeg_hip_ragged_frame* sheet_frames /*host out [nsheets]*/, int* nsheets, int* out_format,
                                      void* stream);
int sjpeg_hip_encode_ragged_sheet_linear_src(sjpeg_hip_engine* engine, int format, int nframes,
                                             const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset, out_capacity ignored*/,
                                             const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                             const sjpeg_hip_flatten* flatten /*or NULL*/, int light,
                                             const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                             const uint8_t* orientations /*host [nframes], or NULL*/,
                                             const struct sjpeg_hip_metadata* meta /*host: [nsheets], [1] or NULL*/, int meta_per_frame,
                                             void* d_out, size_t out_stride, uint64_t* d_sizes /*[nsheets]*/,
                                             int* modes, float* q_out, float* value_out /*host [nsheets], each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_sheet_linear_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                    const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset, out_capacity ignored*/,
                                                    const sjpeg_hip_ragged_params* params, const sjpeg_hip_sheet* sheet,
                                                    const sjpeg_hip_flatten* flatten /*or NULL*/, int light,
                                                    const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                    const uint8_t* orientations /*host [nframes], or NULL*/,
                                                    const struct sjpeg_hip_metadata* meta /*host: [nsheets], [1] or NULL*/, int meta_per_frame,
                                                    void* d_packed, size_t packed_capacity,
                                                    uint64_t* d_offsets /*[nsheets + 1]*/, uint64_t* d_sizes /*[nsheets]*/,
                                                    int* modes, float* q_out, float* value_out /*host [nsheets], each may be NULL*/,
                                                    void* stream);

/* ---- unsharp mask: thumbnails sharpened inside the ragged call ----
 * An area average is a box filter: a 1080p frame brought to 320 x 180 comes out soft, and every thumbnailer sharpens
 * behind its resize (vipsthumbnail --sharpen, ImageMagick's -thumbnail ... -unsharp, an image CDN's sharpen=).  The
 * entries below do it in ONE more small launch behind the launch that makes the pictures, on the made bytes, with one
 * right answer in integers.  ("sharp" elsewhere in this header is the reference's sharp YUV conversion; this is
 * "unsharp" throughout.)
 * THE DEFINITION.  A made plane is rows of bytes with a channel step c: 3 for interleaved RGB, 1 for gray and for a Y,
 * U or V plane.  Sample p at byte x of row y has the 3 x 3 neighbourhood n[i][j] of the samples of its channel at
 * x - c, x, x + c in rows y - 1, y, y + 1; the edge is replicated: an index outside the picture takes the nearest
 * sample of that channel inside it.  With the weights w = [1 2 1] x [1 2 1] (sum 16):
 *   S   = sum of w[i][j] * n[i][j]                  (0 .. 16 * 255)
 *   D   = 16 * p - S                                (-4080 .. 4080: sixteen times p minus the blur)
 *   out = p                                         if |D| < 16 * threshold
 *   out = min(255, max(0, floor((512 * p + amount * D + 256) / 512)))   otherwise
 * amount is 0..255 in 32nds (32: the classic 2 p - blur), threshold 0..255 in byte levels (0: every sample is
 * sharpened); floor is toward minus infinity (an arithmetic shift by 9); everything fits an int32:
 * |amount * D| <= 1 040 400.  Consequences:
 *   amount == 0 is the identity; so is threshold 255 (p itself has weight 4 in S, so |D| <= 12 * 255 < 16 * 255).
 *   A constant picture and a 1 x 1 picture come back unchanged.
 *   The kernel is symmetric under the eight EXIF orientations: sharpening commutes with the turn.
 * Known answers: every row 100 100 100 100 200 200 200 200 with amount 32, threshold 0 gives 100 100 100 75 225 200
 * 200 200, with amount 64 .. 50 250 ..; with threshold 26 the rows are unchanged, with 25 sharpened (|D| = 400 = 16 *
 * 25); the row 10 12 with amount 32 gives 10 13 (the tie rounds up); a 4 x 4 checkerboard with 100 at (0, 0) and 200
 * beside it, amount 32, has the first row 63 250 50 238.
 * ORDER OF STEPS.  RGB-like and gray formats: pixel transform, flatten, light table, average, inverse, turn, unsharp.
 * Video: resize, turn, colour conversion, unsharp on Y ONLY -- U and V are, byte for byte, what the entry without
 * unsharp makes.  What the filter reads are the made bytes, whatever made them.
 * JPEG CONTRACT, the family's usual one: frame k's JPEG is byte for byte what the _full_ call makes of the uint8
 * picture the shape entry below returns.  What is written into a made row's padding is unspecified.
 *
 * sjpeg_hip_unsharp: amount and threshold as above -- every value of either is valid --; a reserved byte that is not 0
 *   is SJPEG_HIP_EINVAL, naming the frame.  One for the call (unsharp_per_frame == 0: unsharp[0]) or one per frame.
 * sjpeg_hip_unsharp_ragged_src: sjpeg_hip_linear_ragged_src's arguments plus `unsharp, unsharp_per_frame` behind the
 *   orientations.  Same output layout, same size (sjpeg_hip_orient_ragged_bytes).
 * sjpeg_hip_encode_ragged_unsharp_src / _unsharp_packed_src: the _linear_ encode entries plus the two.
 * sjpeg_hip_unsharp_ragged_yuv_src, sjpeg_hip_encode_ragged_yuv_unsharp_src / _yuv_unsharp_packed_src: the _yuv16
 *   entries plus the two behind `depth`; depth == NULL: planes of bytes (the _yuv_converted_ entries' path).
 * unsharp == NULL, or amount 0 for every frame, is a pass-through: exactly the corresponding entry above on the same
 *   arguments, with that entry's name in the messages.  Otherwise EVERY frame goes through the resize kernel, at its
 *   own size with orientation 1 too, so "sharpen only" works for any source format; the made pictures stay in the
 *   engine's memory and the sharpened ones go to the caller's buffer or, for the encodes, into engine memory of their
 *   own (counted by sjpeg_hip_engine_scratch_bytes, released by sjpeg_hip_engine_trim).
 * SJPEG_HIP_EINVAL before any device work: a reserved byte (the frame named); a YUV-plane format given to the RGB
 *   entries, or another format given to the _yuv_ ones (named, the other entry pointed at); and every check the
 *   corresponding entry above makes.  Contact sheets are not sharpened here.
 * Host only, for bindings and tests:
 *   sjpeg_hip_unsharp_sample: *byte = out for the neighbourhood n[3 * i + j] (n[4] is p); a NULL pointer or an amount
 *     or threshold outside 0..255 is SJPEG_HIP_EINVAL. */
typedef struct sjpeg_hip_unsharp {
  uint8_t amount;                 /* 0..255 in 32nds: 32 is out = 2 p - blur */
  uint8_t threshold;              /* 0..255 in byte levels: a sample closer than this to its blur is left alone */
  uint8_t reserved[2];            /* 0 */
} sjpeg_hip_unsharp;              /* 4 bytes */
int sjpeg_hip_unsharp_sample(int amount, int threshold, const uint8_t n[9], uint32_t* byte);
int sjpeg_hip_unsharp_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                                 const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                 int light, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                 const uint8_t* orientations /*host [nframes], or NULL*/,
                                 const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                 void* d_out, size_t bytes, sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/, int* out_format,
                                 void* stream);
int sjpeg_hip_encode_ragged_unsharp_src(sjpeg_hip_engine* engine, int format, int nframes,
                                        const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                        const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/, int light,
                                        const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                        const uint8_t* orientations /*host [nframes], or NULL*/,
                                        const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                        const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                        void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                        int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_unsharp_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                               const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                               const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                               int light, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                               const uint8_t* orientations /*host [nframes], or NULL*/,
                                               const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                               const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                               void* d_packed, size_t packed_capacity,
                                               uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                               int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                               void* stream);
int sjpeg_hip_unsharp_ragged_yuv_src(sjpeg_hip_engine* engine, int format, int nframes,
                                     const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                     const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                     const uint8_t* orientations /*host [nframes], or NULL*/,
                                     const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                     const sjpeg_hip_yuv_depth* depth /*or NULL: planes of bytes*/,
                                     const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                     void* d_out, size_t bytes, sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/,
                                     int* out_format, void* stream);
int sjpeg_hip_encode_ragged_yuv_unsharp_src(sjpeg_hip_engine* engine, int format, int nframes,
                                            const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                            const sjpeg_hip_ragged_params* params, const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                            const uint8_t* orientations /*host [nframes], or NULL*/,
                                            const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                            const sjpeg_hip_yuv_depth* depth /*or NULL: planes of bytes*/,
                                            const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                            const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                            void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                            int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_yuv_unsharp_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                   const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                                   const sjpeg_hip_ragged_params* params,
                                                   const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                   const uint8_t* orientations /*host [nframes], or NULL*/,
                                                   const sjpeg_hip_yuv_colour* colour /*host: [nframes], [1] or NULL*/, int colour_per_frame,
                                                   const sjpeg_hip_yuv_depth* depth /*or NULL: planes of bytes*/,
                                                   const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                                   const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                                   void* d_packed, size_t packed_capacity,
                                                   uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                                   int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                                   void* stream);

/* ---- resampling with Pillow's filters: Lanczos, bicubic, bilinear, Hamming and box windows, enlarging too ----
 * Every shape entry above makes its picture with one filter, the exact area average: it only shrinks, it is soft, and
 * it is this library's own answer.  The thumbnails of Python services and dataset pipelines were made by
 * PIL.Image.resize(size, LANCZOS | BICUBIC | BILINEAR | HAMMING | BOX); the entries below make THOSE bytes -- Pillow
 * 12.2.0's, for pictures of bytes -- in ONE launch of a kernel of its own over the batch, to sizes smaller or larger
 * than the source on either axis.
 * THE DEFINITION (one right answer, in integers, given the tables).  A picture of bytes, channels independent, is
 * resampled along x, then along y, with a uint8 intermediate between the passes.  A pass whose input and output size
 * agree is not run; both agreeing is the identity.  Along an axis from `in` to `out` samples with filter f of support
 * s, all in IEEE double:
 *   scale = in / out; fs = max(scale, 1.0); support = s * fs; ksize = 2 * (int)ceil(support) + 1
 *   for output index xx:  center = (xx + 0.5) * scale
 *     xmin = max(0, (int)(center - support + 0.5));  n = min(in, (int)(center + support + 0.5)) - xmin
 *     w[x] = f((x + xmin - center + 0.5) / fs) for x < n;  ww = the sum of w in index order
 *     k[x] = w[x] / ww (left as w[x] when ww == 0)
 *     K[x] = (int)(k[x] * 2^22 + 0.5) for k >= 0, else (int)(k[x] * 2^22 - 0.5)        (C truncation)
 *   out[xx] = min(255, max(0, (2^21 + sum over x < n of K[x] * b[xmin + x]) >> 22))     (int32, arithmetic shift)
 * The filters (x is made |x| first, except for lanczos):
 *   box, support 0.5:      1 for -0.5 < x <= 0.5 on the signed x
 *   bilinear, support 1:   1 - x for x < 1
 *   hamming, support 1:    1 at 0, 0 for x >= 1, else sin(pi x) / (pi x) * (0.54f + 0.46f * cos(pi x)) -- the two
 *                          constants are floats promoted to double
 *   bicubic, support 2:    a = -0.5: ((a + 2) x - (a + 3)) x x + 1 for x < 1, (((x - 5) x + 8) x - 4) a for x < 2
 *   lanczos, support 3:    sinc(x) * sinc(x / 3) for -3 <= x < 3, sinc(0) = 1, sinc(x) = sin(pi x) / (pi x)
 * The tables are made on the host -- they need the host's sin and cos -- and uploaded, once per (filter, in, out) that
 * occurs in a call; the kernel is integers only.  Two bounds are CHECKED for every table a call builds, and the kernel
 * relies on them: every |K| < 2^23 (both factors of a product fit 24 bits), and 2^21 + 255 * max(sum of the positive
 * K, sum of the |negative K|) < 2^31 for every sample.  Measured, not proven: over in 1..69, 100, 257, 1000, 1920, 3840
 * and out 1..69, 100, 180, 320, 1000, 4000 and the five filters the largest |K| is 5 392 348 and the largest sum
 * 1 377 229 532.  A table that breaks one is refused with SJPEG_HIP_EINVAL, the frame and the axis named.
 * THE CAP.  An axis whose ksize is above 385 -- Lanczos shrinking by more than 64, box by more than 384 -- is refused
 * before any device work, the frame, the axis, its ksize and the cap named.  Below the cap every size is taken, 1 x 1
 * sources and 1 x 1 results included.
 * Known answers (tests/golden/resample_pillow.npz, recorded from Pillow 12.2.0): the row 0 255 brought to 4 samples is
 * 0 0 255 255 (box), 0 64 191 255 (bilinear), 0 19 236 255 (hamming), 0 53 202 255 (bicubic), 0 59 196 255 (lanczos);
 * the row 10 20 30 40 250 240 230 220 brought to 2 samples is 25 235, 57 207, 38 224, 47 217, 46 220 in that order;
 * the bilinear table of 7 -> 3 samples has the windows {0, 4}, {1, 5}, {4, 3} and its middle row is 246724 986895
 * 1727066 986895 246724.
 * FORMATS AND ORDER OF STEPS.  Every RGB-like and gray format the resize takes: pixel transform, flatten (optional, as
 * in the _flattened_ entries; without it a fourth sample is dropped), resample, turn, unsharp (optional).  What the
 * filter reads is the byte the encoder sees.  `sizes` are in the STORED orientation, 1..65535 each, and may exceed
 * the source on either axis (NULL: every frame at its own size); the upright picture is U = turn(R), R the resampled
 * stored picture -- the family's "resize, then turn".  It is NOT exif_transpose followed by resize: two passes with a
 * rounded intermediate do not commute with the turn.  unsharp (NULL or amount 0 for every frame: none) is the launch
 * of the _unsharp_ entries, unchanged, behind the resample launch.  There is no linear light and there are no contact
 * sheets here: the entries have no `light` and no sheet argument.  The YUV-plane formats, bytes or 16-bit samples, are
 * refused by name.
 * EVERY frame goes through the kernel: a frame at its own size is copied (turned, flattened), as with unsharp.
 * A picture more than 100 times as tall as wide that is brought to fewer rows is resampled along x first here too;
 * Pillow resamples such a picture along y first, so for it these entries do not make Pillow's bytes (the box entries
 * below refuse it).
 * JPEG CONTRACT, the family's usual one: frame k's JPEG is byte for byte what the _full_ call makes of the uint8
 * picture the shape entry below returns.  What is written into a made row's padding is unspecified.
 *
 * sjpeg_hip_resample: the filter, one of SJPEG_HIP_RESAMPLE_*; reserved must be 0.  One for the call
 *   (resample_per_frame == 0: resample[0]) or one per frame, so filters mix inside a launch.
 * sjpeg_hip_resample_ragged_bytes: the bytes the made pictures take, in the layout of the oriented pictures
 *   (sjpeg_hip_orient_ragged_bytes: interleaved RGB or gray, rows whole dwords apart, pictures at multiples of 16); 0
 *   for a batch the call refuses.
 * sjpeg_hip_resample_ragged_src: the uint8 pictures into d_out; out_frames and out_format as the other shape entries.
 * sjpeg_hip_encode_ragged_resampled_src / _resampled_packed_src: the _unsharp_ encode entries' arguments without
 *   `light`, plus `resample, resample_per_frame` in front of the unsharp.
 * The tables, the made pictures and the sharpened ones are engine memory, counted by sjpeg_hip_engine_scratch_bytes and
 *   released by sjpeg_hip_engine_trim.
 * SJPEG_HIP_EINVAL before any device work, the frame named: resample == NULL; a filter that is none of the five; a
 *   reserved byte; a size below 1 or above 65535; an axis above the cap; a YUV-plane format (named); and the checks
 *   of the flattened and unsharp entries on their arguments.
 * Host only, for bindings and tests:
 *   sjpeg_hip_resample_ksize: ksize of an axis (filter, in, out: 1..65535 each); 0 with the error set otherwise.
 *   sjpeg_hip_resample_table: bounds[xx] = {xmin, n} and K[xx * ksize + x] (x >= n: 0) of an axis, whatever its ksize;
 *     K_capacity counts int32s and must be at least out * ksize.  A table that breaks a bound is SJPEG_HIP_EINVAL. */
#define SJPEG_HIP_RESAMPLE_BOX 0
#define SJPEG_HIP_RESAMPLE_BILINEAR 1
#define SJPEG_HIP_RESAMPLE_HAMMING 2
#define SJPEG_HIP_RESAMPLE_BICUBIC 3
#define SJPEG_HIP_RESAMPLE_LANCZOS 4
typedef struct sjpeg_hip_resample {
  uint8_t filter;                 /* SJPEG_HIP_RESAMPLE_* */
  uint8_t reserved[3];            /* 0 */
} sjpeg_hip_resample;             /* 4 bytes */
int sjpeg_hip_resample_ksize(int filter, int in, int out);
int sjpeg_hip_resample_table(int filter, int in, int out, int32_t (*bounds)[2] /*[out]*/, int32_t* K /*[out * ksize]*/, size_t K_capacity);
size_t sjpeg_hip_resample_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                       const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                       const uint8_t* orientations /*host [nframes], or NULL*/);
int sjpeg_hip_resample_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                                  const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                  const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                  const uint8_t* orientations /*host [nframes], or NULL*/,
                                  const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                  const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                  void* d_out, size_t bytes, sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/, int* out_format,
                                  void* stream);
int sjpeg_hip_encode_ragged_resampled_src(sjpeg_hip_engine* engine, int format, int nframes,
                                          const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                          const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                          const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                          const uint8_t* orientations /*host [nframes], or NULL*/,
                                          const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                          const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                          const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                          void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                          int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_resampled_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                 const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                                 const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                                 const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                 const uint8_t* orientations /*host [nframes], or NULL*/,
                                                 const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                                 const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                                 const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                                 void* d_packed, size_t packed_capacity,
                                                 uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                                 int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                                 void* stream);

/* ---- ... from a source box and behind a reduce: Image.thumbnail and ImageOps.fit ----
 * The thumbnails of Python services mostly do not come from a bare resize.  Image.thumbnail(box) -- BICUBIC,
 * reducing_gap 2.0 -- first runs Image.reduce, an integer box average with Pillow's own rounding, where the source is
 * at least 2 * gap times the target, and resizes the small picture from a FRACTIONAL source box; ImageOps.fit, crop to
 * fill, is a resize from a fractional crop.  The entries below make those bytes -- Pillow 12.2.0's -- of the same
 * formats, in the same order of steps and under the same JPEG contract as the _resampled_ entries above.  The reduce is
 * also what makes large shrinks cheap, and it lifts THE CAP: the cap applies to the window behind the reduce, so 4000 ->
 * 40 samples with Lanczos and reducing_gap 2.0 is a factor 50 and a window of 13.
 * THE DEFINITION of the box entries (sjpeg_amd/csrc/resample_math.h states it once, for the host, the kernel and the
 * tests).  A frame has the stored picture P of W x H bytes per channel (behind the pixel transform and the flatten),
 * the target (w2, h2), the filter of support s, a source box (l, t, r, b) in doubles, in P's samples, and a
 * reducing_gap g.  "double" is IEEE double as Python does it, int() truncates toward zero.
 *   1. The box: 0 <= l, 0 <= t, r <= W, b <= H, r - l > 0, b - t > 0, else refused.  (Pillow takes an empty box; these
 *      entries do not.)  The all-zero box is (0, 0, W, H).
 *   2. The reduce, where g is not 0: fx = int((r - l) / w2 / g) or 1, fy likewise.  Both 1: nothing.  Else, with
 *      sx = (r - l) / w2, sy = (b - t) / h2 and u = s - 0.5, the safe box is R = (max(0, int(l - u sx)),
 *      max(0, int(t - u sy)), min(W, ceil(r + u sx)), min(H, ceil(b + u sy))); the reduced picture has
 *      ceil((R2 - R0) / fx) x ceil((R3 - R1) / fy) samples, each of a block of n = fx * fy source samples from (R0, R1)
 *      on, fewer on the right and bottom edge: ((S + n / 2) * m(n)) >> 24 in uint32, S the block's sum, n / 2 the
 *      integer quotient, m(n) = (uint32)(4294967296.0f / (float)(256 * n)) -- a FLOAT32 division, truncated; it is not
 *      floor(2^24 / n), and the sample is not the exact half-up average of the _reduced_ entries.  The box becomes
 *      ((l - R0) / fx, (t - R1) / fy, (r - R0) / fx, (b - R1) / fy) in double, and P, W, H are the reduced picture's.
 *   3. H > 100 * W and h2 < H: refused -- Pillow resamples such a picture along y first.
 *   4. The tables, of the box rounded to float32, bf: the x pass runs if w2 != W or bf[0] != 0 or bf[2] != W, the y pass
 *      likewise; a pass that does not run has the identity table.  scale = (double)(float)(bf[2] - bf[0]) / w2, the
 *      subtraction in float32; fs, support and ksize as above; center = (double)bf[0] + (xx + 0.5) * scale;
 *      xmin = max(0, int(center - support + 0.5)), xmax = min(W, int(center + support + 0.5)).  The windows are clamped
 *      to the PICTURE, not to the box: samples outside the box are read, as Pillow reads them.  Weights, normalisation
 *      and rounding as above; both bounds and the windows are checked for every table.
 *   5. The x pass, the uint8 intermediate, the y pass, the turn and the unsharp mask as above.
 * With the all-zero box and g = 0 the picture is byte for byte that of the _resampled_ entries; a g whose factors are
 * both 1 changes nothing.  Boxes and sizes are in the STORED orientation.
 * ONE LAUNCH.  A call none of whose frames is reduced runs the kernel of the _resampled_ entries (its tables satisfy
 * what that kernel relies on).  A call with a reduced frame runs ALL its frames through a kernel of its own
 * (resample_box.hip) that sums every block as it stages it; there a frame with factors 1 x 1 has m = 2^24.
 *
 * sjpeg_hip_resample_box: box and reducing_gap (0: none, else 1.0 .. 65536.0).  One for the call (box_per_frame == 0:
 *   box[0]) or one per frame.  A factor above 255 is refused.
 * sjpeg_hip_resample_box_ragged_src, sjpeg_hip_encode_ragged_resampled_box_src / _box_packed_src: the _resampled_
 *   entries' arguments plus `box, box_per_frame` behind the resample; the made pictures take what
 *   sjpeg_hip_resample_ragged_bytes says -- their layout depends on sizes and orientations alone -- or, where that
 *   function refuses an axis by the cap that the reduce lifts, sjpeg_hip_resample_box_ragged_bytes.
 * SJPEG_HIP_EINVAL before any device work, the frame named: box == NULL; a box that is empty or leaves the picture; a
 *   reducing_gap that is neither 0 nor in 1.0 .. 65536.0; a factor above 255; the tall picture of step 3; and
 *   everything the _resampled_ entries refuse, the cap taken behind the reduce.
 * Host only, for bindings and tests (0, or SJPEG_HIP_EINVAL with the error set):
 *   sjpeg_hip_thumbnail_size: the size Image.thumbnail((bw, bh)) gives a width x height picture: the box sides floored
 *     (each at least 1), never larger than the picture, the aspect kept by Pillow's round_aspect.
 *   sjpeg_hip_fit_crop: ImageOps.fit's crop box of a width x height picture for the size out_width x out_height.
 *   sjpeg_hip_resample_box_decide: what steps 1 to 3 come to for one frame: the factors, the safe box, the reduced
 *     picture's size, the four multipliers (interior, right edge, bottom edge, corner) and the box in that picture.
 *   sjpeg_hip_resample_box_ksize, sjpeg_hip_resample_box_table: sjpeg_hip_resample_ksize and _table of step 4, of an
 *     axis of `in` samples and the box ends b0 < b1 inside it, given as float32. */
typedef struct sjpeg_hip_resample_box {
  double box[4];                  /* left, top, right, bottom in the stored picture's samples; all 0: the whole picture */
  double reducing_gap;            /* 0: no reduce */
} sjpeg_hip_resample_box;         /* 40 bytes */
typedef struct sjpeg_hip_resample_box_decision {
  int32_t factor[2];              /* fx, fy */
  int32_t safe_box[4];            /* R; factors 1 x 1: the whole picture */
  int32_t reduced_size[2];        /* W, H of the picture the tables are of */
  uint32_t multiplier[4];         /* m of an interior, right-edge, bottom-edge and corner block */
  double inner_box[4];            /* the box in the reduced picture's samples */
} sjpeg_hip_resample_box_decision;
int sjpeg_hip_thumbnail_size(int width, int height, double box_width, double box_height, int32_t size[2] /*out*/);
int sjpeg_hip_fit_crop(int width, int height, int out_width, int out_height, double bleed, double centering_x, double centering_y,
                       double box[4] /*out*/);
int sjpeg_hip_resample_box_decide(int filter, int width, int height, int out_width, int out_height, const sjpeg_hip_resample_box* box,
                                  sjpeg_hip_resample_box_decision* decision /*out*/);
int sjpeg_hip_resample_box_ksize(int filter, int in, int out, float b0, float b1);
int sjpeg_hip_resample_box_table(int filter, int in, int out, float b0, float b1, int32_t (*bounds)[2] /*[out]*/,
                                 int32_t* K /*[out * ksize]*/, size_t K_capacity);
size_t sjpeg_hip_resample_box_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                           const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                           const uint8_t* orientations /*host [nframes], or NULL*/,
                                           const sjpeg_hip_resample_box* box /*host: [nframes] or [1]*/, int box_per_frame);
int sjpeg_hip_resample_box_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                                      const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                      const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                      const uint8_t* orientations /*host [nframes], or NULL*/,
                                      const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                      const sjpeg_hip_resample_box* box /*host: [nframes] or [1]*/, int box_per_frame,
                                      const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                      void* d_out, size_t bytes, sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/, int* out_format,
                                      void* stream);
int sjpeg_hip_encode_ragged_resampled_box_src(sjpeg_hip_engine* engine, int format, int nframes,
                                              const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                              const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                              const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                              const uint8_t* orientations /*host [nframes], or NULL*/,
                                              const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                              const sjpeg_hip_resample_box* box /*host: [nframes] or [1]*/, int box_per_frame,
                                              const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                              const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                              void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                              int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_resampled_box_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                     const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                                     const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                                     const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                     const uint8_t* orientations /*host [nframes], or NULL*/,
                                                     const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                                     const sjpeg_hip_resample_box* box /*host: [nframes] or [1]*/, int box_per_frame,
                                                     const sjpeg_hip_unsharp* unsharp /*host: [nframes], [1] or NULL*/, int unsharp_per_frame,
                                                     const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                                     void* d_packed, size_t packed_capacity,
                                                     uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                                     int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                                     void* stream);

/* ---- ... and filtered behind it: Pillow's GaussianBlur, BoxBlur and UnsharpMask ----
 * A Python thumbnailer does not stop at thumbnail(): it ends in filter(ImageFilter.UnsharpMask(2, 150, 3)), or in
 * filter(GaussianBlur(r)) for a blurred placeholder.  The entries below run that last link inside the call and make
 * Pillow 12.2.0's bytes.  (The _unsharp entries above are a 3 x 3 mask of this library's own definition; they do not.)
 * THE FILTER runs over the MADE upright bytes, whatever made them: filter(turn(resample(flatten(stored)))), RGB or gray.
 * It is the last step, where the unsharp launch of the _resampled_box_ entries stands; rx and ry are the upright
 * picture's.  THE DEFINITION (sjpeg_amd/csrc/pillow_filter_math.h states it once, for the host, the kernel and the
 * tests); every band of an RGB picture is filtered alike:
 *   One box pass along a line of n samples of one channel, float radius fr > 0 (a float32): r = (int) fr,
 *     ww = (uint32) (16777216.0f / (fr * 2.0f + 1.0f)) -- the sum and the division in FLOAT32, truncated; divided in
 *     double, radii 0.3 and 2.7 make other bytes --, fw = (2^24 - (2 r + 1) ww) / 2, and
 *     out[x] = (ww * SUM(d = -r .. r) in[c(x + d)] + fw * (in[c(x - r - 1)] + in[c(x + r + 1)]) + 2^23) >> 24 in uint32,
 *     c() clamping an index into 0 .. n - 1: edges are replicated.
 *   Box blur (rx, ry): one pass along every row with rx, then one along every column of that uint8 result with ry.  An
 *     axis whose radius is 0 is skipped.
 *   Gaussian blur (sx, sy): THREE passes along the rows, each rounded to uint8, then three along the columns, with
 *     fr = g(sigma): s2 = sigma * sigma / 3; L = sqrt(12 s2 + 1); l = floor((L - 1) / 2);
 *     a = (2 l + 1) (l (l + 1) - 3 s2) / (6 (s2 - (l + 1) (l + 1))); fr = l + a -- every operation rounded to FLOAT32 but
 *     sqrt and floor, which take and return double.  (In doubles many sigmas give another radius.)  Sigma 1 gives 0.25,
 *     sigma 2 gives 1.375.  An axis whose fr is 0 is skipped.
 *   Unsharp mask (radius, percent, threshold): b the Gaussian blur (radius, radius) of the picture; per sample d = p - b;
 *     |d| > threshold (STRICTLY): clip(p + d * percent / 100, 0, 255), the division C's, toward zero; else p.
 * TWO LAUNCHES over the batch's tiles behind the launch that made the pictures, never one per pass or per picture:
 * every pass along the rows into engine scratch of the made pictures' layout, every pass along the columns (and the
 * unsharp combine) from there into the output.  On the device there are only integers.
 *
 * sjpeg_hip_pillow_filter: kind 0 none, 1 box blur, 2 Gaussian blur, 3 unsharp mask; threshold and percent for kind 3;
 *   radius_x, radius_y: box radii (kind 1) or sigmas (2, 3; kind 3: both equal).  One for the call
 *   (filter_per_frame == 0: filter[0]) or one per frame, kinds mixed.
 * sjpeg_hip_filter_ragged_src, sjpeg_hip_encode_ragged_filtered_src / _filtered_packed_src: the _resampled_box_
 *   entries' arguments with `unsharp, unsharp_per_frame` replaced by `filter, filter_per_frame`; same layout, same
 *   bytes function, same JPEG contract.  filter == NULL, or kind 0 for every frame: exactly the _resampled_box_ entry
 *   without unsharp -- byte for byte, its messages under its name, no launch more.
 * SJPEG_HIP_EINVAL before any device work, the frame named: a kind above 3; a radius that is negative or not finite; an
 *   axis whose integer box radius r exceeds 63 -- a box radius of 64 or a sigma above about 64: Pillow has no such
 *   limit, the kernel's staging has --; kind 3 with radius_x != radius_y; a reserved byte that is not 0; made pictures
 *   that are neither RGB nor gray; and everything the _resampled_box_ entries refuse.  Every axis is also held to
 *   (2 r + 1) * ww <= 2^24, which the uint32 above relies on.
 * Host only, for bindings and tests (0, or SJPEG_HIP_EINVAL with the error set):
 *   sjpeg_hip_pillow_filter_weights: r, ww, fw and the number of passes of ONE axis of a kind (1..3) with `radius`;
 *     passes 0: the axis is skipped.  The same refusals. */
typedef struct sjpeg_hip_pillow_filter {
  uint8_t kind;                   /* 0 none, 1 box blur, 2 Gaussian blur, 3 unsharp mask */
  uint8_t threshold;              /* kind 3: 0..255 */
  uint16_t percent;               /* kind 3 */
  float radius_x, radius_y;       /* along the rows, along the columns of the upright picture */
  uint8_t reserved[4];            /* must be 0 */
} sjpeg_hip_pillow_filter;        /* 16 bytes */
int sjpeg_hip_pillow_filter_weights(int kind, float radius, uint32_t* r, uint32_t* ww, uint32_t* fw, uint32_t* passes /*out*/);
int sjpeg_hip_filter_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                                const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                const uint8_t* orientations /*host [nframes], or NULL*/,
                                const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                const sjpeg_hip_resample_box* box /*host: [nframes] or [1]*/, int box_per_frame,
                                const sjpeg_hip_pillow_filter* filter /*host: [nframes], [1] or NULL*/, int filter_per_frame,
                                void* d_out, size_t bytes, sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/, int* out_format,
                                void* stream);
int sjpeg_hip_encode_ragged_filtered_src(sjpeg_hip_engine* engine, int format, int nframes,
                                         const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                         const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                         const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                         const uint8_t* orientations /*host [nframes], or NULL*/,
                                         const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                         const sjpeg_hip_resample_box* box /*host: [nframes] or [1]*/, int box_per_frame,
                                         const sjpeg_hip_pillow_filter* filter /*host: [nframes], [1] or NULL*/, int filter_per_frame,
                                         const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                         void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                         int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_filtered_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                                const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                                const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                const uint8_t* orientations /*host [nframes], or NULL*/,
                                                const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                                const sjpeg_hip_resample_box* box /*host: [nframes] or [1]*/, int box_per_frame,
                                                const sjpeg_hip_pillow_filter* filter /*host: [nframes], [1] or NULL*/, int filter_per_frame,
                                                const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                                void* d_packed, size_t packed_capacity,
                                                uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                                int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                                void* stream);

/* ---- ... and composed behind that: Pillow's ImageOps.pad / expand and the paste of an RGBA overlay ----
 * Between filter() and save() a Python thumbnailer often has two more links: ImageOps.pad(im, (256, 256), color=...) --
 * a fixed tile, a letterboxed square -- and im.paste(logo, (x, y), logo), a watermark or badge.  The entries below run
 * both inside the call and make Pillow 12.2.0's bytes.  COMPOSE is the last link, over the MADE upright bytes:
 * compose(filter(turn(resample(flatten(stored))))), RGB or gray; every coordinate is the UPRIGHT picture's.
 * THE DEFINITION (sjpeg_amd/csrc/compose_math.h states it once, for the host, the kernel and the tests):
 *   Canvas: canvas_width x canvas_height samples filled with colour (a gray picture: colour[0]); the made w x h picture
 *     is copied to (px, py) and must lie wholly inside.  canvas_width == canvas_height == 0: the picture's own size, no
 *     fill.  mode 0: (px, py) as given.  mode 1: Pillow's pad rule from the centering (cx, cy), each clamped into 0..1:
 *     px = round((canvas_width - w) * cx), py likewise, round() Python's (half to even, on the double).
 *   Overlay places: behind the canvas, places[first_place .. first_place + nplaces) IN LIST ORDER (two overlapping
 *     overlays do not commute).  A place puts overlays[overlay] with its top-left at (ox, oy) ON THE CANVAS: anchor 0
 *     top-left (ox = x, oy = y), 1 top-right (ox = cw - ow - x), 2 bottom-left (oy = ch - oh - y), 3 bottom-right
 *     (both), 4 centre (ox = floor((cw - ow) / 2) + x, oy likewise) -- (x, y) the margin inward from the anchor, so ONE
 *     struct for the call means "pad to 256 x 256, logo 8 from the bottom-right corner" over pictures of every size.
 *     The overlay is clipped to the canvas; it may lie partly or wholly outside, where it does nothing; it covers the
 *     padding as it covers the picture.  Every covered sample: out = blend(out, src, a), a the overlay's alpha,
 *     t = out * (255 - a) + src * a + 128; blend = ((t >> 8) + t) >> 8 -- (out * (255 - a) + src * a + 127) / 255, which
 *     is Pillow's paste with the overlay as mask and Image.alpha_composite over an opaque base alike; NOT the sum of two
 *     rounded products.  src is the overlay's channel on an RGB picture, and on a gray one its luma
 *     (19595 R + 38470 G + 7471 B + 32768) >> 16.
 *   Overlays: straight-alpha RGBA bytes on the device, given once per call and referenced by index -- one logo serves
 *     every frame and is never copied.
 * ONE LAUNCH over the tiles of every canvas of the batch behind the launches that made the pictures, out of place.
 *
 * sjpeg_hip_compose_ragged_bytes: what the canvases take in d_out (0: the call would be refused).
 * sjpeg_hip_compose_ragged_src, sjpeg_hip_encode_ragged_composed_src / _composed_packed_src: the _filtered_ entries'
 *   arguments plus compose ([nframes]; compose_per_frame == 0: compose[0] for every frame; NULL), overlays [noverlays]
 *   and places [nplaces].  The usual layout: every canvas at a multiple of 16, rows whole dwords apart; out_frames carry
 *   the CANVAS sizes.  Frame k's JPEG is byte for byte what sjpeg_hip_encode_ragged_full_src makes of the canvas.
 *   compose == NULL, or every frame an identity (canvas 0 x 0 or the picture's own size at (0, 0), and no places):
 *   exactly the _filtered_ entry -- byte for byte, its messages under its name, no launch more.  A call none of whose
 *   frames has a filter runs no filter launch.
 * SJPEG_HIP_EINVAL before any device work, the frame (or overlay, or place) named: a canvas side outside 1..65535
 *   unless both are 0; a picture not wholly inside its canvas; centerings that are not finite; a mode above 1 or an
 *   anchor above 4; first_place + nplaces beyond the call's nplaces; more than 8 places for one frame; an overlay index
 *   out of range; an overlay with a NULL pointer or one that is no multiple of 4, a side outside 1..65535, a stride
 *   below 4 * width or no multiple of 4; a reserved byte that is not 0; made pictures that are neither RGB nor gray; and
 *   everything the _filtered_ entries refuse.
 * Host only, for bindings and tests (0, or SJPEG_HIP_EINVAL with the error set):
 *   sjpeg_hip_contain_size: ImageOps.contain's target (out[0], out[1]) of a width x height picture in box_width x
 *     box_height -- the box where width / height == box_width / box_height in doubles, else (box_width,
 *     round(height / width * box_width)) or (round(width / height * box_height), box_height); a target side of 0
 *     (1000 x 1 into 10 x 10) is refused, as Pillow raises.
 *   sjpeg_hip_pad_place: (out[0], out[1]) = (px, py) of mode 1 for a width x height picture on a canvas.
 *   sjpeg_hip_compose_sample: blend(dst, src, a) of one sample; gray != 0: src is the luma of (r, g, b), else r. */
typedef struct sjpeg_hip_overlay {
  const void* rgba;               /* device: R, G, B, A bytes a pixel, straight alpha; a multiple of 4 */
  int32_t width, height;          /* 1..65535 each */
  int64_t stride;                 /* bytes between rows: a multiple of 4, at least 4 * width */
} sjpeg_hip_overlay;              /* 24 bytes */
typedef struct sjpeg_hip_overlay_place {
  int32_t overlay;                /* index into the call's overlays */
  int32_t x, y;                   /* the margin inward from the anchor; may be negative */
  uint8_t anchor;                 /* 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right, 4 centre */
  uint8_t reserved[3];            /* must be 0 */
} sjpeg_hip_overlay_place;        /* 16 bytes */
typedef struct sjpeg_hip_compose {
  int32_t canvas_width, canvas_height; /* 1..65535 each, or both 0: the picture's own size */
  uint8_t mode;                   /* 0: the picture at (px, py); 1: by the centering (cx, cy), Pillow's pad rule */
  uint8_t colour[3];              /* the canvas's R, G, B; a gray picture uses colour[0] */
  int32_t px, py;                 /* mode 0 */
  uint8_t reserved[4];            /* must be 0 */
  double cx, cy;                  /* mode 1: clamped into 0..1 */
  int32_t first_place, nplaces;   /* this frame's places: places[first_place .. first_place + nplaces), at most 8 */
} sjpeg_hip_compose;              /* 48 bytes */
int sjpeg_hip_contain_size(int width, int height, int box_width, int box_height, int32_t* out /*[2]*/);
int sjpeg_hip_pad_place(int width, int height, int canvas_width, int canvas_height, double cx, double cy, int32_t* out /*[2]*/);
int sjpeg_hip_compose_sample(int dst, int r, int g, int b, int a, int gray);
size_t sjpeg_hip_compose_ragged_bytes(int format, int nframes, const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                      const int32_t (*sizes)[2] /*or NULL*/, const uint8_t* orientations /*or NULL*/,
                                      const sjpeg_hip_resample_box* box /*host: [nframes] or [1]*/, int box_per_frame,
                                      const sjpeg_hip_compose* compose /*host: [nframes], [1] or NULL*/, int compose_per_frame);
int sjpeg_hip_compose_ragged_src(sjpeg_hip_engine* engine, int format, int nframes,
                                 const sjpeg_hip_ragged_frame* frames /*[nframes], host*/, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                 const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                 const uint8_t* orientations /*host [nframes], or NULL*/,
                                 const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                 const sjpeg_hip_resample_box* box /*host: [nframes] or [1]*/, int box_per_frame,
                                 const sjpeg_hip_pillow_filter* filter /*host: [nframes], [1] or NULL*/, int filter_per_frame,
                                 const sjpeg_hip_compose* compose /*host: [nframes], [1] or NULL*/, int compose_per_frame,
                                 const sjpeg_hip_overlay* overlays /*host [noverlays], or NULL*/, int noverlays,
                                 const sjpeg_hip_overlay_place* places /*host [nplaces], or NULL*/, int nplaces,
                                 void* d_out, size_t bytes, sjpeg_hip_ragged_frame* out_frames /*host out [nframes]*/, int* out_format,
                                 void* stream);
int sjpeg_hip_encode_ragged_composed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                         const sjpeg_hip_ragged_frame* frames /*[nframes], host*/,
                                         const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                         const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                         const uint8_t* orientations /*host [nframes], or NULL*/,
                                         const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                         const sjpeg_hip_resample_box* box /*host: [nframes] or [1]*/, int box_per_frame,
                                         const sjpeg_hip_pillow_filter* filter /*host: [nframes], [1] or NULL*/, int filter_per_frame,
                                         const sjpeg_hip_compose* compose /*host: [nframes], [1] or NULL*/, int compose_per_frame,
                                         const sjpeg_hip_overlay* overlays /*host [noverlays], or NULL*/, int noverlays,
                                         const sjpeg_hip_overlay_place* places /*host [nplaces], or NULL*/, int nplaces,
                                         const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                         void* d_out, uint64_t* d_sizes /*[nframes]*/,
                                         int* modes, float* q_out, float* value_out /*host, each may be NULL*/, void* stream);
int sjpeg_hip_encode_ragged_composed_packed_src(sjpeg_hip_engine* engine, int format, int nframes,
                                                const sjpeg_hip_ragged_frame* frames /*[nframes], host; out_offset ignored*/,
                                                const sjpeg_hip_ragged_params* params, const sjpeg_hip_flatten* flatten /*or NULL*/,
                                                const int32_t (*sizes)[2] /*host int32[nframes][2], or NULL*/,
                                                const uint8_t* orientations /*host [nframes], or NULL*/,
                                                const sjpeg_hip_resample* resample /*host: [nframes] or [1]*/, int resample_per_frame,
                                                const sjpeg_hip_resample_box* box /*host: [nframes] or [1]*/, int box_per_frame,
                                                const sjpeg_hip_pillow_filter* filter /*host: [nframes], [1] or NULL*/, int filter_per_frame,
                                                const sjpeg_hip_compose* compose /*host: [nframes], [1] or NULL*/, int compose_per_frame,
                                                const sjpeg_hip_overlay* overlays /*host [noverlays], or NULL*/, int noverlays,
                                                const sjpeg_hip_overlay_place* places /*host [nplaces], or NULL*/, int nplaces,
                                                const struct sjpeg_hip_metadata* meta /*host: [nframes], [1] or NULL*/, int meta_per_frame,
                                                void* d_packed, size_t packed_capacity,
                                                uint64_t* d_offsets /*[nframes + 1]*/, uint64_t* d_sizes /*[nframes]*/,
                                                int* modes, float* q_out, float* value_out /*host, each may be NULL*/,
                                                void* stream);

/* ---- host-side helpers (tiny CPU work, no device needed) -----------------------------
 * They produce exactly what the reference's host code would hand to its hot loop, so that
 * a non-C++ binding can drive sjpeg_hip_encode_scan() without re-implementing them. */

/* quality -> the two 8-bit matrices (natural order) of Encoder::SetQuality
 * (src/enc.cc:100-104, src/quantize.cc:77-96). */
void sjpeg_hip_quality_matrices(float quality, uint8_t quant[2][64]);

/* Encoder::FinalizeQuantMatrix for both tables (src/quantize.cc:123-148): clamps quant to
 * min_quant (NULL = all ones) IN PLACE and fills tables->iquant / tables->bias.
 * q_bias is the reference's quantization_bias (default 0x78). */
void sjpeg_hip_finalize_quant(uint8_t quant[2][64], const uint8_t* min_quant /*[2][64]*/,
                              int q_bias, sjpeg_hip_scan_tables* tables);

/* Installs the default (JPEG Annex K.3) Huffman codes, as WriteDHT/InitCodes does for
 * method 0 (src/headers.cc:221-222, src/entropy.cc:84-128). */
void sjpeg_hip_default_huffman(sjpeg_hip_scan_tables* tables);

/* Writes SOI+APP0, DQT, SOF0, DHT (default tables), SOS for a frame without metadata into
 * buf (capacity cap), bytes identical to src/headers.cc.  Returns the size, 0 on error. */
size_t sjpeg_hip_make_header(int width, int height, int yuv_mode, const uint8_t quant[2][64],
                             uint8_t* buf, size_t cap);

/* Encoder::AnalyseHisto (src/histogram.cc:126-315) on ONE frame's histogram (host memory,
 * uint32 [2][64][128]): adapts quant IN PLACE, then re-finalises both tables into `tables`
 * exactly like the reference (quantization clamped to min_quant, NULL = all ones).
 * qdelta_max_* are EncoderParam::qdelta_max_luma / _chroma (defaults 12 / 1). */
void sjpeg_hip_adapt_quant(const uint32_t* hist, int yuv_mode, uint8_t quant[2][64],
                           const uint8_t* min_quant /*[2][64]*/, int q_bias,
                           int qdelta_max_luma, int qdelta_max_chroma,
                           sjpeg_hip_scan_tables* tables);

/* The same analysis with its bin loops on the device (src/histogram.cc:150-205): for every table,
 * position and candidate step (-12 .. +12 around quant) the rate and distortion sums over the
 * histogram, d_sums[nframes][2][64][25][2] (int64: bits, distortion; distortion == INT64_MIN marks a
 * step outside [min_quant, 255]), and d_totlast[nframes][2][64][2] (population, highest occupied
 * bin + 1).  Integer sums: exactly what the reference's double accumulators hold.  quant / min_quant
 * are host arrays (min_quant NULL = ones).  sjpeg_hip_adapt_quant_sums() is the float half on the
 * host (regression, lambda, choice of the step) for ONE frame's sums; it updates quant and tables
 * like sjpeg_hip_adapt_quant(). */
int sjpeg_hip_adapt_sums(const uint32_t* d_hist, int nframes, const uint8_t quant[2][64],
                         const uint8_t* min_quant /*[2][64]*/, int64_t* d_sums, int32_t* d_totlast,
                         void* stream);
void sjpeg_hip_adapt_quant_sums(const int64_t* sums, const int32_t* totlast, int yuv_mode,
                                uint8_t quant[2][64], const uint8_t* min_quant /*[2][64]*/, int q_bias,
                                int qdelta_max_luma, int qdelta_max_chroma,
                                sjpeg_hip_scan_tables* tables);
/* ... and the float half on the DEVICE too, behind sjpeg_hip_adapt_sums() on the same stream (src/histogram.cc:169-312:
 * the two-cloud line fit per position over the candidate steps, lambda from the slopes summed over the live positions
 * in ascending order, the choice of a step per position -- every expression and accumulation in the reference's order,
 * IEEE double, no contraction: the result is the host's, bit for bit): d_quant_out[nframes][2][64] = the adapted
 * matrices (4:0:0: table 0 only is written).  quant = the starting matrices the sums were made for (host array);
 * sjpeg_hip_finalize_quant() turns a frame's result into its tables.  What sjpeg_hip_encode_batch_src runs: 128 bytes a
 * frame come back from the device instead of 52 KB, and no regression on the host sits between two device passes. */
int sjpeg_hip_adapt_decide(const int64_t* d_sums, const int32_t* d_totlast, int nframes, const uint8_t quant[2][64],
                           int yuv_mode, int qdelta_max_luma, int qdelta_max_chroma, uint8_t* d_quant_out, void* stream);

/* CompileEntropyStats / BuildOptimalTable (src/entropy.cc:254-444) on ONE frame's symbol
 * statistics (host memory, uint32 [2][272]): fills specs[4] = {DC luma, DC chroma, AC luma,
 * AC chroma} (chroma untouched for 4:0:0) and installs their codes into `tables`. */
void sjpeg_hip_optimize_huffman(const uint32_t* freq, int yuv_mode,
                                sjpeg_hip_huffman_spec specs[4], sjpeg_hip_scan_tables* tables);

/* sjpeg_hip_make_header with explicit Huffman tables (specs as above; NULL = Annex K defaults). */
size_t sjpeg_hip_make_header_ex(int width, int height, int yuv_mode, const uint8_t quant[2][64],
                                const sjpeg_hip_huffman_spec* specs, uint8_t* buf, size_t cap);

/* The same with the metadata segments of the reference's EncoderParam (src/sjpeg.h:258-266) in
 * front of the tables, in its order: raw application markers (verbatim), EXIF (one APP1), ICC
 * profile (numbered APP2 chunks), XMP (one APP1, or main packet + extension chunks tied by the
 * MD5 of the extension when it exceeds 64 KiB): src/headers.cc:63-180.  Returns 0 on invalid
 * metadata (EXIF > 64 KiB, ICC >= 256 chunks, malformed extended XMP) or if cap is too small. */
typedef struct sjpeg_hip_metadata {
  const void* app_markers; size_t app_markers_size;
  const void* exif;        size_t exif_size;
  const void* iccp;        size_t iccp_size;
  const void* xmp;         size_t xmp_size;
  uint16_t xmp_split_point;                     /* 0 = default split of a long XMP packet */
} sjpeg_hip_metadata;
size_t sjpeg_hip_make_header_meta(int width, int height, int yuv_mode, const uint8_t quant[2][64],
                                  const sjpeg_hip_huffman_spec* specs,
                                  const sjpeg_hip_metadata* meta, uint8_t* buf, size_t cap);

/* Restart mode (SJPEG_HIP_RESTART_MARKERS): MCUs per restart interval for a colour mode (41 / 82 / 246),
 * and the DRI segment (FF DD 00 04 Ri) inserted in front of the SOS segment of a header made by any of
 * the builders above (in place; returns the new size, 0 if cap < size + 6 or no SOS is found). */
int sjpeg_hip_restart_interval(int yuv_mode);
size_t sjpeg_hip_header_add_restart(uint8_t* header, size_t size, size_t cap, int yuv_mode);

/* Restart mode, one frame over several devices: codes the restart intervals [seg_begin, seg_end) of the
 * frame (segments as counted by sjpeg_hip_segment_count()) into d_out: stuffed entropy bytes, RSTn
 * between the intervals AND behind the last one unless it is the frame's last; no header, no EOI.
 * Intervals are byte aligned and self-contained, so the file is
 *   header with DRI | bytes of band 0 | bytes of band 1 | ... | FF D9
 * put together by plain concatenation (host or device) in band order -- the "segmented at restart
 * markers, gathered, concatenated" form; bit-identical to the one-device restart-mode stream.
 * tables->flags must carry SJPEG_HIP_RESTART_MARKERS.  A band that does not fit out_cap reports size 0. */
int sjpeg_hip_encode_intervals_src(sjpeg_hip_engine* engine, const sjpeg_hip_source* src, int width, int height,
                                   int yuv_mode, const sjpeg_hip_scan_tables* tables, int seg_begin, int seg_end,
                                   void* d_out, size_t out_cap, uint64_t* d_size, void* stream);

/* Exchange step of the multi-device batch path (BASELINE.json config #4; the reference runs on one
 * thread and has no counterpart): packs the `nframes` coded streams an encode call left at
 * d_out + f*out_stride / d_sizes[f] back to back into d_packed, so that ONE collective (RCCL gather over
 * xGMI) or one copy moves them.  Frame f starts at d_offsets[f], a multiple of 16 (the up to 15 bytes
 * of padding behind a frame are zero); d_offsets[nframes] & ~SJPEG_HIP_PACKED_OVERFLOW is the number of
 * bytes the batch needs, and bit 63 (SJPEG_HIP_PACKED_OVERFLOW) is set when that is more than
 * packed_capacity -- a frame that would end behind the capacity is not copied.  The exchange below reads the
 * flag in the rank's row: every rank then returns SJPEG_HIP_ECAPACITY before anything is sent.  One launch on
 * `stream`, no host synchronisation.  d_out, d_packed and out_stride must be multiples of 16.
 * (sjpeg_hip_encode_scan_packed_src() writes this layout directly and needs no second pass.) */
#define SJPEG_HIP_PACKED_OVERFLOW (1ull << 63)
int sjpeg_hip_compact_streams(const void* d_out, size_t out_stride, const uint64_t* d_sizes, int nframes,
                              void* d_packed, size_t packed_capacity, uint64_t* d_offsets /* nframes + 1 */,
                              void* stream);

/* The exchange itself, for a C / C++ caller with one process per GPU: gathers the packed streams of every
 * rank (what sjpeg_hip_compact_streams left in d_packed / d_offsets) into the root's d_gathered over RCCL
 * (xGMI inside a node).  RCCL is resolved at run time (librccl.so.1: the copy already loaded in the
 * process, e.g. PyTorch's, else the one the loader finds, else /opt/rocm/lib): a process that never
 * gathers never loads it.
 *
 * A communicator is either created here -- rank 0 calls sjpeg_hip_comm_unique_id() and hands the 128 bytes
 * to the other ranks by whatever means the application has (MPI, a socket, torch.distributed's store),
 * then every rank calls sjpeg_hip_comm_create() with its device current -- or adopted from an ncclComm_t
 * the application already owns (sjpeg_hip_comm_adopt; not destroyed with the wrapper).
 *
 * sjpeg_hip_gather_streams(), called by every rank with the same frames_per_rank_max, root and
 * gathered_capacity:
 *   1. one ncclAllGather of a row of frames_per_rank_max + 2 uint64 per rank: the rank's packed bytes
 *      (d_offsets[nframes_local], a multiple of 16), its number of frames and its frame sizes (d_sizes,
 *      zero beyond nframes_local) -> d_rows [world][frames_per_rank_max + 2] on every rank;
 *   2. ONE small device-to-host read per rank and call: the rows (8 x world x (frames_per_rank_max + 2)
 *      bytes) -> h_rows, because RCCL's send / receive counts are host values; no per-frame
 *      synchronisation;
 *   3. grouped ncclSend / ncclRecv of EXACT lengths (no padding to the largest rank; RCCL has no
 *      gatherv): rank r's bytes land at d_gathered + h_rank_offsets[r] on the root, in rank order, the
 *      root's own by a device copy.
 * h_rows (host, [world][frames_per_rank_max + 2]) and h_rank_offsets (host, [world + 1]) are filled on
 * every rank; frame k of rank r is at h_rank_offsets[r] + the sum of the 16-aligned sizes of the rank's
 * earlier frames.  Every rank sees the same rows and therefore takes the same decision: a frame of size
 * 0 among the frames of some rank (it did not fit its slot), a rank whose d_offsets[nframes] carries
 * SJPEG_HIP_PACKED_OVERFLOW (its d_packed was too small: size it for nframes x out_stride) or is not the sum
 * of its frames, or a total above gathered_capacity, makes the call return SJPEG_HIP_ECAPACITY on EVERY rank
 * before anything is sent (never a hang).
 * d_gathered is only used on the root.  Everything is enqueued on `stream`; the host read waits for that
 * stream, the byte transfers do not.  Returns 0 or SJPEG_HIP_E*. */
typedef struct sjpeg_hip_comm sjpeg_hip_comm;
#define SJPEG_HIP_COMM_ID_BYTES 128
int sjpeg_hip_comm_unique_id(uint8_t id[SJPEG_HIP_COMM_ID_BYTES]);
int sjpeg_hip_comm_create(const uint8_t id[SJPEG_HIP_COMM_ID_BYTES], int rank, int world, sjpeg_hip_comm** comm);
int sjpeg_hip_comm_adopt(void* nccl_comm /* ncclComm_t */, sjpeg_hip_comm** comm);
/* A communicator on the LOCAL transport: its ranks are threads of ONE process (a server that drives the
 * GPUs of a node from one thread each, or several engines on one GPU), no RCCL in the process.  `id`: any
 * 128 bytes the application picks, the same on every rank of the group; every rank calls this once, with
 * the device it works on current.  The gather functions below are the same code on either transport; here
 * a transfer is a copy on the receiver's stream (a peer copy between devices), ordered behind the sender's
 * stream by an event and the sender's stream behind the copy by another -- the calls of a matched pair meet
 * on the host, so a send returns once its receive has been enqueued, and a rank that does not show up within
 * 60 s makes the call fail with SJPEG_HIP_ERUNTIME on the ranks that wait for it (never a hang). */
int sjpeg_hip_comm_create_local(const uint8_t id[SJPEG_HIP_COMM_ID_BYTES], int rank, int world,
                                sjpeg_hip_comm** comm);
void sjpeg_hip_comm_destroy(sjpeg_hip_comm* comm);
int sjpeg_hip_comm_rank(const sjpeg_hip_comm* comm);
int sjpeg_hip_comm_world(const sjpeg_hip_comm* comm);
/* The two halves of sjpeg_hip_gather_streams() for a root that sizes its buffer from the ACTUAL total:
 * steps 1-2 (every rank; h_rank_offsets[world] = bytes the root will receive; SJPEG_HIP_ECAPACITY on every
 * rank for a frame of size 0 or an overflowed d_packed), then step 3 (every rank).  Step 3 checks the ROOT's own
 * arguments on the root only (d_gathered NULL, gathered_capacity below the total it was just told, d_packed NULL):
 * the peers have queued their sends by then, so such an error leaves them unmatched and the communicator must
 * be destroyed -- size the buffer from h_rank_offsets[world] first (sjpeg_hip_gather_streams(), which knows the
 * capacity on every rank, refuses before anybody sends).  A root whose d_packed IS d_gathered +
 * h_rank_offsets[root] (it coded straight into place with sjpeg_hip_encode_scan_packed_src) copies nothing. */
int sjpeg_hip_gather_rows(sjpeg_hip_comm* comm, const uint64_t* d_offsets, const uint64_t* d_sizes, int nframes_local,
                          int frames_per_rank_max, uint64_t* d_rows, uint64_t* h_rows, uint64_t* h_rank_offsets,
                          void* stream);
int sjpeg_hip_gather_bytes(sjpeg_hip_comm* comm, int root, const void* d_packed, int frames_per_rank_max,
                           const uint64_t* h_rows, const uint64_t* h_rank_offsets, void* d_gathered,
                           size_t gathered_capacity, void* stream);
int sjpeg_hip_gather_streams(sjpeg_hip_comm* comm, int root, const void* d_packed, const uint64_t* d_offsets,
                             const uint64_t* d_sizes, int nframes_local, int frames_per_rank_max,
                             uint64_t* d_rows /* [world + 1][frames_per_rank_max + 2]: the last row is scratch */,
                             void* d_gathered, size_t gathered_capacity,
                             uint64_t* h_rows, uint64_t* h_rank_offsets /* [world + 1] */, void* stream);

/* Duration in milliseconds of the dominant kernel (the fused colour+fDCT+quant+entropy
 * kernel) in the most recent sjpeg_hip_encode_scan() call on this engine, measured with
 * HIP events on the caller's stream.  Timing is recorded only after
 * sjpeg_hip_engine_set_timing(engine, 1).  Negative if unavailable.  Synchronises. */
int sjpeg_hip_engine_set_timing(sjpeg_hip_engine* engine, int enable);
float sjpeg_hip_engine_last_scan_ms(sjpeg_hip_engine* engine);
float sjpeg_hip_engine_last_total_ms(sjpeg_hip_engine* engine);

/* Device memory the engine currently holds (it grows to what the largest call needed and is released
 * by sjpeg_hip_engine_trim / sjpeg_hip_engine_destroy).  The segment scratch of an encode call is sized from the caller's
 * out_stride: per frame about 3.5 x out_stride (segment slots + pool + the un-stuffed stream), capped at
 * the worst case of the geometry -- not the worst case itself. */
size_t sjpeg_hip_engine_scratch_bytes(sjpeg_hip_engine* engine);

/* Gives the engine's scratch back to the device (waits for the device's work first; tables and header
 * buffer included).  The next call allocates what it needs again -- for a service that has just coded
 * an unusually large frame or batch and does not want to keep its high-water mark. */
int sjpeg_hip_engine_trim(sjpeg_hip_engine* engine);

/* The host API (include/sjpeg.h) keeps one device context per calling thread: pixel, stream and plane
 * buffers plus an engine, grown on demand.  A context whose cached device memory exceeds
 * SJPEG_HIP_HOST_CACHE_BYTES (environment, default 1 GiB) after a call that itself needed less than
 * half of it releases it before returning (a steady stream of frames that need more than the limit
 * keeps its buffers: set the limit to what the service may hold, not below what one frame needs);
 * sjpeg_hip_host_trim() releases the calling thread's cache now and returns the bytes it held.
 * The host API first codes against an output capacity of half a byte per sample (0.75 B per pixel in
 * 4:2:0) and repeats the frame against sjpeg_hip_frame_bound() if that was too small
 * (SJPEG_HIP_HOST_FIRST_CAPACITY=bound: worst case from the first pass). */
size_t sjpeg_hip_host_trim(void);

/* Measurement aids of bench.py (no counterpart in the reference, not part of the encode path).
 * sjpeg_hip_debug_stream_read: a read-only streaming kernel over `bytes` of d_buf -- what the device's
 * HBM delivers to the simplest possible reader, beside the 8 TB/s specification figure.
 * sjpeg_hip_debug_valu_rate: cycles (at the nominal 2.4 GHz) a wave64 VALU instruction occupies a SIMD
 * at 8 waves per SIMD, for the two issue classes found on gfx950: cycles[0] = v_perm_b32 (every VOP3,
 * packed, multiply, dot and permute instruction), cycles[1] = v_add_u32 (simple 32-bit integer and
 * f32 instructions).  Synchronises on `stream`. */
int sjpeg_hip_debug_stream_read(const void* d_buf, size_t bytes, uint32_t* d_sink, void* stream);
int sjpeg_hip_debug_valu_rate(float cycles[2], void* stream);
/* sjpeg_hip_debug_shader_clock: the shader clock in MHz as a wave on `stream` measures it (cycle counter against the
 * device-wide 100 MHz counter over 20 us), i.e. the clock of the work that was just queued there.  Synchronises. */
int sjpeg_hip_debug_shader_clock(float* mhz, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* SJPEG_HIP_H_ */
