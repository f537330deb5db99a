// ref_param_meta_shim.cc -- TEST INFRASTRUCTURE ONLY (tests/golden/make_ragged_meta.py builds it into oracle/_ref/, which
// is out of git).  The reference's public sjpeg::Encode() with every EncoderParam field a ragged batch call describes at
// once: sampling, method flags, the search AND the metadata.  (oracle/ref_shim.cc offers the metadata with method 0 only
// and the search without metadata.)  Links against oracle/_ref/libsjpeg_ref.so.
#include <stddef.h>
#include <stdint.h>

#include "sjpeg.h"

extern "C" {

// target_mode: 0 none, 1 size (bytes), 2 PSNR (dB).  Returns the size; *out is freed with ref_pm_free.
size_t ref_pm_encode(const uint8_t* rgb, int w, int h, int stride, float quality, int yuv_mode, int huffman, int adaptive,
                     int trellis, int target_mode, float target_value, int passes, float tolerance, float qmin, float qmax,
                     const char* app, size_t app_size, const char* exif, size_t exif_size, const char* iccp,
                     size_t iccp_size, const char* xmp, size_t xmp_size, int xmp_split, uint8_t** out) {
  sjpeg::EncoderParam param(quality);
  param.yuv_mode = static_cast<SjpegYUVMode>(yuv_mode);
  param.Huffman_compress = (huffman != 0);
  param.adaptive_quantization = (adaptive != 0);
  param.use_trellis = (trellis != 0);
  param.target_mode = static_cast<sjpeg::EncoderParam::TargetMode>(target_mode);
  param.target_value = target_value;
  param.passes = passes;
  param.tolerance = tolerance;
  param.qmin = qmin;
  param.qmax = qmax;
  if (app != nullptr) param.app_markers.assign(app, app_size);
  if (exif != nullptr) param.exif.assign(exif, exif_size);
  if (iccp != nullptr) param.iccp.assign(iccp, iccp_size);
  if (xmp != nullptr) param.xmp.assign(xmp, xmp_size);
  param.xmp_split_point = static_cast<uint16_t>(xmp_split);
  return sjpeg::Encode(rgb, w, h, stride, param, out);
}

void ref_pm_free(uint8_t* p) { SjpegFreeBuffer(p); }

}  // extern "C"
