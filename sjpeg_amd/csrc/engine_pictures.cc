// engine_pictures.cc -- the engine's half of the entries that MAKE pictures for a ragged call: reduction, resize, the
// YUV-plane resize, contact sheets, the video colour conversion, the unsharp mask, Pillow's filters and the compose
// stage.  The plans come from the *_plan.cc files, the kernels and their launch functions live in reduce.hip,
// resize.hip, yuv_colour.hip, unsharp.hip, pillow_filter.hip and compose.hip (ragged_aux.h); here the call is ordered
// behind the engine's earlier work, the engine's memory is sized and the descriptors go up.  Host only.
#include "engine.h"

using namespace sjpeg_internal;

// ---- ragged reduction and resize (reduce.hip, resize.hip).  The two share the engine's memory for the pictures they
// make and for their descriptors; `launch` starts the kernel over the uploaded descriptors.
template <class Frame>
static void picture_rebase(Frame& d, uint8_t* base) { d.dst = base + reinterpret_cast<uintptr_t>(d.dst); }
static void picture_rebase(sjpeg_internal::ResampleBoxFrame& d, uint8_t* base) { d.r.dst = base + reinterpret_cast<uintptr_t>(d.r.dst); }
static void picture_rebase(sjpeg_internal::YuvPlane& p, uint8_t* base) {
  p.r.dst = base + reinterpret_cast<uintptr_t>(p.r.dst);
  if (p.channels == 2) p.dst2 = base + reinterpret_cast<uintptr_t>(p.dst2);
}

template <class Frame, class Launch>
static int engine_make_pictures(sjpeg_hip_engine* e, const std::string& who, const char* what, std::vector<Frame> desc, size_t bytes,
                                uint8_t* d_pictures, uint8_t** base, void* stream, Launch launch) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = ragged_ordered(e, st)) return rc;
  if (d_pictures == nullptr) {
    if (e->reduced.ensure(bytes / 16 + 1) != 0) {
      return fail(SJPEG_HIP_ENOMEM, who + ": no device memory for " + std::to_string(bytes) + " bytes of " + what + " pictures");
    }
    d_pictures = reinterpret_cast<uint8_t*>(e->reduced.p);
  }
  if (base != nullptr) *base = d_pictures;
  for (Frame& d : desc) picture_rebase(d, d_pictures);
  const size_t desc_bytes = sizeof(Frame) * desc.size();
  if (int rc = e->reduce_desc.ensure(desc_bytes / 16 + 1)) return rc;
  if (int rc = upload(e, e->reduce_desc.p, desc.data(), desc_bytes, st)) return rc;
  if (int rc = sync_uploads(e, st)) return rc;
  return launch(reinterpret_cast<const Frame*>(e->reduce_desc.p), static_cast<int>(desc.size()), st);
}

int sjpeg_internal::engine_reduce(sjpeg_hip_engine* e, const std::string& who, const ReducePlan& plan, uint8_t* d_reduced, uint8_t** base,
                                  void* stream) {
  return engine_make_pictures(e, who, "reduced", plan.frames, plan.bytes, d_reduced, base, stream,
                              [&](const ReduceFrame* d_frames, int n, hipStream_t st) {
    if (reduce_ragged_launch(plan.format, e->pscale, e->pbias, d_frames, n, plan.tiles, st) != 0) {
      return fail(SJPEG_HIP_ERUNTIME, who + ": reduce_ragged_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
    }
    return 0;
  });
}

int sjpeg_internal::engine_resize(sjpeg_hip_engine* e, const std::string& who, const ResizePlan& plan, uint8_t* d_resized, uint8_t** base,
                                  void* stream) {
  return engine_make_pictures(e, who, "resized", plan.frames, plan.bytes, d_resized, base, stream,
                              [&](const ResizeFrame* d_frames, int n, hipStream_t st) {
    const int rc = plan.light != SJPEG_HIP_LIGHT_CODED
                       ? resize_ragged_linear_launch(false, plan.format, e->pscale, e->pbias, plan.flat ? &plan.flatten : nullptr, d_frames, n,
                                                     plan.tiles, st)
                   : plan.flat ? resize_ragged_flat_launch(false, plan.format, e->pscale, e->pbias, plan.flatten, d_frames, n, plan.tiles, st)
                               : resize_ragged_launch(plan.format, e->pscale, e->pbias, d_frames, n, plan.tiles, st);
    if (rc != 0) {
      return fail(SJPEG_HIP_ERUNTIME, who + ": resize_ragged_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
    }
    return 0;
  });
}

// ... and of resampling with Pillow's filters (resample_plan.cc, resample.hip): the call's tables into engine memory of
// their own, the descriptors' table pointers rebased to it, then as the two above
int sjpeg_internal::engine_resample(sjpeg_hip_engine* e, const std::string& who, const ResamplePlan& plan, uint8_t* d_out, uint8_t** base,
                                    void* stream) {
  hipStream_t st0 = static_cast<hipStream_t>(stream);
  if (int rc = ragged_ordered(e, st0)) return rc;
  const size_t table_bytes = plan.tables.size() * sizeof(int32_t);
  if (e->resample_tables.ensure(table_bytes / 16 + 1) != 0) {
    return fail(SJPEG_HIP_ENOMEM, who + ": no device memory for " + std::to_string(table_bytes) + " bytes of resampling tables");
  }
  if (int rc = upload(e, e->resample_tables.p, plan.tables.data(), table_bytes, st0)) return rc;
  std::vector<ResampleFrame> desc = plan.frames;
  const uint8_t* const tables = reinterpret_cast<const uint8_t*>(e->resample_tables.p);
  for (ResampleFrame& d : desc) {
    d.xb = reinterpret_cast<const int32_t*>(tables + reinterpret_cast<uintptr_t>(d.xb));
    d.xk = reinterpret_cast<const int32_t*>(tables + reinterpret_cast<uintptr_t>(d.xk));
    d.yb = reinterpret_cast<const int32_t*>(tables + reinterpret_cast<uintptr_t>(d.yb));
    d.yk = reinterpret_cast<const int32_t*>(tables + reinterpret_cast<uintptr_t>(d.yk));
  }
  if (!plan.stages.empty()) {
    // a box call with a reduced frame: every frame with its stage, through the kernel that reduces as it stages
    std::vector<ResampleBoxFrame> boxed(desc.size());
    for (size_t f = 0; f < desc.size(); ++f) { boxed[f].r = desc[f]; boxed[f].s = plan.stages[f]; }
    return engine_make_pictures(e, who, "resampled", std::move(boxed), plan.bytes, d_out, base, stream,
                                [&](const ResampleBoxFrame* d_frames, int n, hipStream_t st) {
      if (resample_box_launch(plan.format, e->pscale, e->pbias, plan.flat ? &plan.flatten : nullptr, d_frames, n, plan.tiles, st) != 0) {
        return fail(SJPEG_HIP_ERUNTIME, who + ": resample_box_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
      }
      return 0;
    });
  }
  return engine_make_pictures(e, who, "resampled", std::move(desc), plan.bytes, d_out, base, stream,
                              [&](const ResampleFrame* d_frames, int n, hipStream_t st) {
    if (resample_launch(plan.format, e->pscale, e->pbias, plan.flat ? &plan.flatten : nullptr, d_frames, n, plan.tiles, st) != 0) {
      return fail(SJPEG_HIP_ERUNTIME, who + ": resample_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
    }
    return 0;
  });
}

// ... and of the YUV-plane formats: a descriptor per plane, the kernel's other instantiation
int sjpeg_internal::engine_yuv_resize(sjpeg_hip_engine* e, const std::string& who, const YuvResizePlan& plan, uint8_t* d_out, uint8_t** base,
                                      void* stream) {
  return engine_make_pictures(e, who, "resized", plan.planes, plan.bytes, d_out, base, stream,
                              [&](const YuvPlane* d_planes, int n, hipStream_t st) {
    if ((plan.deep ? yuv_resize_ragged_deep_launch(false, plan.shift, d_planes, n, plan.tiles, st)
                   : yuv_resize_ragged_launch(d_planes, n, plan.tiles, st)) != 0) {
      return fail(SJPEG_HIP_ERUNTIME, who + ": resize_ragged_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
    }
    return 0;
  });
}

// ... and of the contact sheets (sheet_plan.cc): the background of every sheet, then the placed descriptors of either
// plan, both on the call's stream -- stream order is the only ordering relied on
int sjpeg_internal::engine_sheet(sjpeg_hip_engine* e, const std::string& who, const SheetPlan& plan, uint8_t* d_out, uint8_t** base,
                                 void* stream) {
  uint8_t* sheets = nullptr;
  auto fill = [&](hipStream_t st) {
    if (sheet_fill_launch(plan.fill, sheets, st) != 0) {
      return fail(SJPEG_HIP_ERUNTIME, who + ": sheet_fill_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
    }
    return 0;
  };
  int rc;
  if (plan.yuv) {
    rc = engine_make_pictures(e, who, "sheet", plan.planes.planes, plan.bytes, d_out, &sheets, stream,
                              [&](const YuvPlane* d_planes, int n, hipStream_t st) {
      if (int rcf = fill(st)) return rcf;
      if ((plan.planes.deep ? yuv_resize_ragged_deep_launch(true, plan.planes.shift, d_planes, n, plan.planes.tiles, st)
                            : yuv_resize_ragged_placed_launch(d_planes, n, plan.planes.tiles, st)) != 0) {
        return fail(SJPEG_HIP_ERUNTIME, who + ": resize_ragged_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
      }
      return 0;
    });
  } else {
    rc = engine_make_pictures(e, who, "sheet", plan.rgb.frames, plan.bytes, d_out, &sheets, stream,
                              [&](const ResizeFrame* d_frames, int n, hipStream_t st) {
      if (int rcf = fill(st)) return rcf;
      const int rcl = plan.rgb.light != SJPEG_HIP_LIGHT_CODED
                          ? resize_ragged_linear_launch(true, plan.format, e->pscale, e->pbias, plan.rgb.flat ? &plan.rgb.flatten : nullptr, d_frames,
                                                        n, plan.rgb.tiles, st)
                      : plan.rgb.flat ? resize_ragged_flat_launch(true, plan.format, e->pscale, e->pbias, plan.rgb.flatten, d_frames, n, plan.rgb.tiles, st)
                                      : resize_ragged_placed_launch(plan.format, e->pscale, e->pbias, d_frames, n, plan.rgb.tiles, st);
      if (rcl != 0) {
        return fail(SJPEG_HIP_ERUNTIME, who + ": resize_ragged_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
      }
      return 0;
    });
  }
  if (base != nullptr) *base = sheets;
  return rc;
}

// ... and of the video colour conversion (yuv_colour_plan.cc): the launch behind the resize launch of the same call, on
// the same stream, over the planes that one made at `base`
int sjpeg_internal::engine_yuv_colour(sjpeg_hip_engine* e, const std::string& who, const YuvColourPlan& plan, uint8_t* base, void* stream) {
  if (plan.tiles == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<YuvColourFrame> desc = plan.frames;
  for (YuvColourFrame& d : desc) {
    d.y = base + reinterpret_cast<uintptr_t>(d.y);
    d.u = base + reinterpret_cast<uintptr_t>(d.u);
    d.v = base + reinterpret_cast<uintptr_t>(d.v);
  }
  const size_t desc_bytes = sizeof(YuvColourFrame) * desc.size();
  if (int rc = e->colour_desc.ensure(desc_bytes / 16 + 1)) return rc;
  if (int rc = upload(e, e->colour_desc.p, desc.data(), desc_bytes, st)) return rc;
  if (int rc = sync_uploads(e, st)) return rc;
  if (yuv_colour_launch(plan.placed, reinterpret_cast<const YuvColourFrame*>(e->colour_desc.p), static_cast<int>(desc.size()), plan.tiles, st) != 0) {
    return fail(SJPEG_HIP_ERUNTIME, who + ": yuv_colour_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
  }
  return 0;
}

// ... and of the unsharp mask (unsharp_plan.cc): the launch behind the launches that made the pictures at src_base, on
// the same stream, out of place.  Both buffers are sized before a pointer into either is taken.
int sjpeg_internal::engine_unsharp(sjpeg_hip_engine* e, const std::string& who, const UnsharpPlan& plan, const uint8_t* src_base, uint8_t* d_out,
                                   uint8_t** base, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<UnsharpPlane> desc = plan.planes;
  const size_t desc_bytes = sizeof(UnsharpPlane) * desc.size();
  if (d_out == nullptr) {
    if (e->final_pictures.ensure(plan.bytes / 16 + 1) != 0) {
      return fail(SJPEG_HIP_ENOMEM, who + ": no device memory for " + std::to_string(plan.bytes) + " bytes of sharpened pictures");
    }
  }
  if (int rc = e->unsharp_desc.ensure(desc_bytes / 16 + 1)) return rc;
  if (d_out == nullptr) d_out = reinterpret_cast<uint8_t*>(e->final_pictures.p);
  if (base != nullptr) *base = d_out;
  for (UnsharpPlane& d : desc) {
    d.src = src_base + reinterpret_cast<uintptr_t>(d.src);
    d.dst = d_out + reinterpret_cast<uintptr_t>(d.dst);
  }
  if (plan.tiles == 0) return 0;
  if (int rc = upload(e, e->unsharp_desc.p, desc.data(), desc_bytes, st)) return rc;
  if (int rc = sync_uploads(e, st)) return rc;
  if (unsharp_launch(reinterpret_cast<const UnsharpPlane*>(e->unsharp_desc.p), static_cast<int>(desc.size()), plan.tiles, st) != 0) {
    return fail(SJPEG_HIP_ERUNTIME, who + ": unsharp_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
  }
  return 0;
}

// ... and of Pillow's filters (pillow_filter_plan.cc): the two launches behind the launch that made the pictures at
// src_base, on the same stream -- along the rows into the engine's scratch of the same layout, along the columns from
// there out of place.  Every buffer is sized before a pointer into any is taken.
int sjpeg_internal::engine_pillow_filter(sjpeg_hip_engine* e, const std::string& who, const PillowFilterPlan& plan, const uint8_t* src_base,
                                         uint8_t* d_out, uint8_t** base, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<PillowFilterPlane> desc = plan.planes;
  const size_t desc_bytes = sizeof(PillowFilterPlane) * desc.size();
  if ((d_out == nullptr && e->final_pictures.ensure(plan.bytes / 16 + 1) != 0) || e->filter_mid.ensure(plan.bytes / 16 + 1) != 0) {
    return fail(SJPEG_HIP_ENOMEM, who + ": no device memory for " + std::to_string(plan.bytes) + " bytes of filtered pictures");
  }
  if (int rc = e->filter_desc.ensure(desc_bytes / 16 + 1)) return rc;
  if (d_out == nullptr) d_out = reinterpret_cast<uint8_t*>(e->final_pictures.p);
  if (base != nullptr) *base = d_out;
  uint8_t* const mid = reinterpret_cast<uint8_t*>(e->filter_mid.p);
  for (PillowFilterPlane& d : desc) {
    d.made = src_base + reinterpret_cast<uintptr_t>(d.made);
    d.mid = mid + reinterpret_cast<uintptr_t>(d.mid);
    d.dst = d_out + reinterpret_cast<uintptr_t>(d.dst);
  }
  if (plan.tiles[0] == 0 || plan.tiles[1] == 0) return 0;
  if (int rc = upload(e, e->filter_desc.p, desc.data(), desc_bytes, st)) return rc;
  if (int rc = sync_uploads(e, st)) return rc;
  for (int launch = 0; launch < 2; ++launch) {
    if (pillow_filter_launch(launch, reinterpret_cast<const PillowFilterPlane*>(e->filter_desc.p), static_cast<int>(desc.size()), plan.tiles[launch],
                             st) != 0) {
      return fail(SJPEG_HIP_ERUNTIME, who + ": pillow_filter_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
    }
  }
  return 0;
}

// ... and of the compose stage (compose_plan.cc): the one launch behind the launches that made the pictures at
// src_base, on the same stream, into the caller's buffer or the engine's memory for composed pictures -- never where
// the made pictures stand.  Every buffer is sized before a pointer into any is taken.
int sjpeg_internal::engine_compose(sjpeg_hip_engine* e, const std::string& who, const ComposePlan& plan, const uint8_t* src_base, uint8_t* d_out,
                                   uint8_t** base, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<ComposeFrame> desc = plan.frames;
  const size_t desc_bytes = sizeof(ComposeFrame) * desc.size();
  if (d_out == nullptr && e->composed.ensure(plan.bytes / 16 + 1) != 0) {
    return fail(SJPEG_HIP_ENOMEM, who + ": no device memory for " + std::to_string(plan.bytes) + " bytes of composed pictures");
  }
  if (int rc = e->compose_desc.ensure(desc_bytes / 16 + 1)) return rc;
  if (d_out == nullptr) d_out = reinterpret_cast<uint8_t*>(e->composed.p);
  if (base != nullptr) *base = d_out;
  for (ComposeFrame& d : desc) {
    d.made = src_base + reinterpret_cast<uintptr_t>(d.made);
    d.dst = d_out + reinterpret_cast<uintptr_t>(d.dst);
  }
  if (plan.tiles == 0) return 0;
  if (int rc = upload(e, e->compose_desc.p, desc.data(), desc_bytes, st)) return rc;
  if (int rc = sync_uploads(e, st)) return rc;
  if (compose_launch(reinterpret_cast<const ComposeFrame*>(e->compose_desc.p), static_cast<int>(desc.size()), plan.tiles, st) != 0) {
    return fail(SJPEG_HIP_ERUNTIME, who + ": compose_kernel launch failed: " + hipGetErrorString(hipGetLastError()));
  }
  return 0;
}
