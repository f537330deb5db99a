"""The argument types of every exported C entry, stated once and in the header's order (include/sjpeg.h,
include/sjpeg_hip.h), and the layout of a shaped ragged call.  sjpeg_amd.lib() applies TABLE to the library when it
loads it; nothing else in the package sets a restype or an argument list.

The shaped ragged entries are not written out: each is a row of piece names -- the common head, `params` where the
entry encodes, the family's own segments, one tail -- and PIECES says what slots a piece takes.  layout() puts a call's
values, given by piece name, into the row's order.  A new family is a line in _rows() below."""
import ctypes as C

from sjpeg_amd import HuffmanSpec, RaggedFrame, RaggedParams, ScanTables, SearchParams, Source, _u8p

I, P, Z, F, D, I64 = C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_double, C.c_int64
_ip, _fp, _frames, _tables, _src = C.POINTER(I), C.POINTER(F), C.POINTER(RaggedFrame), C.POINTER(ScanTables), C.POINTER(Source)

# piece -> the types of its slots.  A piece of one slot takes its value as it is, a longer one a tuple.
PIECES = {
    "head": [P, I, I, _frames],                  # engine, format, nframes, frames
    "bytes_head": [I, I, _frames],               # (the _bytes entries take no engine)
    "params": [C.POINTER(RaggedParams)],
    # the segments, by the name of their (first) parameter in the header; the second slot is a count or a per-frame flag
    "factors": [P], "sizes": [P], "orientations": [P], "flatten": [P], "light": [I], "sheet": [P], "depth": [P],
    "colour": [P, I], "unsharp": [P, I], "resample": [P, I], "box": [P, I], "filter": [P, I], "compose": [P, I],
    "overlays": [P, I], "places": [P, I], "meta": [P, I],
    # the tails
    "pictures": [P, Z, _frames, _ip, P],         # d_out, bytes, out_frames, out_format, stream
    "sheets": [P, Z, _frames, _ip, _ip, P],      # ... out_frames, nsheets, out_format, stream
    "unpacked": [P, P, _ip, _fp, _fp, P],        # d_out, d_sizes, modes, q_out, value_out, stream
    "packed": [P, Z, P, P, _ip, _fp, _fp, P],    # d_packed, packed_capacity, d_offsets, d_sizes, modes, ...
    "strided": [P, Z, P, _ip, _fp, _fp, P],      # d_out, out_stride, d_sizes, modes, ... (the unpacked sheet encodes)
}

_SHAPE = ("sizes", "orientations")
_FLAT = ("flatten",) + _SHAPE
_RESAMPLED = _FLAT + ("resample",)
_COMPOSED = _RESAMPLED + ("box", "filter", "compose", "overlays", "places")
# stem -> segments: sjpeg_hip_<stem>_src makes pictures
_MAKERS = {
    "reduce_ragged": ("factors",), "resize_ragged": ("sizes",), "orient_ragged": _SHAPE, "resize_ragged_yuv": _SHAPE,
    "flatten_ragged": _FLAT, "linear_ragged": ("flatten", "light") + _SHAPE,
    "unsharp_ragged": ("flatten", "light") + _SHAPE + ("unsharp",),
    "resample_ragged": _RESAMPLED + ("unsharp",), "resample_box_ragged": _RESAMPLED + ("box", "unsharp"),
    "filter_ragged": _RESAMPLED + ("box", "filter"), "compose_ragged": _COMPOSED,
    "convert_ragged_yuv": _SHAPE + ("colour",), "convert_ragged_yuv16": _SHAPE + ("colour", "depth"),
    "unsharp_ragged_yuv": _SHAPE + ("colour", "depth", "unsharp"),
}
# ... makes contact sheets
_SHEET_MAKERS = {
    "sheet_ragged": ("sheet",) + _SHAPE, "sheet_ragged_flat": ("sheet",) + _FLAT,
    "sheet_ragged_linear": ("sheet", "flatten", "light") + _SHAPE,
    "sheet_ragged_yuv_colour": ("sheet",) + _SHAPE + ("colour",), "sheet_ragged_yuv16": ("sheet",) + _SHAPE + ("colour", "depth"),
}
# sjpeg_hip_<stem>_bytes: what the made pictures take
_BYTES = {
    "reduce_ragged": ("factors",), "resize_ragged": ("sizes",), "orient_ragged": _SHAPE, "resize_ragged_yuv": _SHAPE,
    "sheet_ragged": ("sheet",) + _SHAPE, "resample_ragged": _SHAPE, "resample_box_ragged": _SHAPE + ("box",),
    "compose_ragged": _SHAPE + ("box", "compose"),
}
# sjpeg_hip_encode_ragged_<stem>_src and _<stem>_packed_src
_ENCODERS = {
    "full": (), "full_meta": ("meta",), "reduced": ("factors", "meta"), "resized": ("sizes", "meta"),
    "oriented": _SHAPE + ("meta",), "yuv_resized": _SHAPE + ("meta",), "flattened": _FLAT + ("meta",),
    "linear": ("flatten", "light") + _SHAPE + ("meta",), "unsharp": ("flatten", "light") + _SHAPE + ("unsharp", "meta"),
    "resampled": _RESAMPLED + ("unsharp", "meta"), "resampled_box": _RESAMPLED + ("box", "unsharp", "meta"),
    "filtered": _RESAMPLED + ("box", "filter", "meta"), "composed": _COMPOSED + ("meta",),
    "yuv_converted": _SHAPE + ("colour", "meta"), "yuv16": _SHAPE + ("colour", "depth", "meta"),
    "yuv_unsharp": _SHAPE + ("colour", "depth", "unsharp", "meta"),
}
# ... of contact sheets: the unpacked form writes sheet s at s * out_stride
_SHEET_ENCODERS = {
    "sheet": ("sheet",) + _SHAPE + ("meta",), "sheet_flat": ("sheet",) + _FLAT + ("meta",),
    "sheet_linear": ("sheet", "flatten", "light") + _SHAPE + ("meta",),
    "sheet_yuv_colour": ("sheet",) + _SHAPE + ("colour", "meta"), "sheet_yuv16": ("sheet",) + _SHAPE + ("colour", "depth", "meta"),
}


def _rows():
    """entry name -> (restype, the names of its pieces in the header's order), for every shaped entry"""
    rows = {"sjpeg_hip_encode_ragged_packed_src": (I, ("head", "params", "packed"))}     # (the twin of _full_packed_src)
    for stem, segments in _MAKERS.items():
        rows[f"sjpeg_hip_{stem}_src"] = (I, ("head",) + segments + ("pictures",))
    for stem, segments in _SHEET_MAKERS.items():
        rows[f"sjpeg_hip_{stem}_src"] = (I, ("head",) + segments + ("sheets",))
    for stem, segments in _BYTES.items():
        rows[f"sjpeg_hip_{stem}_bytes"] = (Z, ("bytes_head",) + segments)
    for tails, families in ((("unpacked", "packed"), _ENCODERS), (("strided", "packed"), _SHEET_ENCODERS)):
        for stem, segments in families.items():
            rows[f"sjpeg_hip_encode_ragged_{stem}_src"] = (I, ("head", "params") + segments + (tails[0],))
            rows[f"sjpeg_hip_encode_ragged_{stem}_packed_src"] = (I, ("head", "params") + segments + (tails[1],))
    return rows


SHAPED = _rows()


def layout(row, values):
    """The positional arguments of a shaped entry: row as SHAPED holds it, values a dict piece name -> value (a tuple
    for a piece of several slots).  A piece of the row that is missing, a name the row does not have and a value of
    the wrong length raise."""
    pieces = row[1]
    if set(values) != set(pieces):
        raise KeyError(f"layout: missing {sorted(set(pieces) - set(values))}, unknown {sorted(set(values) - set(pieces))}")
    args = []
    for name in pieces:
        width, value = len(PIECES[name]), values[name]
        if width == 1:
            args.append(value)
            continue
        if len(value) != width:
            raise ValueError(f"layout: {name} takes {width} values, not {len(value)}")
        args.extend(value)
    return tuple(args)


def call(L, symbol, values):
    """the shaped entry `symbol` of the library L on values by piece name; returns what the entry returns"""
    fn = getattr(L, symbol)
    args = layout(SHAPED[symbol], values)
    assert len(args) == len(fn.argtypes), symbol      # (ctypes does not refuse surplus arguments)
    return fn(*args)


_scan = [P, P, I64, I64, I, I, I, I]             # engine, d_rgb, row_stride, frame_stride, width, height, yuv_mode, nframes
_scan_src = [P, _src, I, I, I, I]                # engine, src, width, height, yuv_mode, nframes
_ragged = [P, I, I, I, _frames]                  # engine, format, yuv_mode, nframes, frames
_batch = [P, I, P, I, I, I, I]                   # quant, quant_per_frame, min_quant, q_bias, method, qdelta_max_luma, _chroma

# entry -> (restype, argtypes): everything that is not a shaped ragged entry
TABLE = {
    # include/sjpeg.h
    "SjpegVersion": (C.c_uint32, []),
    "SjpegCompress": (Z, [P, I, I, F, C.POINTER(_u8p)]),
    "SjpegEncode": (Z, [P, I, I, I, C.POINTER(_u8p), F, I, I]),
    "SjpegFreeBuffer": (None, [_u8p]),
    "SjpegDimensions": (C.c_bool, [P, Z, _ip, _ip, _ip]),
    "SjpegFindQuantizer": (I, [P, Z, P]),
    "SjpegEstimateQuality": (F, [P, C.c_bool]),
    "SjpegQuantMatrix": (None, [F, C.c_bool, P]),
    "SjpegRiskiness": (I, [P, I, I, I, _fp]),
    "SjpegHipLastError": (C.c_char_p, []),
    # include/sjpeg_hip.h
    "sjpeg_hip_abi_version": (I, []),
    "sjpeg_hip_device_count": (I, []),
    "sjpeg_hip_last_error": (C.c_char_p, []),
    "sjpeg_hip_engine_create": (I, [I, C.POINTER(P)]),
    "sjpeg_hip_engine_destroy": (None, [P]),
    "sjpeg_hip_frame_bound": (Z, [I, I, I, Z]),
    "sjpeg_hip_encode_scan": (I, _scan + [_tables, P, Z, I, P, Z, P, P]),
    "sjpeg_hip_scan_coeffs": (I, _scan + [_tables, P, P]),
    "sjpeg_hip_scan_histogram": (I, _scan + [P, P]),
    "sjpeg_hip_scan_symbol_stats": (I, _scan + [_tables, P, P]),
    "sjpeg_hip_quality_matrices": (None, [F, P]),
    "sjpeg_hip_finalize_quant": (None, [P, P, I, _tables]),
    "sjpeg_hip_default_huffman": (None, [_tables]),
    "sjpeg_hip_make_header": (Z, [I, I, I, P, P, Z]),
    "sjpeg_hip_adapt_quant": (None, [P, I, P, P, I, I, I, _tables]),
    "sjpeg_hip_adapt_sums": (I, [P, I, P, P, P, P, P]),
    "sjpeg_hip_adapt_quant_sums": (None, [P, P, I, P, P, I, I, I, P]),
    "sjpeg_hip_adapt_decide": (I, [P, P, I, P, I, I, I, P, P]),
    "sjpeg_hip_encode_scan_src": (I, _scan_src + [_tables, P, Z, I, P, Z, P, P]),
    "sjpeg_hip_encode_scan_packed_src": (I, [P, P, I, I, I, I, P, C.c_char_p, Z, I, P, Z, P, P, P]),
    "sjpeg_hip_scan_coeffs_src": (I, _scan_src + [_tables, P, P]),
    "sjpeg_hip_scan_histogram_src": (I, _scan_src + [P, P]),
    "sjpeg_hip_scan_symbol_stats_src": (I, _scan_src + [_tables, P, P]),
    "sjpeg_hip_scan_quant_error_src": (I, _scan_src + [_tables, P, P]),
    "sjpeg_hip_engine_entropy_bits": (I, [P, P, I]),
    "sjpeg_hip_engine_trim": (I, [P]),
    "sjpeg_hip_host_trim": (Z, []),
    "sjpeg_hip_encode_scan_multi": (I, _scan_src + [P, C.c_char_p, C.POINTER(Z), I, P, Z, P, P]),
    "sjpeg_hip_scan_symbol_stats_multi": (I, _scan_src + [P, P, P]),
    "sjpeg_hip_engine_set_pipelined": (I, [P, I]),
    "sjpeg_hip_engine_set_pixel_transform": (I, [P, F, F]),
    "sjpeg_hip_engine_get_pixel_transform": (I, [P, _fp, _fp]),
    "sjpeg_hip_engine_set_pixel_transform3": (I, [P, _fp, _fp]),
    "sjpeg_hip_engine_get_pixel_transform3": (I, [P, _fp, _fp]),
    "sjpeg_hip_engine_wait": (I, [P, P]),
    "sjpeg_hip_encode_batch_src": (I, _scan_src + [P, P, I, I, I, I, P, Z, P, P]),
    "sjpeg_hip_optimize_huffman": (None, [P, I, C.POINTER(HuffmanSpec), _tables]),
    "sjpeg_hip_make_header_ex": (Z, [I, I, I, P, C.POINTER(HuffmanSpec), P, Z]),
    "sjpeg_hip_make_header_meta": (Z, [I, I, I, P, P, P, P, Z]),
    "sjpeg_hip_sharp_workspace": (Z, [I, I, I]),
    "sjpeg_hip_sharp_yuv": (I, [P, I, I, I, P, P, P, I64, I64, P, Z, P]),
    "sjpeg_hip_set_riskiness_table": (I, [P, Z]),
    "sjpeg_hip_has_riskiness_table": (I, []),
    "sjpeg_hip_riskiness_sums": (I, [P, I, I, I, P, P, P]),
    "sjpeg_hip_segment_count": (I, [I, I, I]),
    "sjpeg_hip_band_bound": (Z, [I, I, I, I, I]),
    "sjpeg_hip_encode_band_src": (I, [P, P, I, I, I, P, I, I, P, Z, P, P]),
    "sjpeg_hip_stitch_bands": (I, [P, I, P, Z, P, C.c_char_p, Z, I, P, Z, P, P]),
    "sjpeg_hip_engine_set_timing": (I, [P, I]),
    "sjpeg_hip_engine_last_scan_ms": (F, [P]),
    "sjpeg_hip_engine_last_total_ms": (F, [P]),
    "sjpeg_hip_engine_scratch_bytes": (Z, [P]),
    "sjpeg_hip_compact_streams": (I, [P, Z, P, I, P, Z, P, P]),
    "sjpeg_hip_debug_stream_read": (I, [P, Z, P, P]),
    "sjpeg_hip_debug_valu_rate": (I, [P, P]),
    "sjpeg_hip_debug_shader_clock": (I, [P, P]),
    "sjpeg_hip_restart_interval": (I, [I]),
    "sjpeg_hip_header_add_restart": (Z, [P, Z, Z, I]),
    "sjpeg_hip_encode_intervals_src": (I, [P, P, I, I, I, P, I, I, P, Z, P, P]),
    "sjpeg_hip_comm_unique_id": (I, [P]),
    "sjpeg_hip_comm_create": (I, [P, I, I, C.POINTER(P)]),
    "sjpeg_hip_comm_create_local": (I, [P, I, I, C.POINTER(P)]),
    "sjpeg_hip_comm_adopt": (I, [P, C.POINTER(P)]),
    "sjpeg_hip_comm_destroy": (None, [P]),
    "sjpeg_hip_comm_rank": (I, [P]),
    "sjpeg_hip_comm_world": (I, [P]),
    "sjpeg_hip_gather_rows": (I, [P, P, P, I, I, P, P, P, P]),
    "sjpeg_hip_gather_bytes": (I, [P, I, P, I, P, P, P, Z, P]),
    "sjpeg_hip_gather_streams": (I, [P, I, P, P, P, I, I, P, P, Z, P, P, P]),
    "sjpeg_hip_encode_ragged_src": (I, _ragged + [P, I, C.c_char_p, P, I, P, P, P]),
    "sjpeg_hip_scan_histogram_ragged_src": (I, _ragged + [P, P]),
    "sjpeg_hip_scan_symbol_stats_ragged_src": (I, _ragged + [P, I, P, P]),
    "sjpeg_hip_scan_quant_error_ragged_src": (I, _ragged + [P, I, P, P]),
    "sjpeg_hip_scan_counted_bits_ragged_src": (I, _ragged + [P, I, P, P]),
    "sjpeg_hip_encode_ragged_batch_src": (I, _ragged + _batch + [P, P, P]),
    "sjpeg_hip_encode_ragged_auto_src": (I, _ragged + _batch + [P, P, P, P]),
    "sjpeg_hip_encode_ragged_trellis_src": (I, _ragged + _batch + [P, P, P, P]),
    "sjpeg_hip_encode_ragged_search_src": (I, _ragged + _batch + [C.POINTER(SearchParams), I, _fp, _fp, P, P, P]),
    "sjpeg_hip_riskiness_ragged_src": (I, [P, I, I, _frames, P, P, P]),
    "sjpeg_hip_riskiness_verdict": (I, [C.POINTER(C.c_uint64), I, I, _fp]),
    "sjpeg_hip_sharp_ragged_workspace": (Z, [I, _frames]),
    "sjpeg_hip_sharp_yuv_ragged": (I, [P, I, I, _frames, P, P, P, P, Z, P]),
    "sjpeg_hip_engine_search_stats": (I, [P, C.POINTER(C.c_uint64)]),
    "sjpeg_hip_metadata_size": (I, [P, C.POINTER(Z)]),
    # the host-only size and sample rules of the shaped families
    "sjpeg_hip_reduced_size": (I, [I, I, I, _ip, _ip]),
    "sjpeg_hip_fit_size": (I, [I, I, I, I, _ip, _ip]),
    "sjpeg_hip_oriented_size": (I, [I, I, I, _ip, _ip]),
    "sjpeg_hip_exif_orientation": (I, [P, Z]),
    "sjpeg_hip_exif_reset_orientation": (I, [P, Z]),
    "sjpeg_hip_yuv_plane_size": (I, [I, I, I, I, _ip, _ip]),
    "sjpeg_hip_sheet_size": (I, [P, I, _ip, _ip]),
    "sjpeg_hip_sheet_places": (I, [I, I, _frames, P, P, P, P]),
    "sjpeg_hip_yuv_colour_samples": (I, [P, Z, P, P]),
    "sjpeg_hip_yuv16_samples": (I, [P, Z, P, P]),
    "sjpeg_hip_light_table": (I, [I, P]),
    "sjpeg_hip_light_round": (I, [I, C.c_uint64, C.c_uint32, C.c_uint32, P]),
    "sjpeg_hip_unsharp_sample": (I, [I, I, P, P]),
    "sjpeg_hip_resample_ksize": (I, [I, I, I]),
    "sjpeg_hip_resample_table": (I, [I, I, I, P, P, Z]),
    "sjpeg_hip_thumbnail_size": (I, [I, I, D, D, P]),
    "sjpeg_hip_fit_crop": (I, [I, I, I, I, D, D, D, P]),
    "sjpeg_hip_resample_box_decide": (I, [I, I, I, I, I, P, P]),
    "sjpeg_hip_resample_box_ksize": (I, [I, I, I, F, F]),
    "sjpeg_hip_resample_box_table": (I, [I, I, I, F, F, P, P, Z]),
    "sjpeg_hip_pillow_filter_weights": (I, [I, F, P, P, P, P]),
    "sjpeg_hip_contain_size": (I, [I, I, I, I, P]),
    "sjpeg_hip_pad_place": (I, [I, I, I, I, D, D, P]),
    "sjpeg_hip_compose_sample": (I, [I] * 6),
}
TABLE.update((name, (restype, [t for piece in pieces for t in PIECES[piece]])) for name, (restype, pieces) in SHAPED.items())


def apply(L, names):
    """sets the restype and the argument types of every entry in `names` on the library L; a name without a row is an
    error, so that an entry cannot be exported without its types"""
    for name in names:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = TABLE[name][0], list(TABLE[name][1])
