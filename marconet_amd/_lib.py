"""ctypes binding of libmarconet_hip.so (C-ABI declared in include/marconet_hip.h).

There is deliberately NO fallback: if the shared library is missing or a symbol cannot be resolved the
import of the ops fails loudly — the product path never routes through PyTorch eager ops or the CPU oracle.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MARCONET_HIP_LIB", os.path.join(_HERE, "lib", "libmarconet_hip.so"))

ABI_VERSION = 4               # MNET_ABI_VERSION of include/marconet_hip.h this binding was written against
MNET_F32, MNET_F16, MNET_F16X2, MNET_F16M = 0, 1, 2, 3
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_LRELU_SQRT2, ACT_TANH, ACT_GELU, ACT_SIGMOID = range(7)
ALGO_AUTO, ALGO_REG_STAGED, ALGO_LDS_DMA, ALGO_SKINNY, ALGO_DMA_CFG0, ALGO_STRIP_CFG0, ALGO_DMA_CFG16, ALGO_FLAG_ONE_TILE = 0, 1, 2, 3, 16, 32, 64, 256
ALGO_FLAG_X1_CENTER = 512     # x1 contributes through the filter's centre tap only (a 1x1 skip conv folded into the k-loop)
ALGO_FLAG_SHUFFLE2 = 1024     # pixel-shuffle output mode: conv3x3(bilinear x2) in polyphase form (cout = 4 C phase-major, y = [n,2h,2w,C])
ALGO_FLAG_F32_OUT = 2048      # fp32 output of an fp16+8 launch (the one-wave tile's plain epilogue only): the tap planes of an up-conv, which only the fold reads

c_int, c_void_p, c_float, c_double, c_i64 = ctypes.c_int32, ctypes.c_void_p, ctypes.c_float, ctypes.c_double, ctypes.c_int64


class ConvDesc(ctypes.Structure):
    """mirror of ``mnet_conv_desc`` (include/marconet_hip.h)"""
    _fields_ = [
        ("dtype", c_int),
        ("x0", c_void_p), ("c0", c_int),
        ("x1", c_void_p), ("c1", c_int),
        ("n", c_int), ("h", c_int), ("w", c_int),
        ("wgt", c_void_p),
        ("cout", c_int), ("kh", c_int), ("kw", c_int), ("stride_h", c_int), ("stride_w", c_int),
        ("pad_h", c_int), ("pad_w", c_int),
        ("ho", c_int), ("wo", c_int),
        ("in_scale", c_void_p), ("in_shift", c_void_p), ("in_swish", c_int),
        ("valid_w", c_void_p),
        ("out_scale", c_void_p), ("bias", c_void_p),
        ("residual", c_void_p), ("res_mod", c_int),
        ("act", c_int),
        ("post_scale", c_void_p),
        ("y", c_void_p),
        ("gn_partial", c_void_p),
    ]


class LqImage(ctypes.Structure):
    """mirror of ``mnet_lq_image`` (include/marconet_hip.h): one image of mnet_lq_from_u8's device table"""
    _fields_ = [("offset", c_i64), ("h", c_int), ("w", c_int), ("dw", c_int), ("reserved", c_int), ("scale", c_double)]


LQ_FORM_F32_NCHW, LQ_FORM_U8_HWC = 0, 1


class LqWindow(ctypes.Structure):
    """mirror of ``mnet_lq_window`` (include/marconet_hip_windows.h): one window of mnet_lq_windows_u8's device table"""
    _fields_ = [("offset", c_i64), ("pitch", c_int), ("h", c_int), ("w", c_int), ("dw", c_int), ("scale", c_double)]


class RowInkBox(ctypes.Structure):
    """mirror of ``mnet_ink_box`` (include/marconet_hip_rowink.h): one box of mnet_row_ink_u8's device table"""
    _fields_ = [("offset", c_i64), ("pitch", c_int), ("h", c_int), ("w", c_int), ("out", c_int)]


class BoxInkBox(ctypes.Structure):
    """mirror of ``mnet_ink_box2`` (include/marconet_hip_boxink.h): one box of mnet_box_ink_u8's device table"""
    _fields_ = [("offset", c_i64), ("pitch", c_int), ("h", c_int), ("w", c_int), ("out_rows", c_int), ("out_cols", c_int), ("reserved", c_int)]


BOXINK_TILE_W, BOXINK_TILE_H = 256, 32      # the tile of one workgroup of mnet_box_ink_u8 (csrc/ink_kernels.hip)


class SkewInkBox(ctypes.Structure):
    """mirror of ``mnet_skew_box`` (include/marconet_hip_skewink.h): one record of mnet_skew_ink_u8's device table"""
    _fields_ = [("c1", c_int), ("r1", c_int), ("c2", c_int), ("r2", c_int), ("slope", c_int), ("out_rows", c_int), ("out_cols", c_int),
                ("px1", c_int), ("py1", c_int), ("px2", c_int), ("py2", c_int), ("reserved", c_int)]


SKEWINK_TILE_W, SKEWINK_TILE_H = 256, 32    # the tile of one workgroup of mnet_skew_ink_u8 (csrc/ink_kernels.hip)


class PanelStrip(ctypes.Structure):
    """mirror of ``mnet_panel_strip`` (include/marconet_hip.h): one strip of mnet_panel_u8's device table"""
    _fields_ = [("show_w", c_int), ("preview_index", c_int), ("glyph0", c_int), ("n_glyphs", c_int), ("step", c_double)]


class StitchLine(ctypes.Structure):
    """mirror of ``mnet_stitch_line`` (include/marconet_hip.h): one line of mnet_stitch_u8's device table"""
    _fields_ = [("out_w", c_int), ("win0", c_int), ("n_win", c_int), ("reserved", c_int)]


class StitchWindow(ctypes.Structure):
    """mirror of ``mnet_stitch_window`` (include/marconet_hip.h): one restored window of a line"""
    _fields_ = [("sr_index", c_int), ("offset", c_int), ("show_w", c_int), ("reserved", c_int)]


class PasteRegion(ctypes.Structure):
    """mirror of ``mnet_paste_region`` (include/marconet_hip.h): one text region of mnet_paste_u8's device table"""
    _fields_ = [("line_index", c_int), ("src_w", c_int), ("x0", c_int), ("y0", c_int), ("rw", c_int), ("rh", c_int), ("feather", c_int), ("k", c_int),
                ("scale_x", c_double), ("scale_y", c_double)]


class QuadCrop(ctypes.Structure):
    """mirror of ``mnet_quad_crop`` (include/marconet_hip_quad.h): one rectified window of mnet_quad_crop_u8's device table"""
    _fields_ = [("offset", c_i64), ("w", c_int), ("h", c_int), ("c0", c_int), ("reserved", c_int), ("m", c_double * 9)]


class QuadRegion(ctypes.Structure):
    """mirror of ``mnet_quad_region`` (include/marconet_hip_quad.h): one quadrilateral region of mnet_quad_paste_u8's device table"""
    _fields_ = [("ax0", c_int), ("ay0", c_int), ("rw", c_int), ("rh", c_int), ("bx0", c_int), ("by0", c_int), ("bw", c_int), ("bh", c_int),
                ("feather", c_int), ("reserved", c_int), ("n", c_double * 9)]


class ColumnCell(ctypes.Structure):
    """mirror of ``mnet_column_cell`` (include/marconet_hip_columns.h): one character cell of one window of mnet_column_gather_u8's device table"""
    _fields_ = [("offset", c_i64), ("win_w", c_int), ("dx", c_int), ("dw", c_int), ("sx", c_int), ("sy", c_int), ("sw", c_int), ("sh", c_int),
                ("reserved", c_int), ("scale_x", c_double), ("scale_y", c_double)]


class ColumnPaste(ctypes.Structure):
    """mirror of ``mnet_column_paste`` (include/marconet_hip_columns.h): one character cell of mnet_column_paste_u8's device table"""
    _fields_ = [("line_index", c_int), ("src_x0", c_int), ("src_w", c_int), ("x0", c_int), ("y0", c_int), ("rw", c_int), ("rh", c_int), ("feather", c_int),
                ("k", c_int), ("fx0", c_int), ("fy0", c_int), ("fw", c_int), ("fh", c_int), ("reserved", c_int), ("scale_x", c_double), ("scale_y", c_double)]


class TileSpan(ctypes.Structure):
    """mirror of ``mnet_tile_span`` (include/marconet_hip_ordered.h): one 64 x 16 tile of the page in mnet_paste_ordered_u8's span array"""
    _fields_ = [("first", c_int), ("count", c_int)]


class PageItem(ctypes.Structure):
    """mirror of ``mnet_page_item`` (include/marconet_hip_mixed.h): one thing mnet_paste_mixed_u8 pastes — entry ``index`` of the table of its ``kind``"""
    _fields_ = [("kind", c_int), ("index", c_int), ("x0", c_int), ("y0", c_int), ("rw", c_int), ("rh", c_int)]


ITEM_CELL, ITEM_QUAD, ITEM_CURVE = 0, 1, 2      # MNET_ITEM_*


class CurveSeg(ctypes.Structure):
    """mirror of ``mnet_curve_seg`` (include/marconet_hip_curve.h): one bilinear segment of a curved region"""
    _fields_ = [("c", c_double * 8), ("u0", c_int), ("w", c_int), ("bx0", c_int), ("by0", c_int), ("bw", c_int), ("bh", c_int)]


class CurveCrop(ctypes.Structure):
    """mirror of ``mnet_curve_crop`` (include/marconet_hip_curve.h): one rectified window of mnet_curve_crop_u8's device table"""
    _fields_ = [("offset", c_i64), ("w", c_int), ("h", c_int), ("c0", c_int), ("seg0", c_int), ("nseg", c_int), ("reserved", c_int)]


class CurveRegion(ctypes.Structure):
    """mirror of ``mnet_curve_region`` (include/marconet_hip_curve.h): one curved region of mnet_curve_paste_u8's device table"""
    _fields_ = [("ax0", c_int), ("ay0", c_int), ("rw", c_int), ("rh", c_int), ("bx0", c_int), ("by0", c_int), ("bw", c_int), ("bh", c_int),
                ("feather", c_int), ("seg0", c_int), ("nseg", c_int), ("reserved", c_int)]


class CmpStats(ctypes.Structure):
    """mirror of ``mnet_cmp_stats`` (include/marconet_hip.h): one group's record of mnet_compare_stats"""
    _fields_ = [("max_abs_diff", c_float), ("max_abs_ref", c_float), ("max_abs_mode", c_float), ("reserved", c_int),
                ("argmax_index", c_i64), ("sum_sq_diff", c_double), ("sum_sq_ref", c_double),
                ("nonfinite_mode", c_i64), ("nonfinite_ref", c_i64)]


CMP_WG_ELEMS, CMP_MAX_SLICES = 2048, 32      # MNET_CMP_WG_ELEMS, MNET_CMP_MAX_SLICES


def cmp_slices(elems_per_group):
    """MNET_CMP_SLICES: workgroups (= partial records) per group"""
    return max(1, min(CMP_MAX_SLICES, -(-int(elems_per_group) // CMP_WG_ELEMS)))


def cmp_workspace_bytes(n_groups, elems_per_group):
    """MNET_CMP_WORKSPACE_BYTES"""
    return int(n_groups) * cmp_slices(elems_per_group) * ctypes.sizeof(CmpStats)


def cmp_records(raw):
    """bytes / uint8 array (a host copy of ops.compare_stats' result) → list of CmpStats, one per group"""
    raw = bytes(memoryview(raw).cast("B")) if not isinstance(raw, (bytes, bytearray)) else bytes(raw)
    n = ctypes.sizeof(CmpStats)
    if len(raw) % n:
        raise ValueError("cmp_records: %d bytes are no whole number of %d-byte records" % (len(raw), n))
    return [CmpStats.from_buffer_copy(raw, k) for k in range(0, len(raw), n)]


# name -> (restype, argtypes); every symbol include/marconet_hip.h declares
SYMBOLS = {
    "mnet_last_error": (ctypes.c_char_p, []),
    "mnet_abi_version": (c_int, []),
    "mnet_conv2d_nhwc": (c_int, [ctypes.POINTER(ConvDesc), c_void_p]),
    "mnet_conv2d_nhwc_ex": (c_int, [ctypes.POINTER(ConvDesc), c_int, c_void_p]),
    "mnet_conv2d_splitk": (c_int, [ctypes.POINTER(ConvDesc), c_int, c_void_p, c_void_p]),
    "mnet_conv2d_plan": (c_int, [ctypes.POINTER(ConvDesc), c_int]),
    "mnet_conv2d_flops": (c_double, [ctypes.POINTER(ConvDesc)]),
    "mnet_nchw_to_nhwc": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mnet_nhwc_to_nchw": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mnet_upsample2x_nhwc": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mnet_upsample2x_scale_nhwc": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mnet_upsample2x_convert_nhwc": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mnet_affine_act_nhwc": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "mnet_groupnorm_affine": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                      c_float, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mnet_groupnorm_affine_from_partial": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "mnet_polyphase_ring_fix": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mnet_groupnorm_affine_from_partial_ring": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "mnet_adain_crop_concat": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mnet_adain_crop_concat_gn": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "mnet_adain_crop_concat_split": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_int, c_void_p]),
    "mnet_glyph_scatter_affine": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                          c_void_p, c_void_p, c_void_p, c_void_p]),
    "mnet_layernorm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "mnet_token_mix": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                               c_int, c_float, c_void_p]),
    "mnet_attention": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "mnet_pixelnorm": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "mnet_embed_gather": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mnet_embed_gather_scaled": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mnet_demod": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mnet_argmax_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "mnet_convert": (c_int, [c_void_p, c_int, c_void_p, c_int, c_i64, c_void_p]),
    "mnet_fused_bias_act": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_float, c_float, c_void_p]),
    "mnet_torgb": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mnet_conv3x3_rgb": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mnet_sr_postprocess": (c_int, [c_void_p, c_int, c_void_p, c_int, c_i64, c_int, c_void_p]),
    "mnet_nonfinite_flag": (c_int, [c_void_p, c_int, c_i64, c_void_p, c_void_p]),
    "mnet_compare_stats": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_i64, c_void_p, c_void_p, c_void_p]),
    "mnet_lq_from_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "mnet_panel_u8": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "mnet_stitch_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "mnet_paste_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "mnet_pack_weights": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_int, c_int, c_int, c_void_p,
                                  c_void_p, c_void_p]),
    "mnet_pack_wsq": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "mnet_demod_scaled": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mnet_style_rows": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "mnet_gather_rows": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
}

# name -> (restype, argtypes); the entry point include/marconet_hip_upfold.h declares beside that table (bound by load() like the table's)
UPFOLD_SYMBOLS = {
    "mnet_upfold3x3_nhwc": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
}

# ... and the one include/marconet_hip_upfold_f32.h declares (the fold with its tap planes in fp32)
UPFOLD_F32Z_SYMBOLS = {
    "mnet_upfold3x3_f32z_nhwc": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
}

# ... and the two include/marconet_hip_quad.h declares (quadrilateral text regions of a page: the gather in and the gather out)
QUAD_SYMBOLS = {
    "mnet_quad_crop_u8": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_i64, c_void_p]),
    "mnet_quad_paste_u8": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
}

# ... and the two include/marconet_hip_columns.h declares (vertical text columns of a page: the gather of the cells and their paste)
COLUMN_SYMBOLS = {
    "mnet_column_gather_u8": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_i64, c_void_p]),
    "mnet_column_paste_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
}

# ... and the two include/marconet_hip_curve.h declares (curved text regions of a page, polygon strips: the gather in and the gather out)
CURVE_SYMBOLS = {
    "mnet_curve_crop_u8": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_i64, c_void_p]),
    "mnet_curve_paste_u8": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
}

# ... and the one include/marconet_hip_ordered.h declares (overlapping regions and cells of a page pasted in the caller's order, by page tile)
ORDERED_SYMBOLS = {
    "mnet_paste_ordered_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
}

# ... and the one include/marconet_hip_mixed.h declares (regions of every kind of a page, overlapping, pasted in the caller's order by page tile)
MIXED_SYMBOLS = {
    "mnet_paste_mixed_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                    c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
}

# ... and the one include/marconet_hip_windows.h declares (the encoder's input from windows — views — of images on the device)
WINDOW_SYMBOLS = {
    "mnet_lq_windows_u8": (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
}

# ... and the one include/marconet_hip_rowink.h declares (the ink profile of boxes of a page: where a column's characters are, from its pixels)
ROWINK_SYMBOLS = {
    "mnet_row_ink_u8": (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_void_p, c_i64, c_void_p]),
}

# ... and the one include/marconet_hip_boxink.h declares (both ink profiles of boxes of a page above a noise floor: where a page's lines are)
BOXINK_SYMBOLS = {
    "mnet_box_ink_u8": (c_int, [c_void_p, c_i64, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_void_p]),
}

# ... and the one include/marconet_hip_skewink.h declares (both ink profiles of boxes of a sheared frame of a page: a skewed page's slope and lines)
SKEWINK_SYMBOLS = {
    "mnet_skew_ink_u8": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_void_p]),
}

_lib = None


class MarconetHipError(RuntimeError):
    """Raised for a non-zero C-ABI status; test_sr.py's ``try/except ... continue`` (:181-190) still works."""


def load():
    """dlopen the library once and bind every declared symbol (raises if anything is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            "marconet_amd: %s not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or marconet_amd/csrc/build.sh (there is no CPU/eager fallback)" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in [f for k, table in sorted(globals().items()) if k.endswith("SYMBOLS") for f in table.items()]:      # every header's table
        fn = getattr(lib, name)          # AttributeError if the symbol is absent
        fn.restype = res
        fn.argtypes = args
    if lib.mnet_abi_version() != ABI_VERSION:
        raise ImportError("marconet_amd: ABI version mismatch in %s" % LIB_PATH)
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().mnet_last_error()
        raise MarconetHipError("%s failed (status %d): %s" % (what, status, msg.decode() if msg else "?"))
