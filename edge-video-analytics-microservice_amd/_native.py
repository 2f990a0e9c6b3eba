"""ctypes binding of ``libevam_pp.so`` (the C ABI declared in ``include/evam_pp.h``).

The structures below mirror the header field-for-field; ``tests/test_abi.py`` checks their sizes
against the compiled library's expectations and that every declared symbol is exported.

``torch`` is imported before the library is loaded: the ROCm PyTorch wheel ships its own
``libamdhip64.so`` (SONAME ``libamdhip64.so.7``), and loading torch first makes the dynamic linker
bind this library to that same HIP runtime instead of a second copy from ``/opt/rocm``. Device
pointers and streams created by torch are then valid here.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
import sys

LIB_NAME = "libevam_pp.so"
PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, LIB_NAME)

# evam_fourcc
FOURCC_NV12 = 0x3231564E
FOURCC_I420 = 0x30323449
FOURCC_BGRX = 0x58524742
FOURCC_BGRA = 0x41524742
FOURCC_BGR = 0x20524742

# evam_pp_status
OK = 0
ERR_INVALID_ARG = -1
ERR_UNSUPPORTED = -2
ERR_ALIGNMENT = -3
ERR_EMPTY_ROI = -4
ERR_HIP = -5
ERR_NO_DEVICE = -6
ERR_OOM = -7
STATUS_NAMES = {
    OK: "EVAM_PP_OK", ERR_INVALID_ARG: "EVAM_PP_ERR_INVALID_ARG", ERR_UNSUPPORTED: "EVAM_PP_ERR_UNSUPPORTED",
    ERR_ALIGNMENT: "EVAM_PP_ERR_ALIGNMENT", ERR_EMPTY_ROI: "EVAM_PP_ERR_EMPTY_ROI", ERR_HIP: "EVAM_PP_ERR_HIP",
    ERR_NO_DEVICE: "EVAM_PP_ERR_NO_DEVICE", ERR_OOM: "EVAM_PP_ERR_OOM",
}

RESIZE_NO_ASPECT, RESIZE_ASPECT, RESIZE_ASPECT_CROP = 0, 1, 2
PLACE_TOP_LEFT, PLACE_CENTER = 0, 1
COLOR_BGR, COLOR_RGB = 0, 1
DTYPE_U8, DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2, 3  # F16 / BF16: the F32 value rounded once (RNE)
LAYOUT_NCHW, LAYOUT_NHWC = 0, 1
NORM_RANGE, NORM_MEAN_STD = 1, 2
OPT_STATS, OPT_TIMING = 1, 2

ABI_VERSION = 3  # 2: evam_pp_run_slots; 3: evam_tensor.layout

# Every symbol include/evam_pp.h declares.
EXPORTED_SYMBOLS = (
    "evam_pp_create", "evam_pp_run", "evam_pp_run_slots", "evam_pp_sync", "evam_pp_set_stream", "evam_pp_set_option",
    "evam_pp_get_stats", "evam_pp_destroy", "evam_pp_last_error", "evam_pp_abi_version",
    "evam_pp_linear_table", "evam_pp_norm_table",
    "evam_pp_jpeg_header", "evam_pp_encode_jpeg",
    "evam_pp_ssd_rois", "evam_pp_ssd_rois_host", "evam_pp_run_device_rois",
    "evam_pp_jpeg_info", "evam_pp_decode_jpeg", "evam_pp_decode_jpeg_host",
    "evam_pp_decode_jpeg_planes", "evam_pp_decode_jpeg_planes_host",
    "evam_pp_track_host", "evam_pp_tracker_create", "evam_pp_tracker_destroy", "evam_pp_tracker_reset",
    "evam_pp_tracker_read", "evam_pp_track_device_rois", "evam_pp_ssd_rois_ex",
    "evam_pp_detection_output", "evam_pp_detection_output_host",
)
# ... and the one that returns size_t (tests/test_abi.py reads the header's int / void / const char* declarations)
EXPORTED_SYMBOLS_SIZE_T = ("evam_pp_jpeg_bound",)
EXPORTED_SYMBOLS_FLOAT = ("evam_pp_expf",)  # ... and the one that returns float

c_i32 = ctypes.c_int32


class EvamImage(ctypes.Structure):
    _fields_ = [("fourcc", c_i32), ("width", c_i32), ("height", c_i32), ("pitch", c_i32 * 3),
                ("planes", ctypes.c_void_p * 3)]


class EvamRoi(ctypes.Structure):
    _fields_ = [("src_index", c_i32), ("x", c_i32), ("y", c_i32), ("w", c_i32), ("h", c_i32)]


class EvamPreproc(ctypes.Structure):
    _fields_ = [("resize_mode", c_i32), ("placement", c_i32), ("color_order", c_i32), ("out_dtype", c_i32),
                ("norm_flags", c_i32), ("fill", ctypes.c_uint8 * 4), ("range", ctypes.c_float * 2),
                ("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3)]


class EvamTensor(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("n", c_i32), ("c", c_i32), ("h", c_i32), ("w", c_i32),
                ("slot_offset", c_i32), ("slot_stride", c_i32), ("layout", c_i32), ("reserved", c_i32)]


class EvamTransform(ctypes.Structure):
    _fields_ = [("scale_x", ctypes.c_float), ("scale_y", ctypes.c_float), ("crop_x", c_i32), ("crop_y", c_i32),
                ("crop_w", c_i32), ("crop_h", c_i32), ("pad_x", c_i32), ("pad_y", c_i32),
                ("resized_w", c_i32), ("resized_h", c_i32)]


class EvamRoiList(ctypes.Structure):
    """``evam_roi_list``: a ROI list in device memory (host memory for ``evam_pp_ssd_rois_host``)."""

    _fields_ = [("rois", ctypes.c_void_p), ("count", ctypes.c_void_p), ("cap", c_i32), ("reserved", c_i32)]


class EvamStats(ctypes.Structure):
    _fields_ = [("src_bytes", ctypes.c_int64), ("dst_bytes", ctypes.c_int64), ("n_items", c_i32),
                ("n_launches", c_i32), ("last_kernel_ms", ctypes.c_float), ("kernels", ctypes.c_uint32)]


class EvamJpegInfo(ctypes.Structure):
    """``evam_jpeg_info``: what ``evam_pp_jpeg_info`` reads from a file's markers."""

    _fields_ = [("width", c_i32), ("height", c_i32), ("components", c_i32), ("h_samp", c_i32), ("v_samp", c_i32),
                ("restart_interval", c_i32), ("scan_offset", ctypes.c_uint32)]


TRACK_SLOTS, TRACK_DETS, TRACK_NONE = 128, 128, 0xFFFFFFFF  # EVAM_TRACK_*


class EvamTrackSlot(ctypes.Structure):
    _fields_ = [("id", ctypes.c_uint32), ("label", c_i32), ("x", c_i32), ("y", c_i32), ("w", c_i32), ("h", c_i32),
                ("lost", c_i32), ("classified_at", ctypes.c_uint32)]


class EvamTrackState(ctypes.Structure):
    """``evam_track_state``: one stream's tracker state. Zeroed memory counts as a fresh state."""

    _fields_ = [("next_id", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 7), ("slots", EvamTrackSlot * TRACK_SLOTS)]


class EvamTrackCfg(ctypes.Structure):
    _fields_ = [("max_lost", c_i32), ("iou_threshold", ctypes.c_float)]


class EvamTrackItem(ctypes.Structure):
    _fields_ = [("stream", c_i32), ("frame", ctypes.c_uint32)]


DETOUT_MAX_TOP_K, DETOUT_MAX_CLASSES = 1024, 256  # EVAM_DETOUT_*


class EvamDetoutCfg(ctypes.Structure):
    """``evam_detout_cfg``: what ``evam_pp_detection_output`` reads of an SSD DetectionOutput layer's attributes."""

    _fields_ = [("num_classes", c_i32), ("background_label", c_i32), ("top_k", c_i32), ("keep_top_k", c_i32),
                ("confidence_threshold", ctypes.c_float), ("nms_threshold", ctypes.c_float)]


# evam_pp_stats.kernels bits (include/evam_pp.h evam_kernel_family)
KERNEL_GENERIC, KERNEL_ROWS, KERNEL_STAGED, KERNEL_WAVE = 1, 2, 4, 8
KERNEL_STRIP, KERNEL_BAND, KERNEL_ROI = 16, 32, 64
KERNEL_JPEG = 128
KERNEL_JPEG_DEC = 256
KERNEL_DETOUT = 512

JPEG_HEADER_LEN = 623  # SOI .. SOS of every file evam_pp_encode_jpeg writes


STRUCT_SIZES = {EvamImage: 48, EvamRoi: 20, EvamPreproc: 56, EvamTensor: 40, EvamTransform: 40, EvamStats: 32,
                EvamRoiList: 24, EvamJpegInfo: 28, EvamTrackSlot: 32, EvamTrackState: 4128, EvamTrackCfg: 8,
                EvamTrackItem: 8, EvamDetoutCfg: 24}

_LIB = None


def _declare(lib: ctypes.CDLL) -> ctypes.CDLL:
    P = ctypes.POINTER
    vp = ctypes.c_void_p
    lib.evam_pp_create.argtypes = [ctypes.c_int, vp, P(vp)]
    lib.evam_pp_create.restype = ctypes.c_int
    lib.evam_pp_run.argtypes = [vp, P(EvamImage), ctypes.c_int, P(EvamRoi), ctypes.c_int, P(EvamPreproc),
                                P(EvamTensor), P(EvamTransform)]
    lib.evam_pp_run.restype = ctypes.c_int
    lib.evam_pp_run_slots.argtypes = [vp, P(EvamImage), ctypes.c_int, P(EvamRoi), ctypes.c_int, P(EvamPreproc),
                                      P(EvamTensor), P(c_i32), P(EvamTransform)]
    lib.evam_pp_run_slots.restype = ctypes.c_int
    lib.evam_pp_sync.argtypes = [vp]
    lib.evam_pp_sync.restype = ctypes.c_int
    lib.evam_pp_set_stream.argtypes = [vp, vp]
    lib.evam_pp_set_stream.restype = ctypes.c_int
    lib.evam_pp_set_option.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    lib.evam_pp_set_option.restype = ctypes.c_int
    lib.evam_pp_get_stats.argtypes = [vp, P(EvamStats)]
    lib.evam_pp_get_stats.restype = ctypes.c_int
    lib.evam_pp_destroy.argtypes = [vp]
    lib.evam_pp_destroy.restype = None
    lib.evam_pp_last_error.argtypes = []
    lib.evam_pp_last_error.restype = ctypes.c_char_p
    lib.evam_pp_abi_version.argtypes = []
    lib.evam_pp_abi_version.restype = ctypes.c_int
    lib.evam_pp_linear_table.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, P(c_i32),
                                         P(ctypes.c_int16), P(ctypes.c_int16)]
    lib.evam_pp_linear_table.restype = ctypes.c_int
    lib.evam_pp_norm_table.argtypes = [P(EvamPreproc), vp]
    lib.evam_pp_norm_table.restype = ctypes.c_int
    lib.evam_pp_jpeg_header.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t,
                                        P(ctypes.c_size_t)]
    lib.evam_pp_jpeg_header.restype = ctypes.c_int
    lib.evam_pp_jpeg_bound.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.evam_pp_jpeg_bound.restype = ctypes.c_size_t
    lib.evam_pp_encode_jpeg.argtypes = [vp, P(EvamImage), ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t, vp]
    lib.evam_pp_encode_jpeg.restype = ctypes.c_int
    if not hasattr(lib, "evam_pp_ssd_rois"):  # an A/B variant built before the device-list calls (EVAM_PP_LIB)
        return lib
    ssd = [vp, ctypes.c_int, ctypes.c_int, P(EvamImage), P(EvamTransform), ctypes.c_int, ctypes.c_int, ctypes.c_float,
           P(c_i32), ctypes.c_int, P(EvamRoiList)]
    lib.evam_pp_ssd_rois.argtypes = [vp] + ssd
    lib.evam_pp_ssd_rois.restype = ctypes.c_int
    lib.evam_pp_ssd_rois_host.argtypes = ssd
    lib.evam_pp_ssd_rois_host.restype = ctypes.c_int
    lib.evam_pp_run_device_rois.argtypes = [vp, P(EvamImage), ctypes.c_int, P(EvamRoiList), P(EvamPreproc),
                                            P(EvamTensor), vp]
    lib.evam_pp_run_device_rois.restype = ctypes.c_int
    lib.evam_pp_jpeg_info.argtypes = [vp, ctypes.c_size_t, P(EvamJpegInfo)]
    lib.evam_pp_jpeg_info.restype = ctypes.c_int
    dec = [P(vp), P(ctypes.c_size_t), ctypes.c_int, P(EvamImage), vp]
    lib.evam_pp_decode_jpeg.argtypes = [vp] + dec
    lib.evam_pp_decode_jpeg.restype = ctypes.c_int
    lib.evam_pp_decode_jpeg_host.argtypes = dec
    lib.evam_pp_decode_jpeg_host.restype = ctypes.c_int
    if not hasattr(lib, "evam_pp_decode_jpeg_planes"):  # an A/B variant built before the raw-plane output
        return lib
    lib.evam_pp_decode_jpeg_planes.argtypes = [vp] + dec
    lib.evam_pp_decode_jpeg_planes.restype = ctypes.c_int
    lib.evam_pp_decode_jpeg_planes_host.argtypes = dec
    lib.evam_pp_decode_jpeg_planes_host.restype = ctypes.c_int
    lib.evam_pp_track_host.argtypes = [P(EvamTrackState), P(EvamTrackCfg), ctypes.c_uint32, vp, vp, ctypes.c_int,
                                       vp, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.evam_pp_track_host.restype = ctypes.c_int
    lib.evam_pp_tracker_create.argtypes = [vp, ctypes.c_int, P(EvamTrackCfg), P(vp)]
    lib.evam_pp_tracker_create.restype = ctypes.c_int
    lib.evam_pp_tracker_destroy.argtypes = [vp]
    lib.evam_pp_tracker_destroy.restype = None
    lib.evam_pp_tracker_reset.argtypes = [vp, vp, ctypes.c_int]
    lib.evam_pp_tracker_reset.restype = ctypes.c_int
    lib.evam_pp_tracker_read.argtypes = [vp, vp, ctypes.c_int, P(EvamTrackState)]
    lib.evam_pp_tracker_read.restype = ctypes.c_int
    lib.evam_pp_track_device_rois.argtypes = [vp, vp, P(EvamRoiList), vp, ctypes.c_int, P(EvamTrackItem), vp,
                                              ctypes.c_int, ctypes.c_int, vp, P(EvamRoiList)]
    lib.evam_pp_track_device_rois.restype = ctypes.c_int
    lib.evam_pp_ssd_rois_ex.argtypes = [vp] + ssd + [vp]
    lib.evam_pp_ssd_rois_ex.restype = ctypes.c_int
    if not hasattr(lib, "evam_pp_detection_output"):  # an A/B variant built before DetectionOutput
        return lib
    det = [vp, vp, vp, ctypes.c_int, ctypes.c_int, P(EvamDetoutCfg), vp, vp]
    lib.evam_pp_detection_output.argtypes = [vp] + det
    lib.evam_pp_detection_output.restype = ctypes.c_int
    lib.evam_pp_detection_output_host.argtypes = det
    lib.evam_pp_detection_output_host.restype = ctypes.c_int
    lib.evam_pp_expf.argtypes = [ctypes.c_float]
    lib.evam_pp_expf.restype = ctypes.c_float
    return lib


def load_library(path: str | None = None) -> ctypes.CDLL:
    """Load the in-tree HIP library. Raises RuntimeError when it is missing — there is no fallback."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    import torch  # noqa: F401  (binds the library to torch's HIP runtime; see module docstring)

    p = path or LIB_PATH
    ab = os.environ.get("EVAM_PP_LIB")
    if path is None and ab:
        # A/B runs only: a variant of this library built by tools/build_variant.sh into <repo>/ab/. Anything
        # else is refused, and the swap is announced, so a stray setting cannot silently replace the product.
        ab_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(LIB_PATH))), "ab")
        real = os.path.realpath(ab)
        if os.path.dirname(real) != os.path.realpath(ab_dir) or not os.path.basename(real).startswith("libevam_pp_"):
            raise RuntimeError(f"EVAM_PP_LIB={ab}: only variant builds in {ab_dir} (tools/build_variant.sh) are loaded")
        print(f"[evam_pp] EVAM_PP_LIB: loading the A/B variant {real}", file=sys.stderr)
        p = real
    if not os.path.exists(p):
        raise RuntimeError(
            f"{LIB_NAME} is not built at {p}: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP backend has no CPU fallback)")
    lib = _declare(ctypes.CDLL(p))
    if lib.evam_pp_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{p}: ABI version {lib.evam_pp_abi_version()} != expected {ABI_VERSION}")
    if path is None:
        _LIB = lib
    return lib


def jpeg_header(width: int, height: int, quality: int) -> bytes:
    """The 623 header bytes (SOI .. SOS) of a file ``evam_pp_encode_jpeg`` writes. Host-only."""
    lib = load_library()
    buf = (ctypes.c_uint8 * JPEG_HEADER_LEN)()
    n = ctypes.c_size_t()
    check(lib, lib.evam_pp_jpeg_header(int(width), int(height), int(quality), buf, JPEG_HEADER_LEN, ctypes.byref(n)))
    return bytes(buf[:n.value])


def jpeg_bound(width: int, height: int) -> int:
    """Worst-case bytes of one encoded ``width`` x ``height`` frame, header and EOI included. Host-only."""
    n = int(load_library().evam_pp_jpeg_bound(int(width), int(height)))
    if n == 0:
        raise PreProcError(ERR_INVALID_ARG, f"jpeg_bound: bad frame size {width}x{height}")
    return n


def _file_bytes(file) -> bytes:
    if isinstance(file, bytes):
        return file
    if isinstance(file, (bytearray, memoryview)):
        return bytes(file)
    raise PreProcError(ERR_INVALID_ARG, f"a JPEG file is bytes, bytearray or memoryview, not {type(file).__name__}")


def jpeg_file_arrays(files):
    """``(kept bytes objects, const uint8_t*[n], size_t[n])`` of a sequence of JPEG files for the decode calls."""
    keep = [_file_bytes(f) for f in files]
    n = len(keep)
    ptrs = (ctypes.c_void_p * max(n, 1))()
    lens = (ctypes.c_size_t * max(n, 1))()
    for i, b in enumerate(keep):
        ptrs[i] = ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)
        lens[i] = len(b)
    return keep, ptrs, lens


def jpeg_info_struct(file) -> EvamJpegInfo:
    """``evam_pp_jpeg_info`` of one file (bytes-like). Raises PreProcError for a refused file. Host-only."""
    lib = load_library()
    b = _file_bytes(file)
    info = EvamJpegInfo()
    check(lib, lib.evam_pp_jpeg_info(ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p), len(b), ctypes.byref(info)))
    return info


def decode_jpeg_host(files, fourcc: int = FOURCC_BGRX, pad: int = 0):
    """``evam_pp_decode_jpeg_host``: decode files of one geometry on the host.

    Returns ``(uint8 [n, H, pitch] array, pitch, int32 [n] status)``; the pitch is the row bytes rounded up to 16 plus
    ``pad`` (a multiple of 16), and the bytes behind each row's pixels keep the value 0xA5. Host-only."""
    import numpy as np

    lib = load_library()
    keep, ptrs, lens = jpeg_file_arrays(files)
    n = len(keep)
    info = jpeg_info_struct(keep[0]) if n else EvamJpegInfo()
    bpp = 3 if fourcc == FOURCC_BGR else 4
    pitch = (info.width * bpp + 15) // 16 * 16 + int(pad)
    raw = np.full(n * info.height * pitch + 16, 0xA5, np.uint8)
    off = (-raw.ctypes.data) % 16
    buf = raw[off:off + n * info.height * pitch].reshape(n, info.height, pitch)
    imgs = (EvamImage * max(n, 1))()
    for i in range(n):
        imgs[i].fourcc, imgs[i].width, imgs[i].height = fourcc, info.width, info.height
        imgs[i].pitch[0] = pitch
        imgs[i].planes[0] = buf[i].ctypes.data
    status = np.full(max(n, 1), 0x7FFFFFFF, np.int32)
    check(lib, lib.evam_pp_decode_jpeg_host(ptrs, lens, n, imgs, status.ctypes.data))
    return buf, pitch, status[:n]


def jpeg_planes_ok(info) -> bool:
    """True when ``evam_pp_decode_jpeg_planes`` serves a file of this header (a ``jpeg_info`` result or the ctypes
    struct): three components, luma sampling (2,2), even width and height. Any other file decodes to BGR / BGRX."""
    return (info.components == 3 and info.h_samp == 2 and info.v_samp == 2 and info.width % 2 == 0
            and info.height % 2 == 0)


def decode_jpeg_planes_host(files, fourcc: int = FOURCC_NV12):
    """``evam_pp_decode_jpeg_planes_host``: the raw planes of 4:2:0 files of one geometry, decoded on the host.

    Returns ``([per file: list of compact uint8 planes], int32 [n] status)``: NV12 ``[Y [H, W], UV [H/2, W]]``, I420
    ``[Y [H, W], U [H/2, W/2], V [H/2, W/2]]``. Host-only."""
    import numpy as np

    lib = load_library()
    keep, ptrs, lens = jpeg_file_arrays(files)
    n = len(keep)
    info = jpeg_info_struct(keep[0]) if n else EvamJpegInfo()
    w, h = info.width, info.height
    dims = [(h, w), (h // 2, w)] if fourcc == FOURCC_NV12 else [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    imgs = (EvamImage * max(n, 1))()
    bufs = []
    for i in range(n):
        imgs[i].fourcc, imgs[i].width, imgs[i].height = fourcc, w, h
        bufs.append([])
        for p, (rows, row) in enumerate(dims):
            pitch = (row + 15) // 16 * 16
            raw = np.zeros(max(rows, 1) * max(pitch, 16) + 16, np.uint8)
            off = (-raw.ctypes.data) % 16
            bufs[i].append(raw[off:off + rows * pitch].reshape(rows, pitch))
            imgs[i].pitch[p] = pitch
            imgs[i].planes[p] = raw.ctypes.data + off
    status = np.full(max(n, 1), 0x7FFFFFFF, np.int32)
    check(lib, lib.evam_pp_decode_jpeg_planes_host(ptrs, lens, n, imgs, status.ctypes.data))
    planes = [[np.ascontiguousarray(b[:, :row]) for b, (_, row) in zip(bufs[i], dims)] for i in range(n)]
    return planes, status[:n]


def transforms_array(transforms, n: int):
    """``evam_transform[n]`` of a sequence of transforms (objects with the struct's fields), or None for None (every
    item a plain full-frame resize). A ctypes array of EvamTransform passes through."""
    if transforms is None:
        return None
    if isinstance(transforms, ctypes.Array) and transforms._type_ is EvamTransform:
        arr = transforms
    else:
        raw = getattr(transforms, "_xf", None)  # preproc.Transforms: the array evam_pp_run filled
        if isinstance(raw, ctypes.Array) and raw._type_ is EvamTransform:
            arr = raw
        else:
            arr = (EvamTransform * len(transforms))()
            for i, t in enumerate(transforms):
                a = arr[i]
                a.scale_x, a.scale_y = t.scale_x, t.scale_y
                a.crop_x, a.crop_y, a.crop_w, a.crop_h = t.crop_x, t.crop_y, t.crop_w, t.crop_h
                a.pad_x, a.pad_y, a.resized_w, a.resized_h = t.pad_x, t.pad_y, t.resized_w, t.resized_h
    if len(arr) != n:
        raise PreProcError(ERR_INVALID_ARG, f"{len(arr)} transforms for {n} items")
    return arr


def ssd_rois_host(det, sizes, transforms, tensor_size, threshold: float, labels=None, cap: int | None = None):
    """``evam_pp_ssd_rois_host``: the rects a gvaclassify stage crops from an SSD output, on the host.

    ``det``: float32 ``[n, K, 7]``; ``sizes``: ``(width, height)`` of every item's frame; ``transforms``: None or one
    per item; ``tensor_size``: ``(W, H)`` of the detector's input; ``labels``: accepted label ids or None.
    Returns ``(int32 [min(count, cap), 5] rows of (src_index, x, y, w, h), count)``. Host-only."""
    import numpy as np

    lib = load_library()
    a = np.ascontiguousarray(det, dtype=np.float32)
    a = a.reshape(a.shape[0], -1, 7)
    n, k = int(a.shape[0]), int(a.shape[1])
    if len(sizes) != n:
        raise PreProcError(ERR_INVALID_ARG, f"{len(sizes)} frame sizes for {n} items")
    srcs = (EvamImage * max(n, 1))()
    for i, (w, h) in enumerate(sizes):
        srcs[i].width, srcs[i].height = int(w), int(h)
    xf = transforms_array(transforms, n)
    cap = n * k if cap is None else int(cap)
    rois = np.full((max(cap, 1), 5), -1, np.int32)
    count = ctypes.c_uint32(0)
    lab = None if labels is None else np.ascontiguousarray(list(labels), dtype=np.int32)
    lst = EvamRoiList(rois.ctypes.data, ctypes.addressof(count), cap, 0)
    check(lib, lib.evam_pp_ssd_rois_host(
        a.ctypes.data, n, k, srcs, xf, int(tensor_size[0]), int(tensor_size[1]), float(threshold),
        None if lab is None else lab.ctypes.data_as(ctypes.POINTER(c_i32)), 0 if lab is None else int(lab.size),
        ctypes.byref(lst)))
    return rois[:min(int(count.value), cap)].copy(), int(count.value)


TRACKING_TYPES = {"zero-term-imageless": 0, "short-term-imageless": 8}  # gvatrack tracking-type -> max_lost
TRACK_IOU_THRESHOLD = 0.3


def track_cfg(tracking_type=None, iou_threshold: float = TRACK_IOU_THRESHOLD) -> EvamTrackCfg:
    """The ``evam_track_cfg`` of a gvatrack element's ``tracking-type`` (absent: ``short-term-imageless``). The types
    that need image features (``zero-term``, ``short-term``) are ``ERR_UNSUPPORTED``; an unknown one is
    ``ERR_INVALID_ARG``."""
    kind = "short-term-imageless" if tracking_type in (None, "") else str(tracking_type)
    if kind in ("zero-term", "short-term"):
        raise PreProcError(ERR_UNSUPPORTED, f"tracking-type {kind!r} needs image features, which this tracker does not "
                                            f"compute; use {' or '.join(sorted(TRACKING_TYPES))}")
    if kind not in TRACKING_TYPES:
        raise PreProcError(ERR_INVALID_ARG, f"tracking-type {kind!r} is not one of {', '.join(sorted(TRACKING_TYPES))}")
    return EvamTrackCfg(TRACKING_TYPES[kind], float(iou_threshold))


def classify_set_args(classify_labels):
    """``(kept array, pointer, n)`` of a gate's label set: None is no gate, ``"all"`` every label, else label ids."""
    import numpy as np

    if classify_labels is None:
        return None, None, 0
    if isinstance(classify_labels, str):
        if classify_labels != "all":
            raise PreProcError(ERR_INVALID_ARG, f"classify_labels {classify_labels!r}: None, \"all\" or label ids")
        return None, None, -1
    a = np.ascontiguousarray(list(classify_labels), dtype=np.int32)
    keep = a if a.size else np.zeros(1, np.int32)
    return keep, ctypes.c_void_p(keep.ctypes.data), int(a.size)


class HostTracker:
    """One stream's tracker on the host (``evam_pp_track_host``): the state lives in this object. Needs no GPU."""

    def __init__(self, tracking_type=None, iou_threshold: float = TRACK_IOU_THRESHOLD, cfg: EvamTrackCfg | None = None):
        self._lib = load_library()
        self.cfg = cfg if cfg is not None else track_cfg(tracking_type, iou_threshold)
        self.state = EvamTrackState()

    def reset(self):
        self.state = EvamTrackState()

    def step(self, frame: int, boxes, labels, classify_labels=None, reclassify: int = 1):
        """One frame: ``boxes`` ``[n, 4]`` rows of (x, y, w, h) and ``labels`` ``[n]`` in list order. Returns
        ``(uint32 [n] ids, bool [n] due)``; ``classify_labels`` as for :func:`classify_set_args`."""
        import numpy as np

        b = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
        n = len(b)
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if len(lab) != n:
            raise PreProcError(ERR_INVALID_ARG, f"{len(lab)} labels for {n} boxes")
        rois = np.zeros((max(n, 1), 5), np.int32)
        rois[:n, 1:] = b
        ids = np.zeros(max(n, 1), np.uint32)
        due = np.zeros(max(n, 1), np.uint8)
        keep, ptr, n_set = classify_set_args(classify_labels)
        check(self._lib, self._lib.evam_pp_track_host(
            ctypes.byref(self.state), ctypes.byref(self.cfg), int(frame), rois.ctypes.data, lab.ctypes.data if n else None,
            n, ptr, n_set, int(reclassify), ids.ctypes.data, due.ctypes.data))
        return ids[:n], due[:n].astype(bool)


def track_state_tuple(state: EvamTrackState):
    """``(next_id, [(id, label, x, y, w, h, lost, classified_at) per slot])`` of a state; a zeroed (never used) state
    reads as the fresh state it stands for."""
    if state.next_id == 0:
        return 1, [(0, 0, 0, 0, 0, 0, 0, TRACK_NONE)] * TRACK_SLOTS
    return int(state.next_id), [(int(s.id), int(s.label), int(s.x), int(s.y), int(s.w), int(s.h), int(s.lost),
                                 int(s.classified_at)) for s in state.slots]


# OpenVINO DetectionOutput-1 attributes the rule has one served value for (include/evam_pp.h): name -> that value
_DETOUT_FIXED = {"code_type": "caffe.PriorBoxParameter.CENTER_SIZE", "share_location": True, "normalized": True,
                 "variance_encoded_in_target": False, "clip_before_nms": False, "clip_after_nms": False,
                 "decrease_label_id": False}
# ... and those that do not change the result for that set (read and ignored)
_DETOUT_IGNORED = ("input_height", "input_width", "objectness_score")


def _detout_bool(name: str, v) -> bool:
    if isinstance(v, str):
        t = v.strip().lower()
        if t in ("true", "1"):
            return True
        if t in ("false", "0"):
            return False
        raise PreProcError(ERR_INVALID_ARG, f"detection_output: {name} {v!r} is no boolean")
    return bool(v)


@dataclasses.dataclass(frozen=True)
class DetectionOutputConfig:
    """The attributes of an SSD ``DetectionOutput`` layer that ``evam_pp_detection_output`` serves (``evam_detout_cfg``).
    Build it with :meth:`from_attributes` from the OpenVINO attribute names."""

    num_classes: int
    keep_top_k: int
    background_label: int = 0
    top_k: int = 400
    confidence_threshold: float = 0.01
    nms_threshold: float = 0.45

    @classmethod
    def from_attributes(cls, attrs: dict) -> "DetectionOutputConfig":
        """From a dict of OpenVINO ``DetectionOutput-1`` attributes: ``num_classes`` and ``keep_top_k`` (an int or a
        one-element list) are required; ``background_label_id`` (0), ``top_k`` (400), ``confidence_threshold`` (0.01)
        and ``nms_threshold`` (0.45) have the defaults of the reference's detectors. Every attribute set the rule does
        not serve is refused with ``ERR_UNSUPPORTED`` and the reason; an unknown attribute or a value outside the
        limits with ``ERR_INVALID_ARG``."""
        if not isinstance(attrs, dict):
            raise PreProcError(ERR_INVALID_ARG, f"detection_output: the attributes are a dict, not {type(attrs).__name__}")
        a = dict(attrs)
        for name in _DETOUT_IGNORED:
            a.pop(name, None)
        for name, served in _DETOUT_FIXED.items():
            if name not in a:
                continue
            v = a.pop(name)
            if name == "code_type":
                if str(v).rsplit(".", 1)[-1].upper() != "CENTER_SIZE":
                    raise PreProcError(ERR_UNSUPPORTED, f"detection_output: code_type {v!r} is not served; only "
                                                        f"CENTER_SIZE box deltas are decoded")
            elif _detout_bool(name, v) != served:
                raise PreProcError(ERR_UNSUPPORTED, f"detection_output: {name} = {v!r} is not served; the rule is "
                                                    f"defined for {name} = {str(served).lower()} only")
        for name in ("num_classes", "keep_top_k"):
            if name not in a:
                raise PreProcError(ERR_INVALID_ARG, f"detection_output: the attribute {name} is required")
        keep = a.pop("keep_top_k")
        if isinstance(keep, (list, tuple)):
            if len(keep) != 1:
                raise PreProcError(ERR_UNSUPPORTED, f"detection_output: keep_top_k {keep!r}: one value is served")
            keep = keep[0]
        try:
            cfg = cls(num_classes=int(a.pop("num_classes")), keep_top_k=int(keep),
                      background_label=int(a.pop("background_label_id", 0)), top_k=int(a.pop("top_k", 400)),
                      confidence_threshold=float(a.pop("confidence_threshold", 0.01)),
                      nms_threshold=float(a.pop("nms_threshold", 0.45)))
        except (TypeError, ValueError) as e:
            raise PreProcError(ERR_INVALID_ARG, f"detection_output: {e}") from None
        if a:
            raise PreProcError(ERR_INVALID_ARG, f"detection_output: unknown attribute(s) {', '.join(sorted(a))}")
        for name in ("top_k", "keep_top_k"):
            if getattr(cfg, name) == -1:
                raise PreProcError(ERR_UNSUPPORTED, f"detection_output: {name} = -1 (\"all\") is not served; give a "
                                                    f"value in 1..{DETOUT_MAX_TOP_K}")
        cfg.check()
        return cfg

    def check(self) -> None:
        """The limits of ``include/evam_pp.h`` that do not depend on a call's shapes."""
        import math

        def bad(msg):
            raise PreProcError(ERR_INVALID_ARG, "detection_output: " + msg)

        if not 2 <= self.num_classes <= DETOUT_MAX_CLASSES:
            bad(f"num_classes {self.num_classes} outside 2..{DETOUT_MAX_CLASSES}")
        if not -1 <= self.background_label < self.num_classes:
            bad(f"background_label_id {self.background_label} outside -1..{self.num_classes - 1}")
        for name in ("top_k", "keep_top_k"):
            if not 1 <= getattr(self, name) <= DETOUT_MAX_TOP_K:
                bad(f"{name} {getattr(self, name)} outside 1..{DETOUT_MAX_TOP_K}")
        if not (math.isfinite(self.confidence_threshold) and self.confidence_threshold >= 0):
            bad(f"confidence_threshold {self.confidence_threshold} must be finite and >= 0")
        if not math.isfinite(self.nms_threshold):
            bad(f"nms_threshold {self.nms_threshold} must be finite")

    def to_c(self) -> EvamDetoutCfg:
        return EvamDetoutCfg(int(self.num_classes), int(self.background_label), int(self.top_k), int(self.keep_top_k),
                             float(self.confidence_threshold), float(self.nms_threshold))


def _detout_cfg(cfg) -> EvamDetoutCfg:
    if isinstance(cfg, EvamDetoutCfg):
        return cfg
    if isinstance(cfg, dict):
        cfg = DetectionOutputConfig.from_attributes(cfg)
    if not isinstance(cfg, DetectionOutputConfig):
        raise PreProcError(ERR_INVALID_ARG, f"detection_output: cfg is a DetectionOutputConfig or a dict of attributes, "
                                            f"not {type(cfg).__name__}")
    return cfg.to_c()


def detout_shapes(loc_shape, conf_shape, priors_shape, num_classes: int):
    """``(n, p)`` of raw SSD heads: ``loc`` ``[N, P*4]`` or ``[N, P, 4]``, ``conf`` ``[N, P*C]`` or ``[N, P, C]``,
    ``priors`` ``[2, P*4]``, ``[1, 2, P*4]`` or ``[2, P, 4]``. ``ERR_INVALID_ARG`` when they do not agree."""
    def numel(shape):
        k = 1
        for d in shape:
            k *= int(d)
        return k

    def bad(msg):
        raise PreProcError(ERR_INVALID_ARG, "detection_output: " + msg)

    if len(loc_shape) not in (2, 3) or len(conf_shape) not in (2, 3):
        bad(f"loc {tuple(loc_shape)} / conf {tuple(conf_shape)}: [N, P*4] / [N, P*C] (or [N, P, 4] / [N, P, C]) expected")
    n = int(loc_shape[0])
    if n < 1 or int(conf_shape[0]) != n:
        bad(f"loc {tuple(loc_shape)} and conf {tuple(conf_shape)} differ in their batch size")
    per = numel(loc_shape[1:])
    if per % 4 or per == 0 or (len(loc_shape) == 3 and int(loc_shape[2]) != 4):
        bad(f"loc {tuple(loc_shape)}: four deltas per prior expected")
    p = per // 4
    if numel(conf_shape[1:]) != p * num_classes or (len(conf_shape) == 3 and int(conf_shape[2]) != num_classes):
        bad(f"conf {tuple(conf_shape)}: {p} priors x {num_classes} classes expected")
    ps = tuple(int(d) for d in priors_shape)
    if ps[:1] == (1,) and len(ps) > 2:
        ps = ps[1:]
    if numel(ps) != 2 * p * 4 or ps[0] != 2 or (len(ps) == 3 and ps[2] != 4) or len(ps) not in (2, 3):
        bad(f"priors {tuple(priors_shape)}: [2, {p * 4}] (boxes, then variances) expected")
    return n, p


def detection_output_host(loc, conf, priors, cfg):
    """``evam_pp_detection_output_host``: SSD DetectionOutput of raw heads on numpy arrays (shapes as for
    :func:`detout_shapes`; float32, other float types are converted). ``cfg``: a :class:`DetectionOutputConfig` or a
    dict of attributes. Returns ``(float32 [N, keep_top_k, 7] blob, uint32 [N] survivor counts)``. Needs no GPU."""
    import numpy as np

    lib = load_library()
    c = _detout_cfg(cfg)
    a = np.ascontiguousarray(loc, dtype=np.float32)
    b = np.ascontiguousarray(conf, dtype=np.float32)
    pr = np.ascontiguousarray(priors, dtype=np.float32)
    n, p = detout_shapes(a.shape, b.shape, pr.shape, c.num_classes)
    k = max(int(c.keep_top_k), 1)
    out = np.full((n, k, 7), np.nan, np.float32)
    counts = np.full(n, 0xFFFFFFFF, np.uint32)
    check(lib, lib.evam_pp_detection_output_host(a.ctypes.data, b.ctypes.data, pr.ctypes.data, n, p, ctypes.byref(c),
                                                 out.ctypes.data, counts.ctypes.data))
    return out, counts


def expf(x: float) -> float:
    """``evam_pp_expf``: the exp the DetectionOutput decode uses (the same bits on the host and the device)."""
    return float(load_library().evam_pp_expf(float(x)))


class PreProcError(RuntimeError):
    """A failed evam_pp call; ``status`` is the evam_pp_status code (mirrors DLS throwing runtime_error)."""

    def __init__(self, status: int, message: str):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")


def check(lib: ctypes.CDLL, rc: int) -> None:
    if rc != OK:
        raise PreProcError(rc, lib.evam_pp_last_error().decode(errors="replace"))
