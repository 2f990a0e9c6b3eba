"""Host-side mirror of DL Streamer's pre-processor interface, backed by the HIP kernels.

Reference interface (third party, DL Streamer 2022.1, selected by EVAM's pipeline templates
``pipelines/object_detection/vehicle/pipeline.json:5``,
``pipelines/object_classification/vehicle_attributes/pipeline.json:4-5``,
``pipelines/action_recognition/general/pipeline.json:3-4``):

* ``Image`` — DLS ``InferenceBackend::Image`` (format, width, height, planes, stride, rect);
* ``PreProcInfo`` — DLS ``InputImageLayerDesc`` built from a model-proc ``input_preproc`` entry
  (``models_list/vehicle-detection-0202.json:3`` = defaults, ``models_list/action-recognition-0001.json:3-13``
  = BGR + aspect-ratio + central crop);
* ``Transform`` — DLS ``ImageTransformationParams`` (scale / crop / padding for post-proc);
* ``HipPreProcessor.convert`` — DLS ``ImagePreprocessor::Convert`` batched over frames and ROIs.
  Failures raise :class:`PreProcError` (DLS throws ``std::runtime_error``).

There is no CPU fallback: if ``libevam_pp.so`` is missing the constructor raises.
"""
from __future__ import annotations

import ctypes
import weakref
from collections.abc import Sequence as _SequenceABC
from dataclasses import dataclass, field
from typing import Iterable, Sequence

from . import _native as N
from ._native import PreProcError  # noqa: F401  (re-export)

FOURCC_BY_NAME = {"NV12": N.FOURCC_NV12, "I420": N.FOURCC_I420, "BGRX": N.FOURCC_BGRX,
                  "BGRA": N.FOURCC_BGRA, "BGR": N.FOURCC_BGR}
NAME_BY_FOURCC = {v: k for k, v in FOURCC_BY_NAME.items()}


def plane_layout(fourcc: int, width: int, height: int, pitch_align: int = 64):
    """[(rows, pitch)] for each plane of a frame; pitches rounded up to ``pitch_align`` bytes."""
    al = lambda n: (n + pitch_align - 1) // pitch_align * pitch_align  # noqa: E731
    if fourcc == N.FOURCC_NV12:
        return [(height, al(width)), (height // 2, al(width))]
    if fourcc == N.FOURCC_I420:
        return [(height, al(width)), (height // 2, al(width // 2)), (height // 2, al(width // 2))]
    bpp = 3 if fourcc == N.FOURCC_BGR else 4
    return [(height, al(width * bpp))]


@dataclass
class Image:
    """A decoded frame resident in device memory (DLS ``Image``). ``planes`` are 2-D uint8 torch
    tensors of shape (rows, pitch); the tensors keep the memory alive."""

    fourcc: int
    width: int
    height: int
    planes: list = field(default_factory=list)
    _c: N.EvamImage | None = field(default=None, repr=False, compare=False)
    _cb: bytes | None = field(default=None, repr=False, compare=False)

    @property
    def pitches(self):
        return [int(p.stride(0)) for p in self.planes]

    def to_c(self) -> N.EvamImage:
        if self._c is None:
            c = N.EvamImage()
            c.fourcc, c.width, c.height = self.fourcc, self.width, self.height
            for i, p in enumerate(self.planes):
                c.pitch[i] = int(p.stride(0))
                c.planes[i] = int(p.data_ptr())
            self._c = c
        return self._c

    def c_bytes(self) -> bytes:
        """The packed ``evam_image`` (cached: an ImageBatch joins these instead of copying structs)."""
        if self._cb is None:
            self._cb = bytes(self.to_c())
        return self._cb

    @classmethod
    def alloc(cls, fourcc: int | str, width: int, height: int, device="cuda", pitch_align: int = 64):
        import torch

        fc = FOURCC_BY_NAME[fourcc] if isinstance(fourcc, str) else fourcc
        planes = [torch.empty((r, p), dtype=torch.uint8, device=device) for r, p in
                  plane_layout(fc, width, height, pitch_align)]
        return cls(fc, width, height, planes)

    @classmethod
    def from_host(cls, fourcc: int, width: int, height: int, host_planes: Sequence, device="cuda"):
        """Upload 2-D numpy planes (rows, pitch) to the device (the host->device feed)."""
        import torch

        planes = [torch.from_numpy(p).to(device) for p in host_planes]
        return cls(fourcc, width, height, planes)


class ImageBatch:
    """A list of Images marshalled once into the C array that evam_pp_run takes (keeps per-call
    host overhead flat for a fixed frame pool)."""

    def __init__(self, images: Sequence[Image]):
        self.images = list(images)
        # one join of cached packed structs: ~0.02 us per image instead of ~0.8 us for a ctypes
        # struct-by-struct array constructor (the pipeline hub marshals hundreds of frames per launch)
        self.c_array = (N.EvamImage * len(self.images)).from_buffer_copy(
            b"".join([im.c_bytes() for im in self.images]))

    def __len__(self):
        return len(self.images)


@dataclass(frozen=True)
class Roi:
    """A region of ``srcs[src_index]`` (DLS region of interest, gvaclassify)."""

    src_index: int
    x: int
    y: int
    w: int
    h: int


class RoiBatch:
    """ROIs marshalled once into the ``evam_roi`` array that evam_pp_run takes.

    Backed by a contiguous ``int32 [n, 5]`` numpy array (src_index, x, y, w, h), which has the layout
    of ``evam_roi[n]``: a detector's output converted with numpy is handed to the library without a
    per-ROI Python loop (a gvaclassify batch is ~50 ROIs per frame)."""

    def __init__(self, rois):
        import numpy as np

        if isinstance(rois, np.ndarray):
            a = rois
        else:
            a = np.array([(r.src_index, r.x, r.y, r.w, r.h) if isinstance(r, Roi) else tuple(r) for r in rois])
            if a.size == 0:
                a = np.zeros((0, 5), np.int32)
        # evam_roi is int32: refuse silent truncation (floats) and wrap-around (out-of-range int64)
        if a.dtype != np.int32:
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise PreProcError(N.ERR_INVALID_ARG, f"ROI array must hold integers, got dtype {a.dtype}")
            if a.size and (a.min() < -2**31 or a.max() > 2**31 - 1):
                raise PreProcError(N.ERR_INVALID_ARG, "ROI values outside the int32 range")
        self.array = np.ascontiguousarray(a, dtype=np.int32)
        if self.array.ndim == 1 and self.array.size == 0:
            self.array = self.array.reshape(0, 5)
        if self.array.ndim != 2 or self.array.shape[1] != 5:
            raise PreProcError(N.ERR_INVALID_ARG, f"ROI array must be [n, 5] int32, got {self.array.shape}")
        self.c_ptr = self.array.ctypes.data_as(ctypes.POINTER(N.EvamRoi))

    def __len__(self):
        return int(self.array.shape[0])


class DeviceRoiList:
    """A ROI list resident in device memory (``evam_roi_list``): ``rois`` int32 ``[cap, 5]`` rows of
    (src_index, x, y, w, h) and ``count`` int32 ``[1]`` (the number of entries its producer accepted, which may exceed
    ``cap``; the bits of a uint32). :meth:`HipPreProcessor.detections_to_rois` fills it,
    ``HipPreProcessor.convert(..., rois=<DeviceRoiList>)`` crops its entries; the host reads neither."""

    def __init__(self, cap: int, device="cuda"):
        import torch

        if int(cap) <= 0:
            raise PreProcError(N.ERR_INVALID_ARG, f"DeviceRoiList: cap must be > 0, got {cap}")
        self.cap = int(cap)
        self.rois = torch.zeros((self.cap, 5), dtype=torch.int32, device=device)
        self.count = torch.zeros((1,), dtype=torch.int32, device=device)
        self._c = N.EvamRoiList(self.rois.data_ptr(), self.count.data_ptr(), self.cap, 0)
        self.c_ref = ctypes.byref(self._c)

    @property
    def device(self):
        return self.rois.device

    def set(self, rois):
        """Fill the list from host rects (an ``int32 [n, 5]`` array or what :class:`RoiBatch` takes), n <= cap: for
        tests and for callers whose rects come from the host. Asynchronous on the current torch stream."""
        import torch

        a = RoiBatch(rois).array
        if len(a) > self.cap:
            raise PreProcError(N.ERR_INVALID_ARG, f"DeviceRoiList.set: {len(a)} rects for cap {self.cap}")
        if len(a):
            self.rois[:len(a)].copy_(torch.from_numpy(a))
        self.count.fill_(len(a))
        return self

    def __len__(self):
        return self.cap


class DeviceTracker:
    """The gvatrack states of ``n_streams`` streams in device memory (``evam_pp_tracker``), created through the handle
    ``pp`` and driven by :meth:`HipPreProcessor.track_rois` of any handle of that device: calls through different
    handles (different streams) are ordered one behind the other on the device by the tracker's own event, and the
    host never waits. ``tracking_type``: the element property (None: ``short-term-imageless``); ``zero-term`` and
    ``short-term`` are refused with ``ERR_UNSUPPORTED``."""

    def __init__(self, pp: "HipPreProcessor", n_streams: int, tracking_type=None,
                 iou_threshold: float = N.TRACK_IOU_THRESHOLD):
        self.cfg = N.track_cfg(tracking_type, iou_threshold)
        self._lib = pp._lib
        self.n_streams = int(n_streams)
        self.device = pp.device
        t = ctypes.c_void_p()
        pp._bind_stream()
        N.check(self._lib, self._lib.evam_pp_tracker_create(pp._h, self.n_streams, ctypes.byref(self.cfg), ctypes.byref(t)))
        self._t = t

    def reset(self, pp: "HipPreProcessor", stream: int):
        """Make stream slot ``stream`` fresh again (its stream ended). Asynchronous on ``pp``'s stream."""
        pp._bind_stream()
        N.check(self._lib, self._lib.evam_pp_tracker_reset(pp._h, self._t, int(stream)))

    def read_state(self, pp: "HipPreProcessor", stream: int) -> N.EvamTrackState:
        """Stream slot ``stream``'s state, behind every call issued so far. Synchronises (diagnostics and tests)."""
        st = N.EvamTrackState()
        pp._bind_stream()
        N.check(self._lib, self._lib.evam_pp_tracker_read(pp._h, self._t, int(stream), ctypes.byref(st)))
        return st

    def close(self):
        if getattr(self, "_t", None) and self._t.value:
            self._lib.evam_pp_tracker_destroy(self._t)
            self._t = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class PreProcInfo:
    """Model input pre-processing description (DLS ``InputImageLayerDesc`` from a model-proc)."""

    resize: str = "no-aspect-ratio"     # "no" | "no-aspect-ratio" | "aspect-ratio"
    crop: str | None = None             # None | "central"
    color_space: str = "BGR"            # "BGR" | "RGB"
    range: tuple | None = None          # (min, max)
    mean: tuple | None = None           # per output channel
    std: tuple | None = None            # per output channel
    placement: str = "top_left"         # letterbox placement: "top_left" | "center"
    fill: tuple = (0, 0, 0)             # u8 pad value per output channel
    precision: str | None = None        # "FP16" | "BF16": a 16-bit output tensor (opt-in); anything else: as None

    @classmethod
    def from_model_proc(cls, entry: dict | None) -> "PreProcInfo":
        """From one ``input_preproc`` entry of a DLS model-proc json (``{"format": "image", "params": {...}}``)."""
        if not entry:
            return cls()
        params = entry.get("params", entry)
        info = cls()
        if "resize" in params:
            info.resize = params["resize"]
        if "crop" in params:
            info.crop = params["crop"]
        if "color_space" in params:
            info.color_space = params["color_space"]
        if "range" in params:
            info.range = tuple(float(v) for v in params["range"])
        if "mean" in params:
            info.mean = tuple(float(v) for v in params["mean"])
        if "std" in params:
            info.std = tuple(float(v) for v in params["std"])
        if "precision" in entry or "precision" in params:
            info.precision = entry.get("precision", params.get("precision"))
        if "padding" in params:
            pad = params["padding"]
            if "fill_value" in pad:
                fv = pad["fill_value"]
                info.fill = tuple(int(v) for v in (fv if isinstance(fv, (list, tuple)) else [fv] * 3))
        return info

    def cache_key(self, out_dtype: int):
        """Hashable value of every field that reaches the C struct (lists are normalised to tuples)."""
        t = lambda v: tuple(v) if isinstance(v, list) else v  # noqa: E731
        return (self.resize, self.crop, self.color_space, t(self.range), t(self.mean), t(self.std),
                self.placement, t(self.fill), out_dtype)

    def resize_mode(self) -> int:
        if self.resize in ("no", "no-aspect-ratio", None):
            if self.crop not in (None, "", "none"):
                raise PreProcError(N.ERR_UNSUPPORTED, f"crop={self.crop!r} requires resize=aspect-ratio")
            return N.RESIZE_NO_ASPECT
        if self.resize == "aspect-ratio":
            if self.crop in (None, "", "none"):
                return N.RESIZE_ASPECT
            if self.crop == "central":
                return N.RESIZE_ASPECT_CROP
            raise PreProcError(N.ERR_UNSUPPORTED, f"crop={self.crop!r} is not supported (central only)")
        raise PreProcError(N.ERR_UNSUPPORTED, f"resize={self.resize!r} is not supported")

    def to_c(self, out_dtype: int) -> N.EvamPreproc:
        c = N.EvamPreproc()
        c.resize_mode = self.resize_mode()
        c.placement = N.PLACE_CENTER if self.placement == "center" else N.PLACE_TOP_LEFT
        if self.color_space not in ("BGR", "RGB"):
            raise PreProcError(N.ERR_UNSUPPORTED, f"color_space={self.color_space!r} is not supported")
        c.color_order = N.COLOR_RGB if self.color_space == "RGB" else N.COLOR_BGR
        c.out_dtype = out_dtype
        flags = 0
        c.range[0], c.range[1] = (0.0, 255.0)
        if self.range is not None:
            flags |= N.NORM_RANGE
            c.range[0], c.range[1] = self.range
        mean = self.mean or (0.0, 0.0, 0.0)
        std = self.std or (1.0, 1.0, 1.0)
        if self.mean is not None or self.std is not None:
            flags |= N.NORM_MEAN_STD
        for i in range(3):
            c.mean[i] = mean[i]
            c.std[i] = std[i]
            c.fill[i] = int(self.fill[i])
        c.norm_flags = flags
        return c


@dataclass
class Transform:
    """DLS ``ImageTransformationParams`` for one item: maps source pixels to tensor pixels."""

    scale_x: float
    scale_y: float
    crop_x: int
    crop_y: int
    crop_w: int
    crop_h: int
    pad_x: int
    pad_y: int
    resized_w: int
    resized_h: int

    def tensor_to_source(self, u: float, v: float):
        """Inverse mapping of a tensor coordinate back to source-frame coordinates (for boxes)."""
        return ((u - self.pad_x) / self.scale_x + self.crop_x, (v - self.pad_y) / self.scale_y + self.crop_y)


class Transforms(_SequenceABC):
    """The per-item transforms of one call, built on access (a detection batch needs the transform only
    of the frames that produced detections)."""

    __slots__ = ("_xf",)

    def __init__(self, xf):
        self._xf = xf

    def __len__(self):
        return len(self._xf)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        x = self._xf[i]
        return Transform(x.scale_x, x.scale_y, x.crop_x, x.crop_y, x.crop_w, x.crop_h, x.pad_x, x.pad_y,
                         x.resized_w, x.resized_h)


_PRECISION_DTYPE = {"FP16": N.DTYPE_F16, "BF16": N.DTYPE_BF16}
_DTYPE_PRECISION = {v: k for k, v in _PRECISION_DTYPE.items()}


def _pair_dtype(code: int, precision) -> int:
    """The pairing rule of :func:`output_dtype` on a tensor's own dtype code."""
    want = _PRECISION_DTYPE.get(precision) if isinstance(precision, str) else None
    if code >= N.DTYPE_F16:
        if want != code:
            raise PreProcError(N.ERR_UNSUPPORTED,
                               f"a 16-bit out tensor is lossy against the reference's fp32 input and is opt-in: state "
                               f"PreProcInfo.precision={_DTYPE_PRECISION[code]!r} (got precision={precision!r})")
    elif want is not None:
        raise PreProcError(N.ERR_INVALID_ARG, f"precision={precision!r} needs a "
                                              f"{'float16' if want == N.DTYPE_F16 else 'bfloat16'} out tensor")
    return code


def output_dtype(out, info: "PreProcInfo | None" = None) -> int:
    """The ``evam_dtype`` code a call with output tensor ``out`` and ``info`` runs in.

    uint8 and float32 tensors are ``DTYPE_U8`` / ``DTYPE_F32``. 16-bit output is opt-in, because it is one more
    rounding than the fp32 tensor the reference hands its inference engine: a ``torch.float16`` / ``torch.bfloat16``
    tensor needs ``info.precision`` ``"FP16"`` / ``"BF16"`` (else ``ERR_UNSUPPORTED``), and a stated ``"FP16"`` /
    ``"BF16"`` with a tensor of any other dtype is ``ERR_INVALID_ARG``. Other ``precision`` values behave as ``None``.
    Pure: reads only the tensor's dtype and ``info``."""
    import torch

    code = {torch.uint8: N.DTYPE_U8, torch.float32: N.DTYPE_F32, torch.float16: N.DTYPE_F16,
            torch.bfloat16: N.DTYPE_BF16}.get(out.dtype)
    if code is None:
        raise PreProcError(N.ERR_UNSUPPORTED,
                           f"out dtype {out.dtype} is not supported (uint8, float32; float16, bfloat16 with precision)")
    return _pair_dtype(code, info.precision if info is not None else None)


def tensor_layout(out) -> int:
    """``LAYOUT_NCHW`` or ``LAYOUT_NHWC`` of an ``[N,3,H,W]`` output tensor (``evam_tensor.layout``).

    A contiguous tensor is planar, shapes where both formats coincide (H = W = 1) included; otherwise a tensor that
    is contiguous in ``torch.channels_last`` is interleaved (DLS ``Convert(..., make_planar=false)``); anything
    else raises ``ERR_INVALID_ARG``. Pure: reads only shape and strides, so it works on tensors of any device."""
    import torch

    if out.dim() == 4 and out.shape[1] == 3:
        if out.is_contiguous():
            return N.LAYOUT_NCHW
        if out.is_contiguous(memory_format=torch.channels_last):
            return N.LAYOUT_NHWC
    raise PreProcError(N.ERR_INVALID_ARG, "out must be a contiguous or channels-last [N,3,H,W] tensor, got "
                                          f"shape {tuple(out.shape)} strides {tuple(out.stride())}")


class HipPreProcessor:
    """The ``pre-process-backend=hip`` implementation: one handle per (device, stream-thread)."""

    backend_name = "hip"

    def __init__(self, device: int = 0, stream=None):
        import torch

        self._lib = N.load_library()
        self.device = int(device)
        self._torch = torch
        self._follow_torch_stream = stream is None
        if not torch.cuda.is_available():
            raise PreProcError(N.ERR_NO_DEVICE, "no HIP device visible (the HIP backend has no CPU fallback)")
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._stream_ptr = int(getattr(s, "cuda_stream", s) or 0)
        h = ctypes.c_void_p()
        N.check(self._lib, self._lib.evam_pp_create(self.device, ctypes.c_void_p(self._stream_ptr),
                                                     ctypes.byref(h)))
        self._h = h
        self._cfg_cache: dict = {}
        self._last_cfg = None  # (info, dtype code, its fields, byref of the C struct) of the last call
        self._tdesc: dict = {}  # id(output tensor) -> (weakref, version, data_ptr, evam_tensor, dtype code, byref)
        self._default_info = PreProcInfo()
        self._export_info: dict = {}  # color_space -> the PreProcInfo of export_bgr (identity resize, u8)
        self._jpeg_dev = None   # encode_jpeg: (uint8 [n, stride] slots, uint32 [n] sizes) on the device
        self._jpeg_host = None  # ... and their pinned host mirrors
        self._jpeg_need = {}    # (width, height) -> slot bytes, once files of that size outgrew the default slot
        self._jpeg_guess = 0    # bytes of every slot the next encode_jpeg copies to the host first
        self._run = self._lib.evam_pp_run
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        self._raw_stream = raw if raw is not None else (
            lambda d: torch.cuda.current_stream(d).cuda_stream)

    # -- lifecycle ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.evam_pp_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- options ---------------------------------------------------------------------------------
    def set_option(self, option: int, value: int):
        N.check(self._lib, self._lib.evam_pp_set_option(self._h, option, int(value)))

    def stats(self) -> N.EvamStats:
        st = N.EvamStats()
        N.check(self._lib, self._lib.evam_pp_get_stats(self._h, ctypes.byref(st)))
        return st

    def sync(self):
        N.check(self._lib, self._lib.evam_pp_sync(self._h))

    def _bind_stream(self):
        if self._follow_torch_stream:
            s = int(self._raw_stream(self.device) or 0)
            if s != self._stream_ptr:
                N.check(self._lib, self._lib.evam_pp_set_stream(self._h, ctypes.c_void_p(s)))
                self._stream_ptr = s

    def _tensor_desc(self, out, slot_offset: int, slot_stride: int):
        """``byref`` of the validated evam_tensor for ``out``, and its own dtype's code. Cached per output tensor (a stage
        packs into the same inference blob every call; a runner or a bench cycles through a few): the same tensor
        object at the same version (``resize_`` / ``set_`` / ``as_strided_`` bump it) and storage has the shape,
        dtype, device and layout it was checked with, so they are not read again (~1 us per call)."""
        e = self._tdesc.get(id(out))
        if e is None or e[0]() is not out or e[1] != out._version or e[2] != out.data_ptr():
            e = self._tensor_entry(out)
        t = e[3]
        if t.slot_offset != slot_offset or t.slot_stride != slot_stride:
            t.slot_offset, t.slot_stride = int(slot_offset), int(slot_stride)
        return e[5], e[4]

    def _check_device(self, out):
        if out.device.type != "cuda" or (out.device.index or 0) != self.device:
            raise PreProcError(N.ERR_INVALID_ARG, f"out must live on cuda:{self.device}, got {out.device}")

    def _tensor_entry(self, out):
        torch = self._torch
        layout = tensor_layout(out)
        if out.dtype == torch.uint8:
            dt = N.DTYPE_U8
        elif out.dtype == torch.float32:
            dt = N.DTYPE_F32
        elif out.dtype == torch.float16:  # the 16-bit types: convert() pairs them with info.precision
            dt = N.DTYPE_F16
        elif out.dtype == torch.bfloat16:
            dt = N.DTYPE_BF16
        else:
            raise PreProcError(N.ERR_UNSUPPORTED,
                               f"out dtype {out.dtype} is not supported (uint8, float32; float16, bfloat16 with precision)")
        self._check_device(out)
        t = N.EvamTensor()
        t.data = out.data_ptr()
        t.n, t.c, t.h, t.w = (int(v) for v in out.shape)
        t.layout = layout
        e = (weakref.ref(out), out._version, t.data, t, dt, ctypes.byref(t))
        if len(self._tdesc) >= 16:
            self._tdesc.clear()
        self._tdesc[id(out)] = e
        return e

    # -- the hot path ------------------------------------------------------------------------------
    def convert(self, srcs, out, info: PreProcInfo | None = None, rois: Iterable | None = None,
                slot_offset: int = 0, slot_stride: int = 1, want_transform: bool = False, slots=None, status=None):
        """Pre-process ``srcs`` (or ``rois`` of them) into ``out`` ([N,3,H,W] uint8/float32, device; float16/bfloat16 with
        ``info.precision`` ``"FP16"`` / ``"BF16"``, see :func:`output_dtype`).

        ``srcs``: an :class:`ImageBatch` (marshalled once) or a sequence of :class:`Image`.
        ``rois``: a :class:`RoiBatch`, an ``int32 [n, 5]`` array or a sequence of :class:`Roi`; or a
        :class:`DeviceRoiList`: entry i below its count goes to slot ``slot_offset + i * slot_stride``, the slots from
        the count on are not touched, nothing is returned, and ``status`` (None or an int32 ``[cap]`` device tensor)
        receives 0 or the error of every entry (``evam_pp_run_device_rois``).
        Item i goes to slot ``slot_offset + i * slot_stride`` of ``out``, or to ``slots[i]`` when ``slots`` (one
        distinct slot per item, ``evam_pp_run_slots``) is given.
        Returns a list of :class:`Transform` when ``want_transform`` (``"lazy"``: a :class:`Transforms`
        sequence that builds each on access). Asynchronous on the current
        torch stream of ``self.device`` (or the stream given at construction).
        """
        info = info or self._default_info
        batch = srcs if isinstance(srcs, ImageBatch) else ImageBatch(srcs)
        tref, dt = self._tensor_desc(out, slot_offset, slot_stride)
        if dt >= N.DTYPE_F16 or info.precision is not None:
            _pair_dtype(dt, info.precision)  # 16-bit output is opt-in (output_dtype); raises on a mismatch
        lc = self._last_cfg
        if lc is not None and lc[0] is info and lc[1] == dt and lc[2] == info.__dict__:
            cached = lc[3]  # the last call's info object, every field as it was (~1.3 us of key building saved)
        else:
            # keyed on the field values (PreProcInfo is mutable; a field changed after a call must not reuse
            # a stale struct), bounded so callers building a new info per call cannot grow it without limit
            key = info.cache_key(dt)
            cached = self._cfg_cache.get(key)
            if cached is None:
                if len(self._cfg_cache) >= 64:
                    self._cfg_cache.clear()
                cached = ctypes.byref(info.to_c(dt))
                self._cfg_cache[key] = cached
            # snapshot of the fields for the identity check above; a list field can change in place, so an info
            # holding one takes the keyed path every call
            d = info.__dict__
            self._last_cfg = None if any(v.__class__ is list for v in d.values()) else (info, dt, dict(d), cached)
        if rois.__class__ is DeviceRoiList:
            # the rects stay on the device (evam_pp_run_device_rois): no transforms, no explicit slots
            if slots is not None or want_transform:
                raise PreProcError(N.ERR_INVALID_ARG, "convert: a DeviceRoiList takes neither slots nor want_transform")
            if status is not None:
                torch = self._torch
                if status.dtype != torch.int32 or status.dim() != 1 or status.shape[0] < rois.cap \
                        or not status.is_contiguous():
                    raise PreProcError(N.ERR_INVALID_ARG, f"convert: status must be a contiguous int32 [>= {rois.cap}] "
                                                          f"tensor, got {status.dtype} {tuple(status.shape)}")
                self._check_device(status)
            self._check_device(rois.rois)
            self._bind_stream()
            rc = self._lib.evam_pp_run_device_rois(self._h, batch.c_array, len(batch), rois.c_ref, cached, tref,
                                                   None if status is None else ctypes.c_void_p(status.data_ptr()))
            if rc:
                N.check(self._lib, rc)
            return None
        if status is not None:
            raise PreProcError(N.ERR_INVALID_ARG, "convert: status belongs to a DeviceRoiList call")
        if rois is not None:
            rb = rois if isinstance(rois, RoiBatch) else RoiBatch(rois)
            n_items = len(rb)
            if n_items == 0:
                raise PreProcError(N.ERR_INVALID_ARG, "rois is empty")
            items_p = rb.c_ptr
        else:
            n_items = len(batch)
            items_p = None
        xf = (N.EvamTransform * n_items)() if want_transform else None
        self._bind_stream()
        if slots is not None:
            import numpy as np

            sl = np.ascontiguousarray(slots, dtype=np.int32)
            if sl.shape != (n_items,):
                raise PreProcError(N.ERR_INVALID_ARG, f"slots must hold one slot per item ({n_items}), got {sl.shape}")
            rc = self._lib.evam_pp_run_slots(self._h, batch.c_array, len(batch), items_p, n_items, cached,
                                             tref, sl.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), xf)
        else:
            rc = self._run(self._h, batch.c_array, len(batch), items_p, n_items, cached, tref, xf)
        if rc:
            N.check(self._lib, rc)
        if not want_transform:
            return None
        return Transforms(xf) if want_transform == "lazy" else list(Transforms(xf))

    def detections_to_rois(self, det, frames, transforms, tensor_size, threshold: float, labels=None,
                           out_list: DeviceRoiList | None = None, out_labels=None):
        """The rects a gvaclassify stage crops from a detector's SSD output, written into a device list with no host
        round trip (``evam_pp_ssd_rois``): what ``postproc.parse_ssd_batch`` -> ``detections_to_regions`` ->
        the label filter -> ``pipeline_server.roi_inside`` give on the host, in their order.

        ``det``: a float32 device tensor ``[n, K, 7]`` or ``[n, 1, K, 7]``; ``frames``: the n frames (an
        :class:`ImageBatch` or Images; only sizes are read); ``transforms``: what ``convert(..., want_transform=...)``
        returned for the detector's input, or None (plain full-frame resizes); ``tensor_size``: ``(W, H)`` of that
        input; ``labels``: accepted label ids, or None for all; ``out_list``: the list to fill (default: a new one of
        n * K entries); ``out_labels``: None, or a contiguous int32 device tensor of at least ``out_list.cap`` elements
        that receives each entry's label id beside its rect (``evam_pp_ssd_rois_ex``; what :meth:`track_rois` takes).
        Returns the list. Asynchronous, as :meth:`convert`."""
        import numpy as np

        torch = self._torch
        batch = frames if isinstance(frames, ImageBatch) else ImageBatch(frames)
        n = len(batch)
        if det.dtype != torch.float32 or not det.is_contiguous() or det.dim() not in (3, 4) or det.shape[-1] != 7 \
                or det.shape[0] != n or (det.dim() == 4 and det.shape[1] != 1):
            raise PreProcError(N.ERR_INVALID_ARG, f"detections_to_rois: det must be a contiguous float32 [{n}, K, 7] or "
                                                  f"[{n}, 1, K, 7] tensor, got {det.dtype} {tuple(det.shape)}")
        self._check_device(det)
        k = int(det.shape[-2])
        if out_list is None:
            out_list = DeviceRoiList(n * k, device=det.device)
        self._check_device(out_list.rois)
        xf = N.transforms_array(transforms, n)
        lab = None if labels is None else np.ascontiguousarray(list(labels), dtype=np.int32)
        self._bind_stream()
        args = (self._h, ctypes.c_void_p(det.data_ptr()), n, k, batch.c_array, xf, int(tensor_size[0]), int(tensor_size[1]),
                float(threshold), None if lab is None else lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                0 if lab is None else int(lab.size), out_list.c_ref)
        if out_labels is None:
            rc = self._lib.evam_pp_ssd_rois(*args)
        else:
            self._check_i32(out_labels, out_list.cap, "detections_to_rois: out_labels")
            rc = self._lib.evam_pp_ssd_rois_ex(*args, ctypes.c_void_p(out_labels.data_ptr()))
        if rc:
            N.check(self._lib, rc)
        return out_list

    def detection_output(self, loc, conf, priors, cfg, out=None, counts=None):
        """SSD DetectionOutput of a detector's raw heads, on the device (``evam_pp_detection_output``: the rule of
        ``include/evam_pp.h``): the ``[N, keep_top_k, 7]`` blob :meth:`detections_to_rois` and
        ``postproc.parse_ssd_batch`` read.

        ``loc``: box deltas ``[N, P*4]`` (or ``[N, P, 4]``); ``conf``: class probabilities ``[N, P*C]`` (or
        ``[N, P, C]``), softmax applied; ``priors``: ``[2, P*4]`` (``[1, 2, P*4]``, ``[2, P, 4]``), boxes then variances.
        All are CUDA tensors on the handle's device; fp16 / bf16 heads are cast with ``.float()`` here, any other dtype
        and a non-contiguous tensor are ``ERR_INVALID_ARG`` (no silent copy). ``cfg``: a
        :class:`DetectionOutputConfig` or a dict of the layer's attributes. ``out``: a contiguous float32
        ``[N, keep_top_k, 7]`` tensor to fill (default: a new one); ``counts``: None, or a contiguous int32 tensor of
        ``>= N`` elements that receives each image's survivor count. Returns ``out``. Asynchronous, as
        :meth:`convert`."""
        torch = self._torch
        c = N._detout_cfg(cfg)

        def head(t, what):
            if not isinstance(t, torch.Tensor):
                raise PreProcError(N.ERR_INVALID_ARG, f"detection_output: {what} must be a tensor, got {type(t).__name__}")
            self._check_device(t)
            if not t.is_contiguous():
                raise PreProcError(N.ERR_INVALID_ARG, f"detection_output: {what} {tuple(t.shape)} is not contiguous")
            if t.dtype in (torch.float16, torch.bfloat16):
                return t.float()
            if t.dtype != torch.float32:
                raise PreProcError(N.ERR_INVALID_ARG, f"detection_output: {what} must be float32 (or fp16 / bf16), got {t.dtype}")
            return t

        loc, conf, priors = head(loc, "loc"), head(conf, "conf"), head(priors, "priors")
        n, p = N.detout_shapes(loc.shape, conf.shape, priors.shape, c.num_classes)
        k = int(c.keep_top_k)
        if out is None:
            if not 1 <= k <= N.DETOUT_MAX_TOP_K:
                raise PreProcError(N.ERR_INVALID_ARG, f"detection_output: keep_top_k {k} outside 1..{N.DETOUT_MAX_TOP_K}")
            out = torch.empty((n, k, 7), dtype=torch.float32, device=loc.device)
        else:
            self._check_device(out)
            if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n, k, 7):
                raise PreProcError(N.ERR_INVALID_ARG, f"detection_output: out must be a contiguous float32 [{n}, {k}, 7] "
                                                      f"tensor, got {out.dtype} {tuple(out.shape)}")
        if counts is not None:
            self._check_i32(counts, n, "detection_output: counts")
        self._bind_stream()
        rc = self._lib.evam_pp_detection_output(
            self._h, ctypes.c_void_p(loc.data_ptr()), ctypes.c_void_p(conf.data_ptr()), ctypes.c_void_p(priors.data_ptr()),
            n, p, ctypes.byref(c), ctypes.c_void_p(out.data_ptr()),
            None if counts is None else ctypes.c_void_p(counts.data_ptr()))
        if rc:
            N.check(self._lib, rc)
        return out

    def _check_i32(self, t, n: int, what: str):
        torch = self._torch
        if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < n:
            raise PreProcError(N.ERR_INVALID_ARG, f"{what} must be a contiguous int32 tensor of >= {n} elements, got "
                                                  f"{t.dtype} {tuple(t.shape)}")
        self._check_device(t)

    def track_rois(self, lst: DeviceRoiList, labels, tracker: DeviceTracker, items, classify_labels=None,
                   reclassify: int = 1, out_ids=None, due: DeviceRoiList | None = None):
        """Object ids for the entries of a device list, and the entries due for classification, with no host round trip
        (``evam_pp_track_device_rois``: the gvatrack rule of ``include/evam_pp.h``, one workgroup per stream).

        ``lst``: the detections of ``len(items)`` items in item order, as :meth:`detections_to_rois` writes them;
        ``labels``: int32 device tensor ``[>= lst.cap]``, each entry's label id; ``items``: per item ``(stream slot,
        frame index)``, every slot's items contiguous and in ascending frame order (else ``ERR_INVALID_ARG``);
        ``classify_labels``: None (no gate), ``"all"`` or the label ids a classify stage crops; ``reclassify``: its
        ``reclassify-interval``; ``out_ids``: int32 device tensor ``[>= lst.cap]`` to fill (the bits of uint32 ids;
        default: a new one); ``due``: None, or the list that receives the due entries in list order (its count is
        the true total, also past its cap). Returns ``out_ids``. Asynchronous, as :meth:`convert`."""
        torch = self._torch
        self._check_i32(labels, lst.cap, "track_rois: labels")
        if out_ids is None:
            out_ids = torch.zeros((lst.cap,), dtype=torch.int32, device=lst.device)
        self._check_i32(out_ids, lst.cap, "track_rois: out_ids")
        self._check_device(lst.rois)
        if due is not None:
            self._check_device(due.rois)
        n = len(items)
        tab = (N.EvamTrackItem * max(n, 1))()
        for i, (s, f) in enumerate(items):
            tab[i].stream, tab[i].frame = int(s), int(f)
        keep, ptr, n_set = N.classify_set_args(classify_labels)
        self._bind_stream()
        rc = self._lib.evam_pp_track_device_rois(
            self._h, tracker._t, lst.c_ref, ctypes.c_void_p(labels.data_ptr()), n, tab, ptr, n_set, int(reclassify),
            ctypes.c_void_p(out_ids.data_ptr()), None if due is None else due.c_ref)
        if rc:
            N.check(self._lib, rc)
        return out_ids

    def export_bgr(self, srcs, out=None, color_space: str = "BGR"):
        """The packed ``[N,H,W,3]`` uint8 image of every frame of ``srcs`` at source size, in one launch: the frame
        the reference publishes (``videoconvert ! video/x-raw,format=BGR ! appsink``), with the BT.601 arithmetic of
        the rest of this path. All frames must have one size. ``out``: an ``[N,H,W,3]`` uint8 device tensor to write
        into (returned); default: a new one. Asynchronous, as :meth:`convert`."""
        torch = self._torch
        batch = srcs if isinstance(srcs, ImageBatch) else ImageBatch(srcs)
        if len(batch) == 0:
            raise PreProcError(N.ERR_INVALID_ARG, "export_bgr: no frames")
        w, h = batch.images[0].width, batch.images[0].height
        for im in batch.images:
            if im.width != w or im.height != h:
                raise PreProcError(N.ERR_INVALID_ARG, f"export_bgr: frames of one call must share a size, got "
                                                      f"{w}x{h} and {im.width}x{im.height}")
        shape = (len(batch), h, w, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=f"cuda:{self.device}")
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous():
            raise PreProcError(N.ERR_INVALID_ARG, f"export_bgr: out must be a contiguous uint8 {shape} tensor, got "
                                                  f"{out.dtype} {tuple(out.shape)}")
        info = self._export_info.get(color_space)
        if info is None:
            info = self._export_info[color_space] = PreProcInfo(resize="no-aspect-ratio", color_space=color_space)
        self.convert(batch, out.permute(0, 3, 1, 2), info)
        return out


    # -- JPEG encoding of the published frame ------------------------------------------------------------
    @staticmethod
    def _jpeg_args(srcs, quality):
        """(ImageBatch, width, height) of an encode call; every refusal that needs no device happens here."""
        batch = srcs if isinstance(srcs, ImageBatch) else ImageBatch(srcs)
        if len(batch) == 0:
            raise PreProcError(N.ERR_INVALID_ARG, "encode_jpeg: no frames")
        if isinstance(quality, bool) or not isinstance(quality, int) or not 0 <= quality <= 100:
            raise PreProcError(N.ERR_INVALID_ARG, f"encode_jpeg: quality must be an integer in 0..100, got {quality!r}")
        w, h = batch.images[0].width, batch.images[0].height
        for im in batch.images:
            if im.width != w or im.height != h:
                raise PreProcError(N.ERR_INVALID_ARG, f"encode_jpeg: frames of one call must share a size, got "
                                                      f"{w}x{h} and {im.width}x{im.height}")
        return batch, w, h

    def encode_jpeg_into(self, srcs, out, sizes, quality: int = 95):
        """Encode every frame of ``srcs`` as a baseline JFIF file (what the reference's publisher gets from
        ``cv2.imencode('.jpg', frame, [IMWRITE_JPEG_QUALITY, quality])``) into row i of ``out`` (uint8 ``[n, stride]``,
        device, contiguous); ``sizes`` (int32 / uint32-as-int32 ``[n]``, device) receives every file's full length, also
        when it exceeds ``stride`` (that row is then incomplete: encode again with ``N.jpeg_bound``). Asynchronous, as
        :meth:`convert`."""
        batch, _, _ = self._jpeg_args(srcs, quality)  # refusals first: they need no device
        torch = self._torch
        n = len(batch)
        if out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] < n or not out.is_contiguous():
            raise PreProcError(N.ERR_INVALID_ARG, f"encode_jpeg_into: out must be a contiguous uint8 [>= {n}, stride] "
                                                  f"tensor, got {out.dtype} {tuple(out.shape)}")
        if sizes.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or sizes.dim() != 1 \
                or sizes.shape[0] < n or not sizes.is_contiguous():
            raise PreProcError(N.ERR_INVALID_ARG, f"encode_jpeg_into: sizes must be a contiguous 32-bit integer [>= {n}] "
                                                  f"tensor, got {sizes.dtype} {tuple(sizes.shape)}")
        self._check_device(out)
        self._check_device(sizes)
        self._bind_stream()
        rc = self._lib.evam_pp_encode_jpeg(self._h, batch.c_array, n, int(quality), ctypes.c_void_p(out.data_ptr()),
                                           int(out.shape[1]), ctypes.c_void_p(sizes.data_ptr()))
        if rc:
            N.check(self._lib, rc)

    def _jpeg_buffers(self, n: int, stride: int):
        torch = self._torch
        d = self._jpeg_dev
        if d is None or d[0].shape[0] < n or d[0].shape[1] < stride:
            n_cap = max(n, d[0].shape[0] if d is not None else 0)
            s_cap = max(stride, d[0].shape[1] if d is not None else 0)
            dev = f"cuda:{self.device}"
            self._jpeg_dev = (torch.empty((n_cap, s_cap), dtype=torch.uint8, device=dev),
                              torch.empty((n_cap,), dtype=torch.int32, device=dev))
            self._jpeg_host = (torch.empty((n_cap, s_cap), dtype=torch.uint8, pin_memory=True),
                               torch.empty((n_cap,), dtype=torch.int32, pin_memory=True))
        return self._jpeg_dev, self._jpeg_host

    def encode_jpeg(self, srcs, quality: int = 95) -> list:
        """The JFIF file of every frame of ``srcs`` as ``bytes``: one launch sequence, one stream synchronisation (a
        second only when the files outgrow what the last call's sizes predicted), device slots and pinned host staging
        owned by this object. A slot holds ``1024 + W16 * H16`` bytes (one per
        pixel of the frame padded to whole MCUs); frames that need more (noise at high quality) are encoded again with
        the worst-case bound, so the result is always complete; later calls at that size then start with slots a
        quarter larger than the largest such file."""
        import numpy as np

        batch, w, h = self._jpeg_args(srcs, quality)  # refusals first: they need no device
        torch = self._torch
        n = len(batch)
        stride = max(1024 + (-(-w // 16) * 16) * (-(-h // 16) * 16), self._jpeg_need.get((w, h), 0))
        (d_out, d_sizes), (h_out, h_sizes) = self._jpeg_buffers(n, stride)
        d_rows = d_out.view(-1)[:n * stride].view(n, stride)
        self.encode_jpeg_into(batch, d_rows, d_sizes, quality)
        # Only the head of every slot crosses PCIe: as many bytes as the largest file of the last call plus a quarter
        # (the whole slot the first time). A call whose files outgrow that fetches the rest in a second copy.
        g = min(stride, self._jpeg_guess or stride)
        head = d_rows if g == stride else d_rows[:, :g].contiguous()
        h_rows = h_out.view(-1)[:n * g].view(n, g)
        if not self._follow_torch_stream:  # a stream given at construction: the copies below run on torch's
            self.sync()
        h_sizes[:n].copy_(d_sizes[:n], non_blocking=True)
        h_rows.copy_(head, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        lens = h_sizes[:n].numpy().astype(np.int64) & 0xFFFFFFFF
        rows = h_rows.numpy()
        need = int(min(stride, lens.max()))
        if need > g:
            rows = np.concatenate([rows, d_rows[:, g:need].cpu().numpy()], axis=1)
        self._jpeg_guess = min(stride, -(-(need + need // 4) // 4096) * 4096)
        files = [rows[i, :lens[i]].tobytes() if lens[i] <= stride else None for i in range(n)]
        over = [i for i, f in enumerate(files) if f is None]
        if over:
            big = N.jpeg_bound(w, h)
            d_rows = torch.empty((len(over), big), dtype=torch.uint8, device=d_out.device)
            self.encode_jpeg_into([batch.images[i] for i in over], d_rows, d_sizes, quality)
            if not self._follow_torch_stream:
                self.sync()
            lens2 = d_sizes[:len(over)].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            got = d_rows[:, :int(lens2.max())].cpu().numpy()
            for k, i in enumerate(over):
                files[i] = got[k, :lens2[k]].tobytes()
            # frames of this size outgrew the default slot: the next calls start with room for them
            if len(self._jpeg_need) >= 16:
                self._jpeg_need.clear()
            top = int(lens2.max())
            self._jpeg_need[(w, h)] = min(big, -(-(top + top // 4) // 4096) * 4096)
        return files


    # -- JPEG decoding of source frames ----------------------------------------------------------------
    def decode_jpeg_into(self, files, images, status):
        """Decode ``files`` (bytes-like JPEG files of one geometry: size, components, sampling and restart interval, as
        :func:`jpeg_info` reports them) into ``images`` (device ``Image``s of that size, all of one fourcc). BGR / BGRX
        images receive libjpeg's default decode (``evam_pp_decode_jpeg``); NV12 / I420 images receive the files' raw
        4:2:0 planes (``evam_pp_decode_jpeg_planes``: 4:2:0 files of even size only, see :func:`jpeg_planes_ok`).
        ``status`` (int32 ``[n]``, device) receives 0 per file, or ``N.ERR_INVALID_ARG`` for a file whose scan is
        damaged. The bytes are staged before the call returns. Asynchronous, as :meth:`convert`."""
        torch = self._torch
        keep, ptrs, lens = N.jpeg_file_arrays(files)
        n = len(keep)
        batch = images if isinstance(images, ImageBatch) else ImageBatch(images)
        if n == 0 or len(batch) != n:
            raise PreProcError(N.ERR_INVALID_ARG, f"decode_jpeg_into: {n} files for {len(batch)} images")
        if status.dtype != torch.int32 or status.dim() != 1 or status.shape[0] < n or not status.is_contiguous():
            raise PreProcError(N.ERR_INVALID_ARG, f"decode_jpeg_into: status must be a contiguous int32 [>= {n}] tensor, "
                                                  f"got {status.dtype} {tuple(status.shape)}")
        self._check_device(status)
        self._bind_stream()
        planes = batch.images[0].fourcc in (N.FOURCC_NV12, N.FOURCC_I420)
        call = self._lib.evam_pp_decode_jpeg_planes if planes else self._lib.evam_pp_decode_jpeg
        rc = call(self._h, ptrs, lens, n, batch.c_array, ctypes.c_void_p(status.data_ptr()))
        if rc:
            N.check(self._lib, rc)

    def decode_jpeg(self, files, fourcc: int | str = "BGRX", fallback: int | str | None = None) -> list:
        """Decode JPEG files (bytes-like, any mix of geometries) to device ``Image``s of ``fourcc``, in the order
        given: one decode call per geometry group, then one read-back of all statuses (one stream synchronisation per
        call). ``fourcc`` BGRX or BGR is libjpeg's default decode; NV12 or I420 is the files' raw 4:2:0 planes, which
        only files that :func:`jpeg_planes_ok` accepts have: any other file raises ``ERR_UNSUPPORTED``, or with
        ``fallback`` ("BGRX" / "BGR") comes back decoded to that format instead. Raises :class:`PreProcError` naming
        the first refused or damaged file."""
        files = list(files)
        if not files:
            return []
        fc = FOURCC_BY_NAME[fourcc] if isinstance(fourcc, str) else int(fourcc)
        planes = fc in (N.FOURCC_NV12, N.FOURCC_I420)
        fb = None
        if fallback is not None:
            fb = FOURCC_BY_NAME.get(fallback) if isinstance(fallback, str) else int(fallback)
            if not planes or fb not in (N.FOURCC_BGRX, N.FOURCC_BGR):
                raise PreProcError(N.ERR_INVALID_ARG, f"decode_jpeg: fallback {fallback!r}: \"BGRX\" or \"BGR\", beside "
                                                      "an NV12 / I420 fourcc")
        groups: dict = {}
        for i, f in enumerate(files):
            try:
                info = N.jpeg_info_struct(f)
            except PreProcError as e:
                raise PreProcError(e.status, f"decode_jpeg: files[{i}]: {e}") from None
            key = (info.width, info.height, info.components, info.h_samp, info.v_samp, info.restart_interval)
            if planes:
                if N.jpeg_planes_ok(info):
                    key += (fc,)
                elif fb is None:
                    raise PreProcError(N.ERR_UNSUPPORTED, f"decode_jpeg: files[{i}]: {info.width}x{info.height}, "
                                       f"{info.components} components, luma sampling {info.h_samp}x{info.v_samp}: raw "
                                       f"{NAME_BY_FOURCC[fc]} planes are written for 4:2:0 files of even size only "
                                       "(pass fallback=\"BGRX\" to decode such files to pixels)")
                else:
                    key += (fb,)
            groups.setdefault(key, []).append(i)
        torch = self._torch  # the refusals above need no device
        dev = f"cuda:{self.device}"
        status = torch.empty((len(files),), dtype=torch.int32, device=dev)
        images: list = [None] * len(files)
        order: list = []
        at = 0
        for key, members in groups.items():
            imgs = [Image.alloc(key[6] if planes else fc, key[0], key[1], device=dev) for _ in members]
            self.decode_jpeg_into([files[i] for i in members], imgs, status[at:at + len(members)])
            for i, im in zip(members, imgs):
                images[i] = im
            order += members
            at += len(members)
        if not self._follow_torch_stream:  # a stream given at construction: the copy below runs on torch's
            self.sync()
        st = status.cpu().tolist()
        bad = sorted(order[k] for k, v in enumerate(st) if v != 0)
        if bad:
            raise PreProcError(N.ERR_INVALID_ARG, f"decode_jpeg: files[{bad[0]}]: the scan is not a valid baseline scan "
                                                  f"({len(bad)} of {len(files)} files damaged)")
        return images


@dataclass(frozen=True)
class JpegInfo:
    """``evam_jpeg_info``: what the markers of a JPEG file up to SOS say."""

    width: int
    height: int
    components: int
    h_samp: int
    v_samp: int
    restart_interval: int
    scan_offset: int


jpeg_planes_ok = N.jpeg_planes_ok  # re-export: which files decode_jpeg(..., "NV12" / "I420") serves


def jpeg_info(file) -> JpegInfo:
    """Parse a JPEG file's header (host only). Raises :class:`PreProcError` (``ERR_UNSUPPORTED`` / ``ERR_INVALID_ARG``
    with the reason) for a file the decoder refuses."""
    i = N.jpeg_info_struct(file)
    return JpegInfo(i.width, i.height, i.components, i.h_samp, i.v_samp, i.restart_interval, i.scan_offset)


# Backend registry keyed by the DL Streamer element property value `pre-process-backend`.
_BACKENDS = {"hip": HipPreProcessor}
REFERENCE_ONLY_BACKENDS = ("opencv", "ie", "vaapi", "vaapi-surface-sharing")


def create_preprocessor(backend: str = "hip", **kw):
    """Instantiate the pre-processor selected by a ``pre-process-backend`` property value."""
    if backend in _BACKENDS:
        return _BACKENDS[backend](**kw)
    if backend in REFERENCE_ONLY_BACKENDS:
        raise PreProcError(N.ERR_UNSUPPORTED,
                           f"pre-process-backend={backend!r} is the reference DL Streamer CPU/VA path; "
                           "this build provides 'hip'")
    raise PreProcError(N.ERR_INVALID_ARG, f"unknown pre-process-backend {backend!r}")
