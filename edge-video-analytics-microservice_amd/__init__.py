"""MI355X-native pre-process backend for EVAM (Edge Video Analytics Microservice).

The directory name contains hyphens, so import it with importlib::

    import importlib
    evam = importlib.import_module("edge-video-analytics-microservice_amd")

After the first import the package is also reachable as ``evam_amd`` (``sys.modules`` alias).

Scope: decoded NV12/I420/BGRx/BGR frames -> colour conversion -> INTER_LINEAR /
letterbox / central-crop resize -> ROI crop-resize -> normalisation -> NCHW (planar) or NHWC (interleaved:
``torch.channels_last`` tensors, ``HipPreProcessor.export_bgr`` frames) batch packing, baseline JPEG encoding of the published frame
(``HipPreProcessor.encode_jpeg``) and baseline JPEG decoding of source frames (``HipPreProcessor.decode_jpeg``), as
hand-written HIP kernels for gfx950 behind the C ABI in ``include/evam_pp.h``.
"""
import sys as _sys

from ._native import (DetectionOutputConfig, HostTracker, PreProcError, detection_output_host, jpeg_bound,  # noqa: F401
                      jpeg_header, jpeg_planes_ok, load_library)
from .preproc import (DeviceRoiList, DeviceTracker, HipPreProcessor, Image, ImageBatch, JpegInfo, PreProcInfo, Roi,  # noqa: F401
                      RoiBatch, Transform, create_preprocessor, jpeg_info, output_dtype, plane_layout, tensor_layout)
from . import _native as native  # noqa: F401
from . import streams  # noqa: F401
from . import postproc  # noqa: F401
from . import feed  # noqa: F401
from . import pipeline_server  # noqa: F401

_sys.modules.setdefault("evam_amd", _sys.modules[__name__])
