"""jpeggpu_amd -- MI355X-native baseline JPEG decoder behind the jpeggpu C API.

The product is the C-ABI shared library (include/jpeggpu/jpeggpu.h, built from jpeggpu_amd/csrc by
hipcc for gfx950). This package is the thin host-side mirror used by the tests and the benchmark:
ctypes bindings with the reference's function names, argument meaning and status codes.
"""
from .api import (  # noqa: F401
    IMAGE_LAYOUTS,
    TENSOR_TYPES,
    Batch,
    ColorSpace,
    CropInfo,
    Decoder,
    ImgInfo,
    JpegGpuError,
    ProgressiveInfo,
    RgbItem,
    ScaleInfo,
    Status,
    TensorSpec,
    batch_to_rgb,
    crop_to_rgb,
    decode_batch_to_rgb,
    decode_to_planes,
    decode_resized,
    decode_to_rgb,
    draft_scale,
    fused_tail_timeouts,
    lib,
    orient_rect,
    orient_size,
    parse_headers,
    planes_to_rgb,
    resize_scratch_size,
    resize_to_rgb,
    resize_to_tensor,
    resize_weights,
    self_test,
    status_string,
)
