"""hkp — host runtime of the MI355X-native keypoint-heatmap path.

_lib      ctypes binding of libhulkkp.so (include/hulkkp.h)
ops       tensor-level kernel wrappers
net       network executor over the reference-shaped module tree
autograd  the autograd.Function that runs the backward kernels
resample  antialiased resize of uint8 images of any size (axis tables, plans, label maps)
metrics   keypoint evaluation on the device (KeypointMetrics: PCK, precision, AP, mean error)
tta       test-time augmentation: views of a batch and the merge of their low-res logits
grouping  associative-embedding tags: default group labels and the pairing scores
lines     line labels: segments from points and polylines, and LineMetrics for a centreline plane
"""
from ._lib import HkpError, LIB_PATH, lib, version  # noqa: F401
