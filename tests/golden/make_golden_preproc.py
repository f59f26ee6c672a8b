"""Frame indices per segment from the reference's own GenerateMultipleSegments (import placeholders of ref_harness)."""
import os
import sys

import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_harness
sys.path.insert(0, ref_harness.REFERENCE_ROOT)
from models.data.transforms.video_transforms import GenerateMultipleSegments
out = {}
cases = [(64, 16, 1.0), (70, 16, 1.0), (64, 16, 0.5), (16, 16, 1.0), (77, 16, 0.5), (100, 16, 1.0)]
for i, (T, F, step) in enumerate(cases):
    vid = torch.arange(T).view(T, 1, 1, 1).expand(T, 3, 2, 2).contiguous()
    item = {"video": vid, "meta": {"video": {"fps": [25]}}, "path": "x"}
    r = GenerateMultipleSegments(F, step_size_seg=step)(item)["video"]
    out[f"case{i}_T_F_step"] = np.array([T, F, step], np.float64)
    out[f"case{i}_frames"] = r[:, :, 0, 0, 0].numpy().astype(np.int32)
    print(T, F, step, r.shape, r[:, 0, 0, 0, 0].tolist())
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "preproc_segments.npz"), **out)
