"""The reference's utils/flow_viz.py surface (also networks/raft/utils/flow_viz.py and networks/gma/utils/flow_viz.py there)
over the HIP kernels: numpy in, numpy out, the colours computed on the device (accflow_amd.viz)."""
import numpy as np
import torch

from .... import viz


def flow_to_image(flow_uv, clip_flow=None, convert_to_bgr=False):
    """flow_uv: [H,W,2] ndarray -> [H,W,3] uint8 ndarray, scaled by the image's largest flow (clip_flow: np.clip(flow, 0,
    clip_flow) first)."""
    assert flow_uv.ndim == 3, "input flow must have three dimensions"
    assert flow_uv.shape[2] == 2, "input flow must have shape [H,W,2]"
    flow = torch.from_numpy(np.ascontiguousarray(flow_uv, dtype=np.float32)).permute(2, 0, 1).contiguous().cuda()
    return viz.flow_to_image(flow, clip_flow=clip_flow, convert_to_bgr=convert_to_bgr).cpu().numpy()
