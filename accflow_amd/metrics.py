"""Judging a flow: forward-backward occlusion masks and end-point-error metrics on the device.

The reference does this in three places: `calc_occ_mask` (test_cvo.py:53-78), `cal_epe` (:81-101) and the metrics half of
the sequence loss (loss.py:37-45).  Here they are two HIP launches (ops.fb_occlusion, ops.flow_metrics: fixed-order
reductions, reproducible bit for bit, a sample's numbers independent of the batch it sits in) and the divisions below.
Nothing in this module synchronises with the host: every result is a per-sample device tensor.
"""
import torch

from . import ops

__all__ = ["FlowMetrics", "occlusion_masks", "flow_metrics", "cvo_metrics"]


class FlowMetrics:
    """Per-sample metrics, each a (B,) float64 tensor on the device of the sums they were made from:
    epe (mean end-point error), epe_occ / epe_vis (over the mask / its complement, weighted as cal_epe does; NaN where that
    set is empty, the reference's 0/0), px1 / px3 / px5 (share of pixels with epe below 1 / 3 / 5), l1 (mean |pred - gt|
    over both channels); sums: the (B, 8) tensor they were divided from."""
    __slots__ = ("epe", "epe_occ", "epe_vis", "px1", "px3", "px5", "l1", "sums")

    @classmethod
    def from_sums(cls, sums):
        """sums: the (B, 8) tensor of ops.flow_metrics (any device)."""
        if not (isinstance(sums, torch.Tensor) and sums.dim() == 2 and sums.shape[1] == 8):
            raise RuntimeError("FlowMetrics.from_sums: expected a (B,8) tensor, got %s" % (
                tuple(sums.shape) if isinstance(sums, torch.Tensor) else type(sums),))
        s = sums.double()
        m = cls()
        m.sums = s
        n = s[:, 7]
        m.epe = s[:, 0] / n
        m.epe_occ = s[:, 1] / s[:, 2]
        m.epe_vis = (s[:, 0] - s[:, 1]) / (n - s[:, 2])
        m.px1, m.px3, m.px5 = s[:, 3] / n, s[:, 4] / n, s[:, 5] / n
        m.l1 = s[:, 6] / (2.0 * n)
        return m


def occlusion_masks(bflow, fflow, alpha=0.01, beta=0.5):
    """(occ_bw, occ_fw), each (B,1,H,W) with 1 = occluded, of the flow pair bflow = FN0, fflow = F0N (calc_occ_mask)."""
    return ops.fb_occlusion(bflow, fflow, alpha=alpha, beta=beta)


def flow_metrics(pred, gt, occ=None):
    """Metrics of pred against gt, both (B,2,H,W); occ: a (B,1,H,W) mask for the occluded / visible split (without it
    epe_occ is NaN and epe_vis equals epe)."""
    return FlowMetrics.from_sums(ops.flow_metrics(pred, gt, mask=occ))


def cvo_metrics(pred, bflow, fflow):
    """CVO's numbers in one pass: pred against the backward flow bflow, split by the backward occlusion mask of
    (bflow, fflow), which is decided inside the reduction and never stored."""
    return FlowMetrics.from_sums(ops.flow_metrics(pred, bflow, fflow=fflow))
