"""Occlusion masks and flow metrics without a GPU: the C entry points' argument checks, what the ops refuse before they
touch the library, and the divisions of FlowMetrics.from_sums on hand-made rows."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ("accflow_fb_occlusion_f32", "accflow_flow_metrics_f32", "accflow_flow_metrics_ws_bytes")


def test_entry_points_are_declared_exported_and_reject_bad_arguments():
    from accflow_amd import _lib
    header = open(os.path.join(ROOT, "include", "accflow_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|long long)\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
        assert callable(getattr(lib, name))
    assert "accflow_flow_metrics_ws_bytes" in _lib.RETURNS_LONGLONG
    z, nz = ctypes.c_void_p(0), ctypes.c_void_p(256)          # (nz is never dereferenced: the checks come before any launch)
    occ, met, wsb = lib.accflow_fb_occlusion_f32, lib.accflow_flow_metrics_f32, lib.accflow_flow_metrics_ws_bytes
    # occlusion: null flows, both outputs null, non-positive sizes
    assert occ(z, 0, nz, 0, nz, 0, nz, 0, 0.01, 0.5, 1, 8, 8, z) == 1
    assert occ(nz, 0, z, 0, nz, 0, nz, 0, 0.01, 0.5, 1, 8, 8, z) == 1
    assert occ(nz, 0, nz, 0, z, 0, z, 0, 0.01, 0.5, 1, 8, 8, z) == 1
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -3), (-1, 8, 8)):
        assert occ(nz, 0, nz, 0, nz, 0, nz, 0, 0.01, 0.5, B, H, W, z) == 1
    assert occ(nz, 0, nz, 0, nz, 0, nz, 0, 0.01, 0.5, 1, 65536, 65536, z) == 1      # a plane past 2^31 pixels
    # workspace query: 0 bytes for sizes it cannot serve, 32 bytes per (sample, run of pixels) otherwise
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-2, 8, 8), (1, 65536, 65536), (65536, 8, 8)):
        assert wsb(B, H, W) == 0
    one = wsb(1, 1, 1)
    assert one == 32 and wsb(7, 1, 1) == 7 * 32
    assert wsb(3, 264, 520) % (3 * 32) == 0 and wsb(3, 264, 520) > 3 * 32            # several partials per sample
    assert wsb(5, 264, 520) * 3 == wsb(3, 264, 520) * 5                             # the partition does not depend on B
    # sums: null pred / gt / sums / ws, a mode without its operand, an unknown mode, non-positive sizes
    ok = [nz, 0, nz, 0, nz, 0, nz, 0, 0, 0.01, 0.5, nz, nz, 1, 8, 8, z]
    for i in (0, 2, 11, 12):
        a = list(ok)
        a[i] = z
        assert met(*a) == 1, i
    for mode, missing in ((1, 4), (2, 6)):
        a = list(ok)
        a[8], a[missing] = mode, z
        assert met(*a) == 1, mode
    for mode in (-1, 3):
        a = list(ok)
        a[8] = mode
        assert met(*a) == 1, mode
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        a = list(ok)
        a[13:16] = [B, H, W]
        assert met(*a) == 1, (B, H, W)


def test_ops_refuse_cpu_tensors():
    from accflow_amd import ops
    f = torch.zeros(1, 2, 8, 12)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.fb_occlusion(f, f)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.flow_metrics(f, f)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.flow_metrics(f, f, mask=torch.zeros(1, 1, 8, 12))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.flow_metrics(f, f, fflow=f)


def test_shape_and_argument_errors_come_before_the_library(monkeypatch):
    from accflow_amd import _lib, ops

    def untouchable():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", untouchable)
    f = torch.zeros(2, 2, 8, 12)
    m = torch.zeros(2, 1, 8, 12)
    with pytest.raises(RuntimeError, match="not both"):
        ops.flow_metrics(f, f, mask=m, fflow=f)
    for bad in (torch.zeros(2, 3, 8, 12), torch.zeros(2, 8, 12), torch.zeros(0, 2, 8, 12)):
        with pytest.raises(RuntimeError, match=r"\(B,2,H,W\)"):
            ops.flow_metrics(bad, f)
        with pytest.raises(RuntimeError, match=r"\(B,2,H,W\)"):
            ops.fb_occlusion(bad, f)
    for other in (torch.zeros(2, 2, 8, 13), torch.zeros(2, 2, 9, 12), torch.zeros(1, 2, 8, 12)):
        with pytest.raises(RuntimeError, match="expected"):
            ops.flow_metrics(f, other)
        with pytest.raises(RuntimeError, match="expected"):
            ops.flow_metrics(f, f, fflow=other)
        with pytest.raises(RuntimeError, match="expected"):
            ops.fb_occlusion(f, other)
    with pytest.raises(RuntimeError, match=r"\(B,1,H,W\)"):
        ops.flow_metrics(f, f, mask=f)
    with pytest.raises(RuntimeError, match="expected"):
        ops.flow_metrics(f, f, mask=torch.zeros(2, 1, 8, 11))
    with pytest.raises(RuntimeError, match="want"):
        ops.fb_occlusion(f, f, want=())
    with pytest.raises(RuntimeError, match="want"):
        ops.fb_occlusion(f, f, want=("bw", "sideways"))
    with pytest.raises(RuntimeError, match="not in want"):
        ops.fb_occlusion(f, f, want=("bw",), out_fw=m)
    with pytest.raises(RuntimeError, match="expected"):
        ops.fb_occlusion(f, f, out_bw=torch.zeros(2, 1, 8, 13))
    # well-formed arguments get as far as the device check, still without the library
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.flow_metrics(f, f, mask=m)


def test_from_sums_divisions():
    from accflow_amd.metrics import FlowMetrics
    #            s_epe  s_epe*m  s_m   <1    <3    <5    s_l1   n
    rows = [[120.0, 30.0, 10.0, 20.0, 50.0, 90.0, 150.0, 100.0],      # a partial mask
            [120.0, 0.0, 0.0, 0.0, 0.0, 100.0, 150.0, 100.0],         # an empty mask: no occluded pixel
            [120.0, 120.0, 100.0, 100.0, 100.0, 100.0, 0.0, 100.0],   # a full mask: no visible pixel
            [7.5, 1.25, 0.5, 1.0, 2.0, 3.0, 9.0, 3.0]]                # fractional weights
    m = FlowMetrics.from_sums(torch.tensor(rows, dtype=torch.float64))
    for name in ("epe", "epe_occ", "epe_vis", "px1", "px3", "px5", "l1"):
        v = getattr(m, name)
        assert v.dtype == torch.float64 and tuple(v.shape) == (4,) and v.device.type == "cpu", name
    assert m.epe.tolist() == [1.2, 1.2, 1.2, 2.5]
    assert m.epe_occ[0].item() == 3.0 and m.epe_vis[0].item() == 1.0
    assert math.isnan(m.epe_occ[1].item()) and m.epe_vis[1].item() == 1.2           # 0/0 like the reference; vis = all
    assert m.epe_occ[2].item() == 1.2 and math.isnan(m.epe_vis[2].item())
    assert m.epe_occ[3].item() == 2.5 and m.epe_vis[3].item() == 2.5
    assert m.px1.tolist() == [0.2, 0.0, 1.0, 1.0 / 3.0]
    assert m.px3.tolist() == [0.5, 0.0, 1.0, 2.0 / 3.0]
    assert m.px5.tolist() == [0.9, 1.0, 1.0, 1.0]
    assert m.l1.tolist() == [0.75, 0.75, 0.0, 1.5]
    # float32 sums are promoted, other shapes refused
    assert FlowMetrics.from_sums(torch.tensor(rows, dtype=torch.float32)).epe.dtype == torch.float64
    with pytest.raises(RuntimeError):
        FlowMetrics.from_sums(torch.zeros(8))
    with pytest.raises(RuntimeError):
        FlowMetrics.from_sums(torch.zeros(2, 7))
