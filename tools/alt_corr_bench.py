#!/usr/bin/env python3
"""alternate_corr against the correlation volume (DESIGN.md "alternate_corr").

1. B = 11 pairs of 7 frames at 480x1024 (60x128): the packed displaced volume + 12 S16 lookups against the alt pyramid + 12
   alt S16 lookups (smooth flow), and the per-launch time of each lookup;
2. the alt path alone at 2160x3840 (270x480), where the volume (~1 TB for 11 pairs) cannot be allocated;
3. AccFlow(RAFT) on one 7x2160x3840 sequence with alternate_corr: ms per call and torch.cuda.max_memory_allocated.
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from accflow_amd import ops  # noqa: E402
from accflow_amd.networks.AccFlow_ import AccFlow  # noqa: E402

ITERS = 12


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def setup(h8, w8, g):
    pairs = AccFlow.pair_schedule(7)
    fmaps = torch.randn(7, 256, h8, w8, device="cuda", generator=g)
    idx1, idx2 = [i for i, _ in pairs], [j for _, j in pairs]
    B = len(pairs)
    smooth = torch.nn.functional.interpolate(3.0 * torch.randn(B, 2, 4, 8, device="cuda", generator=g), size=(h8, w8),
                                             mode="bilinear", align_corners=True)
    coords = (ops.coords_grid(B, h8, w8, "cuda") + smooth).contiguous()
    return fmaps, idx1, idx2, coords


def alt_path(fmaps, idx1, idx2, coords, out16):
    pairs = ops.AltPairs(ops.corr_alt_pyramid(fmaps), idx1, idx2)
    for _ in range(ITERS):
        ops.corr_lookup_alt_s16(pairs, coords, out16)
    return pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-4k-model", action="store_true")
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    ops.set_conv_mode("f16x3")
    # 1. 480x1024
    h8, w8 = 60, 128
    fmaps, idx1, idx2, coords = setup(h8, w8, g)
    B = len(idx1)
    out16 = ops.S16.empty(B, ops.LOOKUP_S16_CHANNELS, h8, w8, "cuda")

    def vol_path():
        dp = ops.corr_volume_disp_packed(ops.corr_pack(fmaps), idx1, idx2)
        for _ in range(ITERS):
            ops.corr_lookup_s16(dp, coords, out16)
        return dp

    t_vol = timed(vol_path, a.reps)
    t_alt = timed(lambda: alt_path(fmaps, idx1, idx2, coords, out16), a.reps)
    dp = vol_path()
    pairs = ops.AltPairs(ops.corr_alt_pyramid(fmaps), idx1, idx2)
    t_pyr = timed(lambda: ops.corr_alt_pyramid(fmaps), a.reps)
    t_vl = timed(lambda: ops.corr_lookup_s16(dp, coords, out16), 20)
    t_al = timed(lambda: ops.corr_lookup_alt_s16(pairs, coords, out16), 20)
    out32 = torch.empty((B, 324, h8, w8), device="cuda")
    t_al32 = timed(lambda: ops.corr_lookup_alt(pairs, coords, out32), 20)
    noisy = (coords + 4.0 * torch.randn(coords.shape, device="cuda", generator=g)).contiguous()
    t_aln = timed(lambda: ops.corr_lookup_alt_s16(pairs, noisy, out16), 20)
    print(json.dumps({"size": "480x1024", "B": B, "volume_plus_12_lookups_ms": round(t_vol, 3),
                      "alt_pyramid_plus_12_lookups_ms": round(t_alt, 3), "alt_pyramid_ms": round(t_pyr, 3),
                      "volume_lookup_s16_us": round(1e3 * t_vl, 1), "alt_lookup_s16_us": round(1e3 * t_al, 1),
                      "alt_lookup_f32_us": round(1e3 * t_al32, 1), "alt_lookup_s16_noisy_flow_us": round(1e3 * t_aln, 1)}),
          flush=True)
    del dp, pairs, out16, out32
    torch.cuda.empty_cache()
    # 2. 2160x3840, alt only
    h8, w8 = 270, 480
    fmaps, idx1, idx2, coords = setup(h8, w8, g)
    out16 = ops.S16.empty(B, ops.LOOKUP_S16_CHANNELS, h8, w8, "cuda")
    t4 = timed(lambda: alt_path(fmaps, idx1, idx2, coords, out16), 2)
    pairs = ops.AltPairs(ops.corr_alt_pyramid(fmaps), idx1, idx2)
    t4l = timed(lambda: ops.corr_lookup_alt_s16(pairs, coords, out16), 5)
    vol_gb = B * sum((h8 * w8) * (h8 >> l) * (w8 >> l) * 4 for l in range(4)) / 1e9
    print(json.dumps({"size": "2160x3840", "B": B, "alt_pyramid_plus_12_lookups_ms": round(t4, 3),
                      "alt_lookup_s16_ms": round(t4l, 3), "alt_pyramid_GB": round(pairs.pyr.data.numel() * 4 / 1e9, 3),
                      "volume_would_need_GB": round(vol_gb, 1)}), flush=True)
    del pairs, out16, fmaps
    torch.cuda.empty_cache()
    if a.skip_4k_model:
        return
    # 3. AccFlow(RAFT), one 7x2160x3840 sequence
    from accflow_amd.data.synthetic import make_sequence, make_state_dict, normalize
    from accflow_amd.networks import build_flow_estimator
    model = AccFlow(build_flow_estimator("acc|raft"))
    model.load_state_dict(make_state_dict(model), strict=True)
    model = model.cuda().eval()
    model.ofe.args.alternate_corr = True
    frames = [normalize(f).cuda() for f in make_sequence(7, 7, 2160, 3840)]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    outs = model(images=frames)
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated() - base
    t0 = time.perf_counter()
    outs = model(images=frames)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    print(json.dumps({"size": "7x2160x3840", "model": "AccFlow(RAFT) alternate_corr", "ms": round(ms, 1),
                      "first_call_s": round(first, 2), "peak_allocated_GB": round(peak / 1e9, 2),
                      "finite": all(bool(torch.isfinite(o).all()) for o in outs), "outputs": len(outs)}), flush=True)


if __name__ == "__main__":
    main()
