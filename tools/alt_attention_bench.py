#!/usr/bin/env python3
"""alternate_attention against the stored attention matrix.

1. the per-iteration aggregate of both routes at 90x160 (P = 14 400) with n = 1 and n = 2 items per run, and the
   once-per-image1 part (the matrix / the packs and statistics);
2. the alternate route alone at 180x320 (P = 57 600), where the stored route's 32-bit addressing ends;
3. AccFlow(GMA) on one 7x720x1280 sequence (C5) with the switch off and on, runs alternating in one process.
Medians of per-call event timings.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from accflow_amd import ops  # noqa: E402

D = 128


def timings(fns, reps):
    """{name: median ms} of the callables, interleaved round by round."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ms[k].append(s.elapsed_time(e))
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def op_level(h, w, stored, reps, g):
    P = h * w
    qk = torch.randn(1, 2 * D, h, w, device="cuda", generator=g) * 1.5
    gm = torch.tensor([0.37], device="cuda")
    handle = ops.gma_attention_alt(qk, D, D ** -0.5)
    fns = {"alt_prepare": lambda: ops.gma_attention_alt(qk, D, D ** -0.5)}
    a16 = ops.gma_attention_s16(qk, D, D ** -0.5) if stored else None
    if stored:
        fns["stored_prepare"] = lambda: ops.gma_attention_s16(qk, D, D ** -0.5)
    keep = []
    for n in (1, 2):
        v = torch.randn(n, D, h, w, device="cuda", generator=g)
        fm = torch.randn(n, D, h, w, device="cuda", generator=g)
        out = torch.empty_like(fm)
        keep.append((v, fm, out))
        fns["alt_aggregate_n%d" % n] = (lambda v=v, fm=fm, out=out, n=n: ops.gma_aggregate_alt(
            handle, 0, v, fm.data_ptr(), fm.stride(0), gm, out.data_ptr(), out.stride(0), None, 0, n, D, h, w))
        if stored:
            fns["stored_aggregate_n%d" % n] = (lambda v=v, fm=fm, out=out, n=n: ops.gma_aggregate_s16(
                a16.ptr(), v, fm.data_ptr(), fm.stride(0), gm, out.data_ptr(), out.stride(0), None, 0, n, D, h, w))
    r = timings(fns, reps)
    r.update({"size": "%dx%d" % (h, w), "P": P, "handle_MB": round(handle.nbytes / 1e6, 2),
              "matrix_MB": round(4.0 * P * P / 1e6, 1)})
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    ops.set_conv_mode("f16x3")
    op_level(90, 160, True, a.reps, g)
    torch.cuda.empty_cache()
    op_level(180, 320, False, max(3, a.reps // 3), g)
    torch.cuda.empty_cache()
    if a.skip_model:
        return
    from accflow_amd.data.synthetic import make_sequence, make_state_dict, normalize
    from accflow_amd.networks import build_flow_estimator
    from accflow_amd.networks.AccFlow_ import AccFlow
    model = AccFlow(build_flow_estimator("acc|gma"))
    model.load_state_dict(make_state_dict(model), strict=True)
    model = model.cuda().eval()
    frames = [normalize(f).cuda() for f in make_sequence(7, 7, 720, 1280)]

    def run(on):
        model.ofe.args.alternate_attention = on
        return model(images=frames)

    peaks = {}
    for on in (False, True):
        run(on)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        run(on)
        torch.cuda.synchronize()
        peaks[on] = torch.cuda.max_memory_allocated() - base
    r = timings({"c5_sequence_off_ms": lambda: run(False), "c5_sequence_on_ms": lambda: run(True)}, a.reps)
    r.update({"size": "7x720x1280", "model": "AccFlow(GMA)", "peak_allocated_GB_off": round(peaks[False] / 1e9, 2),
              "peak_allocated_GB_on": round(peaks[True] / 1e9, 2)})
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
