#!/usr/bin/env python3
"""GMA's positional attention against the content attention: the time to prepare ONE attention (once per image1) in the
default mode (f16x3, S16 output) at 60x128 and 90x160.

    content               ops.gma_attention_s16 (the register-only GEMM, no logits matrix)
    tables                ops.gma_pos_tables alone
    position_and_content  tables + ops.gma_attention_pos_s16(content=True): split QK GEMM into the one-item workspace + softmax
    position_only         tables + ops.gma_attention_pos_s16(content=False): no GEMM, no score matrix
and, fp32 j-major (bf16x6 / ACCFLOW_S16=0 route), ops.gma_attention_t against ops.gma_attention_pos_t in both modes (tables
included) - gma_attention_t is the split QK GEMM plus a softmax without table reads, so what it takes beyond the
position_only figure bounds the GEMM from below.
Medians of per-call event timings, the callables interleaved round by round; peak_MB: the most device memory a call holds
beyond its inputs (result + workspace).  One JSON line per size."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from accflow_amd import ops  # noqa: E402

D, MAXPOS = 128, 160
SCALE = D ** -0.5


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
    return {k + "_ms": round(statistics.median(v), 4) for k, v in ms.items()}


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 1e6, 1)


def one_size(h, w, reps, g):
    qk = torch.randn(1, 2 * D, h, w, device="cuda", generator=g) * 1.5
    eh = torch.randn(2 * MAXPOS - 1, D, device="cuda", generator=g)
    ew = torch.randn(2 * MAXPOS - 1, D, device="cuda", generator=g)

    def tables():
        return ops.gma_pos_tables(qk, eh, ew, D, SCALE)

    fns = {
        "content": lambda: ops.gma_attention_s16(qk, D, SCALE),
        "tables": tables,
        "position_and_content": lambda: ops.gma_attention_pos_s16(qk, tables(), D, SCALE, True),
        "position_only": lambda: ops.gma_attention_pos_s16(qk, tables(), D, SCALE, False),
        "content_t_fp32": lambda: ops.gma_attention_t(qk, D, SCALE),
        "position_and_content_t_fp32": lambda: ops.gma_attention_pos_t(qk, tables(), D, SCALE, True),
        "position_only_t_fp32": lambda: ops.gma_attention_pos_t(qk, tables(), D, SCALE, False),
    }
    r = {"size": "%dx%d" % (h, w), "P": h * w, "reps": reps}
    r.update(timings(fns, reps))
    for k in ("content", "position_and_content", "position_only", "position_and_content_t_fp32"):
        r[k + "_peak_MB"] = peak_mb(fns[k])
    r["matrix_MB"] = round(4.0 * (h * w) ** 2 / 1e6, 1)
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gma_pos_bench: needs the GPU (no CPU timing stands in for it)")
    g = torch.Generator(device="cuda").manual_seed(0)
    ops.set_conv_mode("f16x3")
    for h, w in ((60, 128), (90, 160)):
        one_size(h, w, a.reps, g)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
