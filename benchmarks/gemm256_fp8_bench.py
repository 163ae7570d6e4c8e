"""The FP8 arm of gemm256 against the kernels it replaces (profiles/gemm256_fp8.md): needs a GPU.

    python benchmarks/gemm256_fp8_bench.py gemm    # Llama-3-8B qkv / o / gate_up / down: FP8 arm, bf16 gemm256, gemm_mid
    python benchmarks/gemm256_fp8_bench.py index   # 10M x 768, k = 250: bf16 index, FP8 single launch, FP8 grouped scans

The arms of one shape alternate inside one process (round 0 warms up and is dropped, three rounds are printed);
a time is a host clock around ``iters`` calls that end in a device synchronise.  The grouped scans are the FP8
index's search path before the arm, reached by raising ``VectorIndex.FP8_WIDE_MIN_M``.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from django_assistant_bot_amd import ops  # noqa: E402
from django_assistant_bot_amd.engine.vector_index import VectorIndex  # noqa: E402

DEV = "cuda"


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def rounds(arms, iters, scale=1.0, digits=3):
    runs = {a: [] for a in arms}
    for rnd in range(4):
        for a, fn in arms.items():
            ms = timed(fn, 3 if rnd == 0 else iters)
            if rnd:
                runs[a].append(round(ms * scale, digits))
    return runs


def index_part(rows, dim, k, batches):
    def build(dtype):
        idx = VectorIndex(dim, DEV, capacity=rows + 1024, dtype=dtype)
        g = torch.Generator(device=DEV).manual_seed(7)
        ids = np.arange(rows, dtype=np.int64)
        for s in range(0, rows, 1 << 20):
            i = ids[s:s + (1 << 20)]
            idx.add(i, torch.randn((len(i), dim), device=DEV, generator=g), doc_ids=i // 10,
                    groups=np.zeros(len(i), dtype=np.int32))
        return idx

    i8, i16 = build("fp8"), build("bf16")
    g = torch.Generator(device=DEV).manual_seed(11)
    wide_from = VectorIndex.FP8_WIDE_MIN_M
    res = {}

    def search(idx, q, min_m):
        VectorIndex.FP8_WIDE_MIN_M = min_m
        return idx.search(q, k)

    for B in batches:
        q = torch.randn((B, dim), device=DEV, generator=g)
        runs = rounds({"bf16": lambda: search(i16, q, wide_from), "fp8_wide": lambda: search(i8, q, wide_from),
                       "fp8_grouped": lambda: search(i8, q, 1 << 30)}, 20)
        runs["same_scores"] = bool(torch.equal(search(i8, q, wide_from)[0], search(i8, q, 1 << 30)[0]))
        res[B] = runs
    VectorIndex.FP8_WIDE_MIN_M = wide_from
    return {"unit": "ms per search", "rows": rows, "dim": dim, "k": k, "results": res}


def gemm_part(ms_list):
    shapes = {"qkv": (6144, 4096, 1, "none"), "o": (4096, 4096, 1, "res"), "gate_up": (28672, 4096, 8, "swiglu8"),
              "down": (4096, 14336, 1, "res")}
    res = {}
    g = torch.Generator().manual_seed(3)
    for name, (N, K, grp, epi) in shapes.items():
        data, exps = ops.weight_quantize_fp8((torch.randn(N, K, generator=g) * 0.02).bfloat16())
        dq = ops.weight_dequantize_fp8(data, exps)
        w8, e, w16 = ops.shuffle_weights_fp8(data, grp).to(DEV), exps.to(DEV), ops.shuffle_weights(dq, grp).to(DEV)
        for M in ms_list:
            A = torch.randn(M, K, generator=g).bfloat16().to(DEV)
            r = torch.randn(M, N, generator=g).bfloat16().to(DEV) if epi == "res" else None
            code = ops.EPI_SWIGLU8 if epi == "swiglu8" else ops.EPI_NONE
            arms = {"fp8": lambda: ops.gemm256(A, w8, residual=r, epilogue=code, shuffled=True, b_group=grp, w_exps=e),
                    "bf16": lambda: ops.gemm256(A, w16, residual=r, epilogue=code, shuffled=True, b_group=grp)}
            if name != "gate_up" and ops.kernels.gemm_mid_ok(M, N, K, K):
                arms["gemm_mid"] = lambda: ops.kernels.gemm_mid(A, w16, residual=r, epilogue=code, b_group=grp)
            same = bool(torch.equal(arms["fp8"](), arms["bf16"]()))
            runs = rounds(arms, 10 if M >= 8192 else 50, scale=1e3, digits=1)
            runs["bit_equal"] = same
            res[f"{name}_M{M}"] = runs
        del w8, w16
    return {"unit": "us per call", "results": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("what", choices=("gemm", "index"))
    ap.add_argument("--m", type=int, nargs="+", default=[32768, 1024, 512, 384, 256])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=250)
    ap.add_argument("--batch", type=int, nargs="+", default=[97, 128, 256, 512])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm256_fp8_bench needs a GPU")
    out = gemm_part(a.m) if a.what == "gemm" else index_part(a.rows, a.dim, a.k, a.batch)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
