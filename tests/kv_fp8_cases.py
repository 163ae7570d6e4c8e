"""FP8-KV-cache views of the attention cases of tests/attn_cases.py (shared by the CPU and GPU tests).

``fp8_view(case)`` quantises a paged case's K / V cache (``ops.reference.kv_quantize``) and returns the
quantised tensors with a copy of the case whose k / v are the DEQUANTISED values, so that
``attn_cases.check`` compares against the fp64 reference of exactly what the kernels see.
"""
from __future__ import annotations

import dataclasses
import functools

import torch

import attn_cases as ac
from django_assistant_bot_amd.ops import reference as ref


def fp8_view(case):
    """-> (case over the dequantised cache, (k_data, k_exp, v_data, v_exp))."""
    dev = case.device
    kd, ke = ref.kv_quantize(case.k.cpu())  # (the oracle, on the CPU whatever the case's device)
    vd, ve = ref.kv_quantize(case.v.cpu())
    deq_k, deq_v = ref.kv_dequantize(kd, ke), ref.kv_dequantize(vd, ve)
    assert torch.equal(deq_k.bfloat16().float(), deq_k) and torch.equal(deq_v.bfloat16().float(), deq_v)
    view = dataclasses.replace(case, k=deq_k.bfloat16().to(dev), v=deq_v.bfloat16().to(dev), _cache={})
    return view, tuple(t.contiguous().to(dev) for t in (kd, ke, vd, ve))


def row_scaled(case, seed=0):
    """The case with every K row times 2^r, r in {-1, 0, 1}, and every V row times 2^r, r in {-3 .. 3},
    pseudo-random per (slot, kv head) row: neighbouring rows carry different exponent bytes, so a wrong
    or misindexed exponent moves an output row by far more than the tolerance."""
    g = torch.Generator().manual_seed(1234 + seed)
    rk = torch.randint(-1, 2, case.k.shape[:-1], generator=g).float()
    rv = torch.randint(-3, 4, case.v.shape[:-1], generator=g).float()
    k = (case.k.float().cpu() * torch.exp2(rk)[..., None]).bfloat16().to(case.device)
    v = (case.v.float().cpu() * torch.exp2(rv)[..., None]).bfloat16().to(case.device)
    return dataclasses.replace(case, k=k, v=v, _cache={})


@functools.lru_cache(maxsize=None)
def get_fp8(name, device="cpu", needles=True, scaled=False):
    """(dequantised-view case, quantised cache) of a named case, built once per process."""
    case = ac.get_case(name, device, needles)
    if scaled:
        case = row_scaled(case)
    return fp8_view(case)


def run_fp8(view, cache, ops, **kw):
    """The case through the FP8 ops (CPU tensors: the oracle; device tensors: the HIP kernels)."""
    if view.kind == "decode":
        kw.setdefault("part_size", view.part)
        return ops.paged_decode_fp8(view.q, *cache, view.bt, view.ctx, scale=view.scale, **kw)
    assert view.kind == "paged"
    return ops.flash_attention_paged_fp8(view.q, *cache, view.bt, view.cu_q, view.ctx, max(view.qlens),
                                         causal=view.causal, scale=view.scale, **kw)
