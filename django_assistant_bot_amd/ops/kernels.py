"""Tensor-level wrappers of the gfx950 kernels.

Each function validates shapes / dtypes / devices on the host BEFORE launching (a hand-written
kernel that is fed a wrong shape faults the GPU), then enqueues on the current HIP stream, which
makes every op capturable into a HIP graph.  CPU tensors run ``ops.reference``.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import reference as ref
from ._lib import expect, expect_bf16_contig, native, ptr, same_device, stream

EPI_NONE, EPI_GELU, EPI_SWIGLU, EPI_SCORES = ref.EPI_NONE, ref.EPI_GELU, ref.EPI_SWIGLU, ref.EPI_SCORES
EPI_SWIGLU8 = ref.EPI_SWIGLU8


def _i32(t: torch.Tensor) -> None:
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise TypeError("expected a contiguous int32 tensor")


# ----------------------------------------------------------------------------------------------
# normalisation / embeddings / pooling


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, residual: torch.Tensor | None = None):
    """RMSNorm over the last dim; with ``residual`` the input is ``x + residual`` and the sum is
    also returned (fused residual stream).  Returns (out, residual_out).

    ``x`` may also be split-K slabs [S, rows, cols] (fp32, or bf16: ``slab_dtype``) of the producing
    projection (``stream_gemm(..., splits=S)``): they are summed in fp32 (and rounded to bf16) inside
    the kernel."""
    slabs = x.dim() == 3 and x.dtype in (torch.float32, torch.bfloat16)
    if not x.is_cuda:
        if slabs:
            x = x.float().sum(0).to(torch.bfloat16)
        return ref.rmsnorm(x, w, eps, residual)
    expect_bf16_contig(w, residual)
    same_device(x, w, residual)
    cols = x.shape[-1]
    expect(w.numel() == cols, "rmsnorm weight size mismatch")
    if slabs:
        expect(x.is_contiguous(), "slabs must be contiguous")
        S, rows = x.shape[0], x.shape[1]
        shape = (rows, cols)
    else:
        expect_bf16_contig(x)
        rows = x.numel() // cols
        shape = tuple(x.shape)
    expect(residual is None or tuple(residual.shape) == shape, "residual shape mismatch")
    out = torch.empty(shape, dtype=torch.bfloat16, device=x.device)
    res_out = torch.empty(shape, dtype=torch.bfloat16, device=x.device) if residual is not None else None
    if slabs:
        native().rmsnorm_slabs(ptr(out), ptr(res_out), ptr(x), S, rows * cols, ptr(residual), ptr(w), rows, cols,
                               float(eps), stream(x), int(x.dtype == torch.bfloat16))
    else:
        native().rmsnorm(ptr(out), ptr(res_out), ptr(x), ptr(residual), ptr(w), rows, cols, float(eps), stream(x))
    return out, res_out


def layernorm(x, gamma, beta, eps, residual=None):
    if not x.is_cuda:
        return ref.layernorm(x, gamma, beta, eps, residual)
    expect_bf16_contig(x, gamma, beta, residual)
    same_device(x, gamma, beta, residual)
    cols = x.shape[-1]
    rows = x.numel() // cols
    expect(gamma.numel() == cols and beta.numel() == cols, "layernorm affine size mismatch")
    expect(residual is None or residual.shape == x.shape, "residual shape mismatch")
    out = torch.empty_like(x)
    native().layernorm(ptr(out), ptr(x), ptr(residual), ptr(gamma), ptr(beta), rows, cols, float(eps), stream(x))
    return out


def bert_embed(ids, pos_ids, type_ids, word, pos, typ, gamma, beta, eps):
    if not ids.is_cuda:
        return ref.bert_embed(ids, pos_ids, type_ids, word, pos, typ, gamma, beta, eps)
    _i32(ids)
    _i32(pos_ids)
    if type_ids is not None:
        _i32(type_ids)
    expect_bf16_contig(word, pos, typ, gamma, beta)
    expect(ids.shape == pos_ids.shape, "ids / position ids mismatch")
    H = word.shape[1]
    out = torch.empty((ids.numel(), H), dtype=word.dtype, device=ids.device)
    native().bert_embed(ptr(out), ptr(ids), ptr(pos_ids), ptr(type_ids), ptr(word), ptr(pos), ptr(typ), ptr(gamma),
                        ptr(beta), ids.numel(), H, float(eps), stream(ids))
    return out


def embed_gather(ids, table):
    if not ids.is_cuda:
        return ref.embed_gather(ids, table)
    _i32(ids)
    expect_bf16_contig(table)
    out = torch.empty((ids.numel(), table.shape[1]), dtype=table.dtype, device=ids.device)
    native().embed_gather(ptr(out), ptr(ids), ptr(table), ids.numel(), table.shape[1], stream(ids))
    return out


def mean_pool(hidden, cu_seqlens, normalize=False, want_bf16=False):
    """Mean over each packed sequence (all tokens, as the reference).  Returns fp32 [B, H]
    (and a bf16 copy when ``want_bf16``)."""
    if not hidden.is_cuda:
        out = ref.mean_pool(hidden, cu_seqlens, normalize)
        return (out, out.to(torch.bfloat16)) if want_bf16 else out
    expect_bf16_contig(hidden)
    _i32(cu_seqlens)
    B = cu_seqlens.numel() - 1
    H = hidden.shape[1]
    expect(H <= 4096, "mean_pool supports hidden <= 4096")
    out = torch.empty((B, H), dtype=torch.float32, device=hidden.device)
    ob = torch.empty((B, H), dtype=torch.bfloat16, device=hidden.device) if want_bf16 else None
    native().mean_pool(ptr(out), ptr(ob), ptr(hidden), ptr(cu_seqlens), B, H, int(bool(normalize)), stream(hidden))
    return (out, ob) if want_bf16 else out


# ----------------------------------------------------------------------------------------------
# element-wise


def gelu(x, bias=None, out=None):
    if not x.is_cuda:
        return ref.gelu(x, bias)
    expect_bf16_contig(x, bias)
    cols = x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    native().gelu(ptr(out), ptr(x), ptr(bias), x.numel() // cols, cols, stream(x))
    return out


def silu_mul(x, interleaved=False, group: int | None = None):
    """x [..., 2F] = [gate | up] -> silu(gate) * up  [..., F].  ``group`` (or ``interleaved`` = 16):
    x columns are ``group``-wide [gate | up] groups (the projection of ``interleave_gate_up``
    weights; 0 = stacked halves)."""
    group = (16 if interleaved else 0) if group is None else int(group)
    if not x.is_cuda:
        if group:
            F2 = x.shape[-1]
            v = x.reshape(*x.shape[:-1], F2 // (2 * group), 2, group)
            x = torch.cat([v[..., 0, :].reshape(*x.shape[:-1], F2 // 2), v[..., 1, :].reshape(*x.shape[:-1], F2 // 2)], -1)
        return ref.silu_mul(x)
    expect(group in (0, 16), "the GPU silu_mul takes stacked or 16-column groups (8-row groups: EPI_SWIGLU8)")
    expect_bf16_contig(x)
    F2 = x.shape[-1]
    rows = x.numel() // F2
    out = torch.empty((*x.shape[:-1], F2 // 2), dtype=x.dtype, device=x.device)
    native().silu_mul(ptr(out), ptr(x), rows, F2 // 2, stream(x), int(group == 16))
    return out


def rope_kv_write(qkv, positions, cos_sin, k_cache, v_cache, slots, Hq, Hkv, D, write_q=True):
    """Applies RoPE to the q/k heads of ``qkv`` [T, (Hq+2Hkv)*D]; writes k, v into the paged caches
    [num_blocks, Hkv, block_size, D] at ``slots`` (int64, <0 skipped); returns q [T, Hq, D].
    ``qkv`` may also be split-K slabs [S, T, (Hq+2Hkv)*D] (fp32 or bf16), summed inside the kernel.
    ``write_q=False`` (bf16 ``qkv``): k / v only, returns None (the prefill attention rotates q on
    load: ``flash_attention_paged(..., rope=...)``)."""
    block_size = k_cache.shape[2]
    slabs = qkv.dim() == 3 and qkv.dtype in (torch.float32, torch.bfloat16)
    if not qkv.is_cuda:
        if slabs:
            qkv = qkv.float().sum(0).to(torch.bfloat16)
        return ref.rope_kv_write(qkv, positions, cos_sin, k_cache, v_cache, slots, Hq, Hkv, D, block_size)
    expect_bf16_contig(k_cache, v_cache)
    _i32(positions)
    expect(slots.dtype == torch.int64 and slots.is_contiguous(), "slots must be contiguous int64")
    expect(cos_sin.dtype == torch.float32 and cos_sin.is_contiguous(), "cos_sin must be contiguous fp32")
    T = qkv.shape[-2]
    expect(qkv.shape[-1] == (Hq + 2 * Hkv) * D, "qkv width mismatch")
    expect(positions.numel() == T and slots.numel() == T, "positions / slots length mismatch")
    expect(tuple(k_cache.shape[1:]) == (Hkv, block_size, D) and k_cache.shape == v_cache.shape, "cache shape mismatch")
    expect(cos_sin.shape[1] == D // 2, "cos/sin table width mismatch")
    if not write_q:
        expect(not slabs, "write_q=False needs a bf16 qkv")
        expect_bf16_contig(qkv)
        native().rope_kv_write(ptr(qkv), qkv.stride(0), ptr(positions), ptr(cos_sin), 0, ptr(k_cache),
                               ptr(v_cache), ptr(slots), T, Hq, Hkv, D, block_size, stream(qkv))
        return None
    q = torch.empty((T, Hq, D), dtype=torch.bfloat16, device=qkv.device)
    if slabs:
        expect(qkv.is_contiguous(), "slabs must be contiguous")
        native().rope_kv_write(0, qkv.shape[-1], ptr(positions), ptr(cos_sin), ptr(q), ptr(k_cache), ptr(v_cache),
                               ptr(slots), T, Hq, Hkv, D, block_size, stream(qkv), ptr(qkv), qkv.shape[0],
                               T * qkv.shape[-1], int(qkv.dtype == torch.bfloat16))
    else:
        expect_bf16_contig(qkv)
        native().rope_kv_write(ptr(qkv), qkv.stride(0), ptr(positions), ptr(cos_sin), ptr(q), ptr(k_cache),
                               ptr(v_cache), ptr(slots), T, Hq, Hkv, D, block_size, stream(qkv))
    return q


# ----------------------------------------------------------------------------------------------
# attention


def _head_strides(t: torch.Tensor):
    # t viewed as [tokens, heads, D] with unit stride on D
    expect(t.stride(-1) == 1, "attention operands need unit stride on the head dim")
    return t.stride(0), t.stride(1)


def flash_attention_packed(q, k, v, cu_q, cu_k, max_seqlen_q, causal=False, scale=None, out=None):
    """Variable-length attention over packed sequences.  q [Tq, Hq, D], k/v [Tk, Hkv, D] may be
    strided views of a fused QKV buffer.  Returns [Tq, Hq, D] contiguous."""
    D = q.shape[-1]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if not q.is_cuda:
        return ref.flash_attention_packed(q, k, v, cu_q, cu_k, causal, scale)
    _i32(cu_q)
    _i32(cu_k)
    expect(q.dtype == torch.bfloat16 and k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16, "bf16 required")
    expect(D in (32, 64, 128), "head dim must be 32, 64 or 128")
    Hq, Hkv = q.shape[1], k.shape[1]
    expect(Hq % Hkv == 0, "GQA requires Hq % Hkv == 0")
    expect(k.stride() == v.stride(), "k and v must share strides")
    qst, qsh = _head_strides(q)
    kst, ksh = _head_strides(k)
    for s in (qst, qsh, kst, ksh):
        expect(s % 8 == 0, "attention strides must be multiples of 8 elements (16 B)")
    out = torch.empty((q.shape[0], Hq, D), dtype=q.dtype, device=q.device) if out is None else out
    B = cu_q.numel() - 1
    native().flash_attention(ptr(q), qst, qsh, ptr(k), ptr(v), kst, ksh, 0, 0, 0, 0, 0, ptr(out), out.stride(0),
                             out.stride(1), ptr(cu_q), ptr(cu_k), 0, B, int(max_seqlen_q), Hq, Hkv, D,
                             int(bool(causal)), 0, float(scale), stream(q))
    return out


def flash_rope_ok(D: int, block_size: int) -> bool:
    """Whether flash_attention_paged can rotate q itself (the 32x32 D = 128 kernel's Q prologue)."""
    return D == 128 and block_size % 64 == 0


def flash_attention_paged(q, k_cache, v_cache, block_tables, cu_q, ctx_lens, max_seqlen_q, causal=True, scale=None,
                          out=None, rope=None):
    """Prefill attention: q [Tq, Hq, D] packed by cu_q, keys/values of each sequence are its first
    ctx_lens[b] tokens in the paged caches (the query chunk is the tail of that context).
    ``rope=(positions int32 [Tq], cos_sin [max_pos, D/2, 2] fp32)``: q is the un-rotated projection
    and RoPE is applied on load (``flash_rope_ok``)."""
    D = q.shape[-1]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if not q.is_cuda:
        if rope is not None:
            pos, cs = rope
            T, Hq = q.shape[0], q.shape[1]
            q = ref.rope_q(q.reshape(T, Hq, D), pos, cs)
        return ref.flash_attention_paged(q, k_cache, v_cache, block_tables, cu_q, ctx_lens, causal, scale)
    _i32(cu_q)
    _i32(ctx_lens)
    _i32(block_tables)
    expect_bf16_contig(k_cache, v_cache)
    expect(D in (32, 64, 128), "head dim must be 32, 64 or 128")
    Hq, Hkv, bs = q.shape[1], k_cache.shape[1], k_cache.shape[2]
    qst, qsh = _head_strides(q)
    out = torch.empty((q.shape[0], Hq, D), dtype=q.dtype, device=q.device) if out is None else out
    B = cu_q.numel() - 1
    expect(block_tables.shape[0] >= B and ctx_lens.numel() >= B, "block table / ctx_lens rows < batch")
    if rope is not None:
        pos, cs = rope
        _i32(pos)
        expect(flash_rope_ok(D, bs) and cs.dtype == torch.float32 and cs.is_contiguous() and pos.numel() == q.shape[0],
               "q RoPE in the attention needs D 128, block size % 64, fp32 cos/sin and one position per query")
        native().flash_attention_rope(ptr(q), qst, qsh, ptr(k_cache), ptr(v_cache), ptr(block_tables),
                                      block_tables.shape[1], bs, ptr(out), out.stride(0), out.stride(1), ptr(cu_q),
                                      ptr(ctx_lens), B, int(max_seqlen_q), Hq, Hkv, D, int(bool(causal)),
                                      float(scale), ptr(pos), ptr(cs), stream(q))
        return out
    native().flash_attention(ptr(q), qst, qsh, 0, 0, 0, 0, ptr(k_cache), ptr(v_cache), ptr(block_tables),
                             block_tables.shape[1], bs, ptr(out), out.stride(0), out.stride(1), ptr(cu_q), 0,
                             ptr(ctx_lens), B, int(max_seqlen_q), Hq, Hkv, D, int(bool(causal)), 1, float(scale),
                             stream(q))
    return out


class DecodeWorkspace:
    """Partition buffers of the split-K paged decode; allocated once (graph-capture safe)."""

    def __init__(self, max_batch, Hq, D, max_parts, device):
        self.max_parts = max_parts
        self.o = torch.empty((max_batch * Hq * max_parts * D,), dtype=torch.float32, device=device)
        self.m = torch.empty((max_batch * Hq * max_parts,), dtype=torch.float32, device=device)
        self.l = torch.empty((max_batch * Hq * max_parts,), dtype=torch.float32, device=device)
        # partition arrival counters of the in-launch combine (one per (sequence, kv head) <= Hq);
        # zero at rest: the last arriving workgroup resets its counter
        self.cnt = torch.zeros((max_batch * Hq,), dtype=torch.int32, device=device)


def paged_decode(q, k_cache, v_cache, block_tables, ctx_lens, part_size=512, workspace: DecodeWorkspace | None = None,
                 scale=None, out=None, order=None, warm=None):
    """q [B, Hq, D] (one new token per sequence) over the paged caches.  ``order`` (int32 [B], a
    permutation of the batch) is the order the (sequence, kv head) items are dispatched in: longest
    context first balances the two rounds of workgroups every CU runs at RAG batch sizes.  Any
    permutation is correct: the kernel bounds its partition walk by its own max over ctx_lens.

    ``warm`` = ``([(tensor, nbytes), ...up to 2], blocks)``: ``blocks`` workgroups appended to the
    launch read the first ``nbytes`` of each tensor into the Infinity Cache (the next projections'
    weights, while the latency-bound attention leaves the CUs idle); the output is unchanged."""
    B, Hq, D = q.shape
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if not q.is_cuda:
        return ref.paged_decode(q, k_cache, v_cache, block_tables, ctx_lens, scale)
    _i32(ctx_lens)
    _i32(block_tables)
    expect_bf16_contig(q, k_cache, v_cache)
    Hkv, bs = k_cache.shape[1], k_cache.shape[2]
    expect(D in (64, 128), "decode head dim must be 64 or 128")
    expect(Hq % Hkv == 0 and Hq // Hkv <= 16, "GQA group must be <= 16")
    expect(part_size % 128 == 0, "part_size must be a multiple of 128")
    expect(block_tables.shape[0] >= B and ctx_lens.numel() >= B, "block table / ctx_lens rows < batch")
    max_parts = workspace.max_parts if workspace is not None else 1
    if workspace is None:
        # single partition covering the longest allowed context
        part_size = max(part_size, ((block_tables.shape[1] * bs + 127) // 128) * 128)
        ws_o = ws_m = ws_l = ws_c = None
    else:
        expect(workspace.o.numel() >= B * Hq * max_parts * D and workspace.cnt.numel() >= B * Hkv,
               "decode workspace too small")
        ws_o, ws_m, ws_l, ws_c = workspace.o, workspace.m, workspace.l, workspace.cnt
    out = torch.empty_like(q) if out is None else out
    if order is not None:
        _i32(order)
        expect(order.is_cuda and order.numel() >= B, "decode order must hold the batch")
    wargs = {}
    if warm is not None and warm[1] > 0:
        ranges, blocks = warm
        expect(1 <= len(ranges) <= 2 and 0 < blocks <= 1024, "warm: 1-2 ranges, 1-1024 workgroups")
        for i, (t, nb) in enumerate(ranges):
            expect(t.is_cuda and t.is_contiguous() and 0 < nb <= t.numel() * t.element_size() and nb % 16 == 0,
                   "warm range must be a 16-B multiple inside a contiguous device tensor")
            wargs[f"w{i}"], wargs[f"w{i}_bytes"] = ptr(t), int(nb)
        wargs["w_blocks"] = int(blocks)
    native().paged_decode_attention(ptr(q), ptr(k_cache), ptr(v_cache), ptr(block_tables), block_tables.shape[1], bs,
                                    ptr(ctx_lens), ptr(out), ptr(ws_o), ptr(ws_m), ptr(ws_l), ptr(ws_c), B, Hq, Hkv,
                                    D, int(part_size), int(max_parts), float(scale), stream(q), ptr(order), **wargs)
    return out


# ----------------------------------------------------------------------------------------------
# FP8 KV cache (opt-in; kv_fp8.hip).  Data uint8 [num_blocks, Hkv, block_size, 128] (OCP e4m3fn),
# exponents uint8 [num_blocks, Hkv, block_size] (E8M0: value = byte * 2^(b - 127)), K and V alike.

kv_quantize = ref.kv_quantize
kv_dequantize = ref.kv_dequantize


def _expect_fp8_cache(k_data, k_exp, v_data, v_exp):
    for t in (k_data, k_exp, v_data, v_exp):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise TypeError("the FP8 KV cache is contiguous uint8 (data and exponent bytes)")
    same_device(k_data, k_exp, v_data, v_exp)
    expect(k_data.dim() == 4 and k_data.shape == v_data.shape and tuple(k_exp.shape) == tuple(k_data.shape[:3])
           and k_exp.shape == v_exp.shape, "FP8 cache: data [blocks, Hkv, block_size, D], exponents [blocks, Hkv, block_size]")
    expect(k_data.shape[3] == 128, "the FP8 KV cache kernels take head dim 128 only")


def rope_kv_write_fp8(qkv, positions, cos_sin, k_data, k_exp, v_data, v_exp, slots, Hq, Hkv, D, write_q=True):
    """``rope_kv_write`` into an FP8 cache: each k / v head row is quantised from the value the bf16
    cache would hold (k: rotated, rounded to bf16); q is returned exactly as ``rope_kv_write`` does."""
    block_size = k_data.shape[2]
    slabs = qkv.dim() == 3 and qkv.dtype in (torch.float32, torch.bfloat16)
    if not qkv.is_cuda:
        if slabs:
            qkv = qkv.float().sum(0).to(torch.bfloat16)
        q = ref.rope_kv_write_fp8(qkv, positions, cos_sin, k_data, k_exp, v_data, v_exp, slots, Hq, Hkv, D, block_size)
        return q if write_q else None
    expect(D == 128, "the FP8 KV cache kernels take head dim 128 only")
    _expect_fp8_cache(k_data, k_exp, v_data, v_exp)
    _i32(positions)
    expect(slots.dtype == torch.int64 and slots.is_contiguous(), "slots must be contiguous int64")
    expect(cos_sin.dtype == torch.float32 and cos_sin.is_contiguous(), "cos_sin must be contiguous fp32")
    T = qkv.shape[-2]
    expect(qkv.shape[-1] == (Hq + 2 * Hkv) * D, "qkv width mismatch")
    expect(positions.numel() == T and slots.numel() == T, "positions / slots length mismatch")
    expect(k_data.shape[1] == Hkv, "cache shape mismatch")
    expect(cos_sin.shape[1] == D // 2, "cos/sin table width mismatch")
    caches = (ptr(k_data), ptr(k_exp), ptr(v_data), ptr(v_exp))
    if not write_q:
        expect(not slabs, "write_q=False needs a bf16 qkv")
        expect_bf16_contig(qkv)
        native().rope_kv_write_fp8(ptr(qkv), qkv.stride(0), ptr(positions), ptr(cos_sin), 0, *caches, ptr(slots), T,
                                   Hq, Hkv, D, block_size, stream(qkv))
        return None
    q = torch.empty((T, Hq, D), dtype=torch.bfloat16, device=qkv.device)
    if slabs:
        expect(qkv.is_contiguous(), "slabs must be contiguous")
        native().rope_kv_write_fp8(0, qkv.shape[-1], ptr(positions), ptr(cos_sin), ptr(q), *caches, ptr(slots), T, Hq,
                                   Hkv, D, block_size, stream(qkv), ptr(qkv), qkv.shape[0], T * qkv.shape[-1],
                                   int(qkv.dtype == torch.bfloat16))
    else:
        expect_bf16_contig(qkv)
        native().rope_kv_write_fp8(ptr(qkv), qkv.stride(0), ptr(positions), ptr(cos_sin), ptr(q), *caches, ptr(slots),
                                   T, Hq, Hkv, D, block_size, stream(qkv))
    return q


def paged_decode_fp8(q, k_data, k_exp, v_data, v_exp, block_tables, ctx_lens, part_size=512,
                     workspace: DecodeWorkspace | None = None, scale=None, out=None, order=None, warm=None):
    """``paged_decode`` over an FP8 cache (D = 128): the same dispatch, partitions, ``order``,
    workspace and in-launch combine; FP8 -> bf16 in registers, bf16 MFMA.  ``warm`` is not supported."""
    B, Hq, D = q.shape
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    expect(warm is None, "paged_decode_fp8 does not take warm= (the L3 warm-up rides on the bf16 kernel only)")
    if not q.is_cuda:
        return ref.paged_decode_fp8(q, k_data, k_exp, v_data, v_exp, block_tables, ctx_lens, scale)
    expect(D == 128, "the FP8 KV cache kernels take head dim 128 only")
    _i32(ctx_lens)
    _i32(block_tables)
    expect_bf16_contig(q)
    _expect_fp8_cache(k_data, k_exp, v_data, v_exp)
    Hkv, bs = k_data.shape[1], k_data.shape[2]
    expect(bs % 32 == 0, "block size must be a multiple of 32")
    expect(Hq % Hkv == 0 and Hq // Hkv <= 16, "GQA group must be <= 16")
    expect(part_size % 128 == 0, "part_size must be a multiple of 128")
    expect(block_tables.shape[0] >= B and ctx_lens.numel() >= B, "block table / ctx_lens rows < batch")
    max_parts = workspace.max_parts if workspace is not None else 1
    if workspace is None:
        part_size = max(part_size, ((block_tables.shape[1] * bs + 127) // 128) * 128)
        ws_o = ws_m = ws_l = ws_c = None
    else:
        expect(workspace.o.numel() >= B * Hq * max_parts * D and workspace.cnt.numel() >= B * Hkv,
               "decode workspace too small")
        ws_o, ws_m, ws_l, ws_c = workspace.o, workspace.m, workspace.l, workspace.cnt
    out = torch.empty_like(q) if out is None else out
    expect(out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == q.shape, "out: contiguous bf16 like q")
    if order is not None:
        _i32(order)
        expect(order.is_cuda and order.numel() >= B, "decode order must hold the batch")
    native().paged_decode_attention_fp8(ptr(q), ptr(k_data), ptr(k_exp), ptr(v_data), ptr(v_exp), ptr(block_tables),
                                        block_tables.shape[1], bs, ptr(ctx_lens), ptr(out), ptr(ws_o), ptr(ws_m),
                                        ptr(ws_l), ptr(ws_c), B, Hq, Hkv, D, int(part_size), int(max_parts),
                                        float(scale), stream(q), ptr(order))
    return out


def kv_dequant_blocks(k_data, k_exp, v_data, v_exp, block_ids, k_out, v_out):
    """k_out[i], v_out[i] ([cap, Hkv, block_size, D] bf16, cap >= n) = the bf16 image of block
    ``block_ids[i]`` (int32 [n]) of an FP8 cache; rows past n are not touched."""
    n = block_ids.numel()
    expect(k_out.shape == v_out.shape and k_out.shape[0] >= n and tuple(k_out.shape[1:]) == tuple(k_data.shape[1:]),
           "scratch: [cap >= n, Hkv, block_size, D]")
    if not k_data.is_cuda:
        ref.kv_dequant_blocks(k_data, k_exp, block_ids, k_out)
        ref.kv_dequant_blocks(v_data, v_exp, block_ids, v_out)
        return k_out, v_out
    _expect_fp8_cache(k_data, k_exp, v_data, v_exp)
    _i32(block_ids)
    expect_bf16_contig(k_out, v_out)
    same_device(k_data, block_ids, k_out, v_out)
    native().kv_fp8_dequant_blocks(ptr(k_data), ptr(k_exp), ptr(v_data), ptr(v_exp), ptr(block_ids), n, ptr(k_out),
                                   ptr(v_out), k_data.shape[1], k_data.shape[2], k_data.shape[3], stream(k_data))
    return k_out, v_out


class KVPrefillPlan:
    """Host-built plan of one prefill step over an FP8 cache: the step's context blocks are
    dequantised into a bf16 scratch pool and the prefill attention runs on the scratch with a
    remapped block table.  ``blocks`` int32 [n]: the cache blocks, group after group; ``scratch_bt``
    int32 [B, cols]: per sequence a running index into its group's scratch (padding columns repeat
    a valid index); ``groups``: runs of whole sequences whose blocks fit the scratch --
    (seq_lo, seq_hi, blk_lo, blk_hi, tok_lo, tok_hi, max_q, cu_q of the group or None for the only one)."""

    __slots__ = ("blocks", "scratch_bt", "groups")

    def __init__(self, blocks, scratch_bt, groups):
        self.blocks, self.scratch_bt, self.groups = blocks, scratch_bt, groups


def kv_prefill_plan(block_tables, ctx_lens, cu_q, block_size: int, cap: int, device=None) -> KVPrefillPlan:
    """``block_tables`` [B, cols], ``ctx_lens`` [B], ``cu_q`` [B + 1]: host (or device: synchronises)
    integer tensors / arrays of the step."""
    bt = torch.as_tensor(block_tables).cpu()
    ctx = [int(x) for x in torch.as_tensor(ctx_lens).cpu().tolist()]
    cu = [int(x) for x in torch.as_tensor(cu_q).cpu().tolist()]
    B = len(cu) - 1
    nblk = [-(-ctx[b] // block_size) for b in range(B)]
    cols = max(1, bt.shape[1])
    sbt = torch.zeros((B, cols), dtype=torch.int32)
    blocks, groups = [], []
    lo = 0
    while lo < B:
        expect(nblk[lo] <= cap, f"a sequence of {nblk[lo]} KV blocks exceeds the FP8 prefill scratch ({cap} blocks)")
        hi, used = lo, 0
        while hi < B and used + nblk[hi] <= cap:
            used += nblk[hi]
            hi += 1
        blk_lo, run = len(blocks), 0
        for b in range(lo, hi):
            blocks.extend(bt[b, :nblk[b]].tolist())
            sbt[b, :nblk[b]] = torch.arange(run, run + nblk[b], dtype=torch.int32)
            sbt[b, nblk[b]:] = run if nblk[b] else 0  # padding columns: any index the group wrote
            run += nblk[b]
        groups.append([lo, hi, blk_lo, len(blocks), cu[lo], cu[hi], max(cu[b + 1] - cu[b] for b in range(lo, hi))])
        lo = hi
    dev = torch.device(device) if device is not None else torch.device("cpu")

    def to(t):
        if dev.type != "cuda":
            return t
        return t.pin_memory().to(dev, non_blocking=True)

    single = len(groups) == 1
    out_groups = []
    for g in groups:
        cu_g = None if single else to(torch.tensor([c - g[4] for c in cu[g[0]:g[1] + 1]], dtype=torch.int32))
        out_groups.append((*g, cu_g))
    return KVPrefillPlan(to(torch.tensor(blocks, dtype=torch.int32)), to(sbt), out_groups)


def flash_attention_paged_fp8(q, k_data, k_exp, v_data, v_exp, block_tables, cu_q, ctx_lens, max_seqlen_q, causal=True,
                              scale=None, out=None, rope=None, scratch=None, plan: KVPrefillPlan | None = None):
    """``flash_attention_paged`` over an FP8 cache.  On the GPU the blocks of ``plan`` (built from
    the step's host arrays: ``kv_prefill_plan``; built here, with a device synchronisation, when it
    is missing) are dequantised into ``scratch`` = (k, v) bf16 [cap, Hkv, block_size, D] and the
    unchanged bf16 prefill kernels run on it, group after group."""
    if not q.is_cuda:
        D = q.shape[-1]
        scale = 1.0 / math.sqrt(D) if scale is None else scale
        if rope is not None:
            q = ref.rope_q(q.reshape(q.shape[0], q.shape[1], D), rope[0], rope[1])
        res = ref.flash_attention_paged_fp8(q, k_data, k_exp, v_data, v_exp, block_tables, cu_q, ctx_lens, causal, scale)
        return res if out is None else out.copy_(res)
    expect(scratch is not None, "the FP8 prefill attention needs the cache's bf16 scratch pool")
    sk, sv = scratch
    if plan is None:
        plan = kv_prefill_plan(block_tables, ctx_lens, cu_q, k_data.shape[2], sk.shape[0], q.device)
    Hq, D = q.shape[1], q.shape[2]
    out = torch.empty((q.shape[0], Hq, D), dtype=q.dtype, device=q.device) if out is None else out
    for lo, hi, b0, b1, t0, t1, max_q, cu_g in plan.groups:
        kv_dequant_blocks(k_data, k_exp, v_data, v_exp, plan.blocks[b0:b1], sk, sv)
        if cu_g is None:  # the whole step: the very launch the bf16 cache would get
            flash_attention_paged(q, sk, sv, plan.scratch_bt, cu_q, ctx_lens, max_seqlen_q, causal, scale, out, rope)
            continue
        if t1 == t0:
            continue
        r = None if rope is None else (rope[0][t0:t1], rope[1])
        flash_attention_paged(q[t0:t1], sk, sv, plan.scratch_bt[lo:hi], cu_g, ctx_lens[lo:hi], max_q, causal, scale,
                              out[t0:t1], r)
    return out


# ----------------------------------------------------------------------------------------------
# GEMM


GEMM256_MIN_M = 1024  # the phased 256x256 kernel from here on; the 128x128 kernel below


# gemm_mid from the first row: at M <= 191 the 128 x 128 kernel re-reads the weights per row tile
# and leaves most CUs idle -- Llama-3-8B qkv / o / gate_up / down at M = 129-187: 54 / 54 / 72 / 181
# us against 31 / 29 / 67 / 47 (profiles/small_prefill_r6.md; decode-sized prefill steps of the
# fragment-layout decoder stream instead, models/llama.py PREFILL_STREAM_MAX_M)
GEMM_MID_MIN_M = 1
GEMM_MID_FILL = 192  # gemm256 keeps a shape whose 256 x 256 tiles fill this many of the 256 CUs


def _g256_fill(M: int, N: int) -> tuple[int, float]:
    """(256 x 256 tiles, share of the last-wave-padded CU slots they fill) of gemm256 on 256 CUs."""
    tiles = -(-M // 256) * (N // 256)
    return tiles, tiles / (-(-tiles // 256) * 256)


def use_gemm_mid(M: int, N: int, K: int, lda: int) -> bool:
    """Mid-M shapes on fragment-layout weights go to the stream-K kernel (gemm_mid.hip) where the
    256 x 256 kernel would leave CUs idle: fewer than GEMM_MID_FILL tiles, or a last wave that
    leaves the chip under 70 % busy.  Measured (profiles/gemm_mid_r6.md): Llama-3-8B qkv / o / down
    at M = 384..2048 run 1.2-2.5x faster than the round-5 dispatch, gate_up at M = 640 / 768 (336
    tiles = 1.31 waves) 12 % faster than gemm256; gate_up at 384 / 512 / 1024 / 2048 and qkv at
    2048 stay on gemm256."""
    if M < GEMM_MID_MIN_M or N % 256 or not gemm_mid_ok(M, N, K, lda):
        return False
    tiles, fill = _g256_fill(M, N)
    return tiles < GEMM_MID_FILL or fill < 0.7


def use_gemm256(M: int, N: int, K: int, lda: int, ldb: int) -> bool:
    """Large-M shapes go to the phased 256x256 kernel (gemm256.hip), and so do shapes from M = 256 on
    whose 256 x 256 tiles fill >= GEMM_MID_FILL CUs (gate_up at M = 384-768: 84-161 us against
    105-184 on the 128 x 128 kernel, profiles/gemm_mid_r6.md)."""
    wide = M >= 256 and N % 256 == 0 and -(-M // 256) * (N // 256) >= GEMM_MID_FILL  # e.g. gate_up at M 256-1023
    return (M >= GEMM256_MIN_M or wide) and bool(native().gemm256_ok(M, N, K, lda, ldb))


def gemm_bt(A, B, bias=None, residual=None, epilogue=EPI_NONE, out_f32=False, row_group=None, q_group=None,
            allow=None, out=None, shuffled=False, n=None, b_group: int = 1, rows=None, as_m=None, w_exps=None,
            w_scales=None):
    """C = A . B^T (+bias) (+act) (+residual) on MFMA; A [M, K], B [N, K] (K-contiguous rows).

    ``shuffled``: B is a ``shuffle_weights`` copy (the layout the decode GEMM streams, so a model
    keeps ONE copy of every projection) of ``B.shape[0]`` rows, of which the first ``n`` (default:
    all) are the matrix; ``b_group`` 8: a ``shuffle_weights(w, 8)`` copy.

    Row subsets, bit-identical to the rows of the full call (the last prefill layer's tail, of which
    only a few rows are read): ``rows`` (int32 [n], device, any order, duplicates allowed) gives
    ``gemm_bt(A, B, residual=R)[rows]`` as a compact [n, N] without computing the other rows -- A
    and the residual are gathered inside the kernel; ``as_m`` makes a call on already compact rows
    take the kernel that ``as_m`` rows would.  Both hold only where that kernel is gemm256, whose
    result for an element depends neither on M nor on the row's place in a tile; any other shape
    is refused.

    ``w_exps`` (FP8 weights, W8A16): B is the uint8 ``shuffle_weights_fp8(data, b_group)`` copy of
    the e4m3fn bytes (``shuffled=True`` required) and ``w_exps`` [N] the rows' exponent bytes.  Every
    such call, at any M and with ``rows`` / ``as_m``, runs the FP8 arm of gemm256 (no other kernel
    reads the bytes): plain / residual / SwiGLU8 projections with N % 256 == 0 and K % 128 == 0,
    anything else is refused.  Bit for bit ``gemm256`` on the dequantised weights.

    ``w_scales`` (MXFP4 weights, W4A16; not together with ``w_exps``): B is the uint8
    ``shuffle_weights_mxfp4(codes, b_group)`` copy [N, K/2] (``shuffled=True`` required) and ``w_scales``
    the ``shuffle_scales_mxfp4`` copy [N, K/32].  Plain / residual / SwiGLU8 projections without bias,
    filters, ``rows`` or ``as_m``, and only where the bf16 call would take ``gemm_mid``
    (``use_gemm_mid``) and ``gemm_mid_mxfp4_ok`` holds: the MXFP4 arm of that kernel, bit for bit its
    result on the dequantised weights.  Any other shape is refused (no other kernel reads the codes).
    On the CPU B and ``w_scales`` are row-major."""
    expect(b_group == 1 or (shuffled and b_group == 8), "b_group: 1, or 8 with a shuffled copy")
    if w_scales is not None:
        expect(w_exps is None, "w_exps (FP8 weights) and w_scales (MXFP4 weights) are mutually exclusive")
        expect(shuffled, "MXFP4 weights (w_scales): B must be the shuffle_weights_mxfp4 copy (shuffled=True)")
        expect(bias is None and epilogue in (EPI_NONE, EPI_SWIGLU8) and not out_f32 and row_group is None
               and q_group is None and allow is None and n is None and rows is None and as_m is None,
               "MXFP4 weights (w_scales): plain / residual / SwiGLU8 projections only, no rows / as_m (the gemm_mid "
               "MXFP4 arm)")
        if A.is_cuda:
            expect(A.dim() == 2 and B.dim() == 2, "MXFP4 weights (w_scales): A [M, K], B [N, K/2]")
            (M, K), N = A.shape, B.shape[0]
            expect(use_gemm_mid(M, N, K, A.stride(0)) and gemm_mid_mxfp4_ok(M, N, K, A.stride(0)),
                   "MXFP4 weights (w_scales): the shape does not take gemm_mid's MXFP4 arm, and no other kernel reads "
                   "the codes")
        return gemm_mid(A, B, residual=residual, epilogue=epilogue, out=out, b_group=b_group, w_scales=w_scales)
    if w_exps is not None:
        expect(shuffled, "FP8 weights (w_exps): B must be the shuffle_weights_fp8 copy (shuffled=True)")
        expect(bias is None and epilogue in (EPI_NONE, EPI_SWIGLU8) and not out_f32 and row_group is None
               and q_group is None and allow is None and n is None,
               "FP8 weights (w_exps): plain / residual / SwiGLU8 projections only (the gemm256 FP8 arm)")
        expect(rows is None or as_m is None, "row subsets: rows or as_m, not both")
        if not A.is_cuda:
            Bd = weight_dequantize_fp8(unshuffle_weights_fp8(B, b_group), w_exps).to(A.dtype)
            y = ref.gemm_bt(A, Bd, None, residual, epilogue)
            y = y if rows is None else y.index_select(0, rows.long())
            return y if out is None else out.copy_(y)
        if as_m is not None:
            expect(int(as_m) >= A.shape[0], "as_m: at least the rows of A")
        return _gemm256_fp8(A, B, w_exps, residual, epilogue, b_group, rows, out)
    if rows is not None or as_m is not None:
        expect(out_f32 is False and row_group is None and q_group is None and allow is None and bias is None
               and n is None and epilogue in (EPI_NONE, EPI_SWIGLU8),
               "row subsets: plain / residual / SwiGLU8 projections only")
        expect(rows is None or as_m is None, "row subsets: rows or as_m, not both")
        if not A.is_cuda:
            y = gemm_bt(A, B, residual=residual, epilogue=epilogue, shuffled=shuffled, b_group=b_group)
            y = y if rows is None else y.index_select(0, rows.long())
            return y if out is None else out.copy_(y)
        return _gemm256_rows(A, B, residual, epilogue, shuffled, b_group, rows, as_m, out)
    if shuffled:
        R = B.shape[0]
        N = R if n is None else int(n)
        expect(R % (16 * b_group) == 0 and B.shape[1] % 32 == 0 and B.is_contiguous() and R >= N,
               "shuffled B: contiguous [R, K] copy, R % (16 b_group) == 0, K % 32 == 0, R >= n")
        if not A.is_cuda:
            Bu = unshuffle_weights(B, b_group)[:N]
            return ref.gemm_bt(A, Bu, bias, residual, epilogue, out_f32, row_group, q_group, allow)
    if not A.is_cuda:
        return ref.gemm_bt(A, B, bias, residual, epilogue, out_f32, row_group, q_group, allow)
    expect(A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16, "bf16 operands required")
    expect(A.stride(-1) == 1 and B.stride(-1) == 1, "operands must be K-contiguous")
    M, K = A.shape
    N = (B.shape[0] if n is None else int(n)) if shuffled else B.shape[0]
    expect(B.shape[1] == K, "inner dims mismatch")
    expect(K % 64 == 0 and N % 4 == 0, "gemm_bt needs K % 64 == 0 and N % 4 == 0")
    expect(A.stride(0) % 8 == 0 and B.stride(0) % 8 == 0, "row strides must be multiples of 8")
    if bias is not None:
        expect_bf16_contig(bias)
        expect(bias.numel() == N, "bias size mismatch")
    n_out = N // 2 if epilogue in (EPI_SWIGLU, EPI_SWIGLU8) else N
    if epilogue == EPI_SWIGLU:
        # (no kernel adds a residual after SwiGLU: gemm.hip's epilogue would store without it)
        expect(N % 32 == 0 and not out_f32 and residual is None,
               "swiglu epilogue needs N % 32 == 0, bf16 output, no residual")
    if epilogue == EPI_SWIGLU8:
        expect(N % 32 == 0 and not out_f32 and bias is None and residual is None,
               "swiglu8 epilogue needs N % 32 == 0, bf16 output, no bias / residual")
    if residual is not None:
        expect(residual.dtype == torch.bfloat16 and residual.stride(-1) == 1, "residual must be bf16 row-major")
        expect(tuple(residual.shape) == (M, n_out), "residual shape mismatch")
    allow_words = 0
    if allow is not None:
        expect(allow.dtype == torch.int32 and allow.is_contiguous() and allow.shape[0] == M, "allow mask shape")
        allow_words = allow.shape[1]
        expect(allow_words * 32 >= N, "allow mask too narrow")
    if row_group is not None:
        _i32(row_group)
        expect(row_group.numel() >= N, "row_group shorter than N")
    if q_group is not None:
        _i32(q_group)
        expect(q_group.numel() >= M, "q_group shorter than M")
    dtype = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty((M, n_out), dtype=dtype, device=A.device)
    expect(out.dtype == dtype and out.stride(-1) == 1 and tuple(out.shape) == (M, n_out), "bad output buffer")
    plain = not out_f32 and row_group is None and q_group is None and allow is None
    if (plain and shuffled and N == B.shape[0] and bias is None and epilogue in (EPI_NONE, EPI_SWIGLU8)
            and use_gemm_mid(M, N, K, A.stride(0))):
        return gemm_mid(A, B, residual=residual, epilogue=epilogue, out=out, b_group=b_group)
    if (epilogue in (EPI_NONE, EPI_GELU, EPI_SWIGLU, EPI_SWIGLU8) and plain and (not shuffled or N == B.shape[0])
            and use_gemm256(M, N, K, A.stride(0), B.stride(0))):
        return _gemm256_into(A, B, out, bias, residual, epilogue, shuffled, b_group)
    native().gemm_bt(ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(out), out.stride(0), ptr(bias), ptr(residual),
                     residual.stride(0) if residual is not None else 0, M, N, K, int(epilogue), int(out_f32),
                     ptr(row_group), ptr(q_group), ptr(allow), allow_words, stream(A),
                     B.shape[0] if shuffled else 0, int(b_group))
    return out


def _gemm256_into(A, B, out, bias, residual, epilogue, shuffled, b_group=1, rows=None):
    M, K = A.shape
    native().gemm256(ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(out), out.stride(0), ptr(bias), ptr(residual),
                     residual.stride(0) if residual is not None else 0, M if rows is None else rows.numel(), B.shape[0],
                     K, int(epilogue), stream(A), int(shuffled), int(b_group), ptr(rows), M if rows is not None else 0)
    return out


def _gemm256_rows(A, B, residual, epilogue, shuffled, b_group, rows, as_m, out=None, direct=False):
    """``gemm_bt`` with ``rows`` / ``as_m``: the dispatch follows the full row count and must end
    at gemm256 (``direct``: ``ops.gemm256``, which takes any M)."""
    expect(A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16, "bf16 operands required")
    expect(A.dim() == 2 and B.dim() == 2 and A.stride(-1) == 1 and B.stride(-1) == 1 and B.shape[1] == A.shape[1],
           "operands must be K-contiguous [M, K] / [N, K]")
    (M, K), N = A.shape, B.shape[0]
    full = M if rows is not None else int(as_m)
    n_out = N // 2 if epilogue == EPI_SWIGLU8 else N
    if rows is not None:
        _i32(rows)
        expect(rows.is_cuda and rows.dim() == 1, "rows: int32 [n] on the device")
    else:
        expect(full >= M, "as_m: at least the rows of A")
    expect(epilogue == EPI_NONE or residual is None, "swiglu8 epilogue takes no residual")
    if residual is not None:
        expect(residual.dtype == torch.bfloat16 and residual.stride(-1) == 1 and tuple(residual.shape) == (M, n_out),
               "residual must be bf16 row-major [M, N]")
    lda = A.stride(0)
    mid = shuffled and use_gemm_mid(full, N, K, lda)
    expect(direct or (not mid and use_gemm256(full, N, K, lda, B.stride(0))),
           "row subsets need the shape's full call on gemm256 (not gemm_mid or the 128 x 128 kernel)")
    expect(bool(native().gemm256_ok(M, N, K, lda, B.stride(0))), "gemm256: N % 256, K % 128, 16-B rows")
    expect(not shuffled or (B.is_contiguous() and B.shape[1] == K), "shuffled B must be a contiguous [N, K] copy")
    n = M if rows is None else rows.numel()
    if out is None:
        out = torch.empty((n, n_out), dtype=torch.bfloat16, device=A.device)
    expect(out.dtype == torch.bfloat16 and out.stride(-1) == 1 and tuple(out.shape) == (n, n_out)
           and (n <= 1 or out.stride(0) % 8 == 0), "bad output buffer")
    if n == 0:
        return out
    return _gemm256_into(A, B, out, None, residual, epilogue, shuffled, b_group, rows)


def _gemm256_fp8(A, B, w_exps, residual, epilogue, b_group, rows, out, bias=None, shuffled=True):
    """The FP8-weight arm of gemm256 (``gemm256_kernel<..., W8>``): checks, then the launch.  Every
    refusal is raised here, before any launch."""
    expect(A.is_cuda and A.dtype == torch.bfloat16 and A.dim() == 2 and A.stride(-1) == 1, "bf16 CUDA A [M, K] required")
    expect(shuffled, "gemm256 FP8 arm: the row-major layout has no FP8 form (shuffled=True)")
    expect(bias is None, "gemm256 FP8 arm: no bias")
    expect(epilogue in (EPI_NONE, EPI_SWIGLU8), "gemm256 FP8 arm: epilogues none (+ residual) or SwiGLU8")
    expect(b_group in (1, 8), "gemm256 FP8 arm: b_group 1 or 8")
    expect(B.is_cuda and B.dtype == torch.uint8 and B.dim() == 2 and B.is_contiguous(),
           "FP8 weights: B must be the contiguous uint8 shuffle_weights_fp8 copy [N, K]")
    (M, K), N = A.shape, B.shape[0]
    expect(B.shape[1] == K, "inner dims mismatch")
    expect(M > 0 and bool(native().gemm256_ok(M, N, K, A.stride(0), K)), "gemm256: N % 256, K % 128, 16-B rows")
    expect(w_exps.dtype == torch.uint8 and w_exps.is_cuda and w_exps.dim() == 1 and w_exps.shape[0] == N
           and w_exps.is_contiguous() and w_exps.data_ptr() % 4 == 0,
           "w_exps must be the uint8 [N] row exponents (contiguous, 4-byte aligned)")
    same_device(A, B, w_exps, residual, rows, out)
    n_out = N // 2 if epilogue == EPI_SWIGLU8 else N
    expect(epilogue == EPI_NONE or residual is None, "swiglu8 epilogue takes no residual")
    if residual is not None:
        expect(residual.dtype == torch.bfloat16 and residual.stride(-1) == 1 and tuple(residual.shape) == (M, n_out),
               "residual must be bf16 row-major [M, N]")
    n = M
    if rows is not None:
        _i32(rows)
        expect(rows.is_cuda and rows.dim() == 1, "rows: int32 [n] on the device")
        n = rows.numel()
    if out is None:
        out = torch.empty((n, n_out), dtype=torch.bfloat16, device=A.device)
    expect(out.dtype == torch.bfloat16 and out.stride(-1) == 1 and tuple(out.shape) == (n, n_out)
           and (n <= 1 or out.stride(0) % 8 == 0), "bad output buffer")
    if n == 0:
        return out
    native().gemm256_fp8(ptr(A), A.stride(0), ptr(B), ptr(w_exps), ptr(out), out.stride(0), 0, ptr(residual),
                         residual.stride(0) if residual is not None else 0, n, N, K, int(epilogue), stream(A), 1,
                         int(b_group), ptr(rows), M if rows is not None else 0)
    return out


def gemm256(A, B, bias=None, residual=None, epilogue=EPI_NONE, shuffled=False, b_group: int = 1, rows=None,
            out=None, w_exps=None):
    """The phased 256x256 kernel directly, for any M (``gemm_bt`` takes it from M >= 1024):
    tests and benchmarks.  N % 256 == 0, K % 128 == 0.  ``rows``: the row-subset mode (see
    ``gemm_bt``), into ``out`` [n, N] if given.  ``w_exps``: the FP8-weight arm (see ``gemm_bt``),
    into ``out`` if given."""
    if w_exps is not None:
        return _gemm256_fp8(A, B, w_exps, residual, epilogue, b_group, rows, out, bias=bias, shuffled=shuffled)
    if rows is not None:
        expect(A.is_cuda and bias is None, "gemm256 rows: CUDA operands, no bias")
        return _gemm256_rows(A, B, residual, epilogue, shuffled, b_group, rows, None, out, direct=True)
    M, K = A.shape
    N = B.shape[0]
    expect(A.is_cuda and A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16, "bf16 CUDA operands required")
    expect(bool(native().gemm256_ok(M, N, K, A.stride(0), B.stride(0))), "gemm256: N % 256, K % 128, 16-B rows")
    expect(not shuffled or (B.is_contiguous() and B.shape[1] == K), "shuffled B must be a contiguous [N, K] copy")
    n_out = N // 2 if epilogue in (EPI_SWIGLU, EPI_SWIGLU8) else N
    out = torch.empty((M, n_out), dtype=torch.bfloat16, device=A.device)
    return _gemm256_into(A, B, out, bias, residual, epilogue, shuffled, b_group)


_MID_WS: dict = {}


def _mid_workspace(device: torch.device, s: int):
    """Partial-tile slabs + ready flags of ``gemm_mid``, one set per (device, stream): two streams
    running the kernel at once must not share them.  The flags are zero at rest (every launch leaves
    them zero)."""
    key = (device.index, s)
    ws = _MID_WS.get(key)
    if ws is None:
        nat = native()
        slabs = torch.empty((nat.gemm_mid_slab_bytes() // 4,), dtype=torch.float32, device=device)
        cnt = torch.zeros((1 << 16,), dtype=torch.int32, device=device)
        ws = _MID_WS[key] = (slabs, cnt)
    return ws


def gemm_mid_ok(M: int, N: int, K: int, lda: int) -> bool:
    """Shapes ``gemm_mid`` serves: N % 256, K % 64, ceil(M / 128) <= 32 (M <= 4096)."""
    return bool(native().gemm_mid_ok(M, N, K, lda)) and -(-M // 128) * (N // 256) <= (1 << 16)


def gemm_mid_mxfp4_ok(M: int, N: int, K: int, lda: int) -> bool:
    """Shapes the MXFP4 arm of ``gemm_mid`` serves: ``gemm_mid_ok`` and K % 128 == 0."""
    return gemm_mid_ok(M, N, K, lda) and bool(native().gemm_mid_mxfp4_ok(M, N, K, lda))


def gemm_mid(A, B, residual=None, epilogue=EPI_NONE, out=None, variant: int = 0, b_group: int = 1, w_scales=None,
             convert: int = 0):
    """C = A . B^T (+ residual) or SwiGLU over 8-row [gate | up] groups, B a ``shuffle_weights`` copy:
    the mid-M kernel (``gemm_mid.hip``: grouped stream-K, 128 x 256 tiles, in-launch owner combine) for
    M = 256..4096 (mixed serving steps, single prompts).  Bit-reproducible: the split-K partials are
    summed in a fixed order.  ``variant`` (A/B harness): 32 / 64 force the K-step; + 1000 leaves
    split tiles uncombined (timing only).

    ``w_scales`` (MXFP4 weights, W4A16): ``B`` is the uint8 ``shuffle_weights_mxfp4(codes, b_group)`` copy
    [N, K/2] and ``w_scales`` the ``shuffle_scales_mxfp4`` copy [N, K/32]; the kernel's MXFP4 arm converts
    the codes in registers and gives, bit for bit, what the bf16 kernel gives on
    ``shuffle_weights(weight_dequantize_mxfp4(...), b_group)``.  K % 128 == 0, ``variant`` 0 only;
    ``convert`` (A/B harness): 1 / 2 place the conversion after / before the phase's read barrier.  On
    the CPU both are row-major and the result is ``ref.gemm_bt`` on the dequantised rows."""
    fp4 = w_scales is not None
    expect(epilogue in (EPI_NONE, EPI_SWIGLU8), "gemm_mid epilogues: none (+residual) or SwiGLU8")
    expect(not fp4 or int(variant) == 0, "gemm_mid MXFP4 arm: variant 0 only")
    expect(fp4 or int(convert) == 0, "convert: the MXFP4 arm only")
    if fp4 and not A.is_cuda:
        expect(epilogue == EPI_NONE or residual is None, "swiglu8 epilogue takes no residual")
        y = ref.gemm_bt(A, weight_dequantize_mxfp4(B, w_scales).to(A.dtype), None, residual, epilogue)
        return y if out is None else out.copy_(y)
    expect(A.dim() == 2 and B.dim() == 2, "A [M, K], B [N, K] (MXFP4: [N, K/2])")
    M, K = A.shape
    N = B.shape[0]
    if fp4:
        expect(A.is_cuda and A.dtype == torch.bfloat16 and B.is_cuda and B.dtype == torch.uint8 and B.is_contiguous()
               and B.data_ptr() % 16 == 0,
               "MXFP4 weights: bf16 CUDA A, contiguous 16-byte aligned uint8 fragment copy [N, K/2]")
        expect(A.stride(-1) == 1 and K % 128 == 0 and B.shape[1] * 2 == K,
               "MXFP4 weights: A K-contiguous, K % 128 == 0, B [N, K/2]")
        expect(w_scales.dtype == torch.uint8 and w_scales.is_cuda and w_scales.dim() == 2
               and tuple(w_scales.shape) == (N, K // 32) and w_scales.is_contiguous() and w_scales.data_ptr() % 4 == 0,
               "w_scales must be the uint8 [N, K/32] shuffle_scales_mxfp4 copy (contiguous, 4-byte aligned)")
        same_device(A, B, w_scales, residual, out)
        expect(gemm_mid_mxfp4_ok(M, N, K, A.stride(0)), "gemm_mid MXFP4 arm: N % 256, K % 128, M <= 4096, 16-B rows")
        expect(int(convert) in (0, 1, 2), "convert: 0, 1 or 2")
    else:
        expect(A.is_cuda and A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16, "bf16 CUDA operands required")
        expect(A.stride(-1) == 1 and B.is_contiguous() and B.shape[1] == K,
               "A K-contiguous, B a contiguous [N, K] copy")
    expect(gemm_mid_ok(M, N, K, A.stride(0)), "gemm_mid: N % 256, K % 64, M <= 4096, 16-B rows")
    expect(b_group in (1, 8), "gemm_mid: b_group 1 or 8")
    n_out = N // 2 if epilogue == EPI_SWIGLU8 else N
    if residual is not None:
        expect(epilogue == EPI_NONE and residual.dtype == torch.bfloat16 and residual.stride(-1) == 1
               and tuple(residual.shape) == (M, N), "residual must be bf16 [M, N]")
    if out is None:
        out = torch.empty((M, n_out), dtype=torch.bfloat16, device=A.device)
    expect(out.dtype == torch.bfloat16 and out.stride(-1) == 1 and tuple(out.shape) == (M, n_out), "bad output")
    s = stream(A)
    slabs, cnt = _mid_workspace(A.device, s)
    if fp4:
        native().gemm_mid_mxfp4(ptr(A), A.stride(0), ptr(B), ptr(w_scales), ptr(out), out.stride(0), ptr(residual),
                                residual.stride(0) if residual is not None else 0, M, N, K, int(epilogue), ptr(slabs),
                                slabs.numel() * 4, ptr(cnt), cnt.numel(), s, int(b_group), int(convert))
        return out
    native().gemm_mid(ptr(A), A.stride(0), ptr(B), ptr(out), out.stride(0), ptr(residual),
                      residual.stride(0) if residual is not None else 0, M, N, K, int(epilogue), ptr(slabs),
                      slabs.numel() * 4, ptr(cnt), cnt.numel(), s, int(variant), int(b_group))
    return out


def score_candidates(A, B, thr, cap, row_group=None, q_group=None):
    """Filtered cosine scores of A [M, K] against B [N, K] that are >= thr[m], appended per query
    (no [M, N] score matrix).  -> (cand_val fp32 [M, cap] (-inf padded), cand_idx int32 [M, cap]
    (defined for the first count entries of a row only), count int32 [M]; count > cap means the
    list overflowed)."""
    expect(A.is_cuda and A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16, "bf16 CUDA operands required")
    expect(A.stride(-1) == 1 and B.stride(-1) == 1 and A.stride(0) % 8 == 0 and B.stride(0) % 8 == 0,
           "operands must be K-contiguous with row strides % 8 == 0")
    M, K = A.shape
    N = B.shape[0]
    expect(B.shape[1] == K and K % 64 == 0 and N % 4 == 0, "score_candidates needs K % 64 == 0 and N % 4 == 0")
    expect(thr.dtype == torch.float32 and thr.is_contiguous() and thr.numel() >= M, "thr must be fp32 [M]")
    if row_group is not None:
        _i32(row_group)
        expect(row_group.numel() >= N, "row_group shorter than N")
    if q_group is not None:
        _i32(q_group)
        expect(q_group.numel() >= M, "q_group shorter than M")
    cand_val = torch.full((M, cap), float("-inf"), dtype=torch.float32, device=A.device)
    cand_idx = torch.empty((M, cap), dtype=torch.int32, device=A.device)
    cnt = torch.zeros(M, dtype=torch.int32, device=A.device)
    native().gemm_score_candidates(ptr(A), A.stride(0), ptr(B), B.stride(0), M, N, K, ptr(row_group), ptr(q_group),
                                   ptr(thr), ptr(cnt), ptr(cand_val), ptr(cand_idx), int(cap), stream(A))
    return cand_val, cand_idx, cnt


def score_candidates_shuffled(A, B_shuf, N, thr, cap, row_group=None, q_group=None):
    """``score_candidates`` over a copy of the rows in the ``shuffle_weights`` layout (``B_shuf``
    [R, K], R >= round_up(N, 128), R % 16 == 0): every 16-row x 32-k fragment is one coalesced 1 KB
    load (1..96 queries at K <= 768, 1..64 at K <= 1024: the persistent scan of index_scan.hip;
    more (K % 128 == 0): gemm256's candidate epilogue; the weight-streaming kernel's candidate
    epilogue otherwise)."""
    expect(A.is_cuda and A.dtype == torch.bfloat16 and B_shuf.dtype == torch.bfloat16, "bf16 CUDA operands required")
    M, K = A.shape
    expect(shuffled_scan_ok(M, K) and A.stride(-1) == 1 and A.stride(0) % 8 == 0, "queries need K % 128 == 0")
    expect(B_shuf.is_contiguous() and B_shuf.shape[1] == K, "shuffled copy [R, K]")
    expect(B_shuf.shape[0] % 16 == 0 and B_shuf.shape[0] >= -(-N // 128) * 128, "shuffled copy needs round_up(N, 128) rows")
    expect(thr.dtype == torch.float32 and thr.is_contiguous() and thr.numel() >= M, "thr must be fp32 [M]")
    if row_group is not None:
        _i32(row_group)
        expect(row_group.numel() >= N, "row_group shorter than N")
    if q_group is not None:
        _i32(q_group)
        expect(q_group.numel() >= M, "q_group shorter than M")
    cand_val = torch.full((M, cap), float("-inf"), dtype=torch.float32, device=A.device)
    cand_idx = torch.empty((M, cap), dtype=torch.int32, device=A.device)
    cnt = torch.zeros(M, dtype=torch.int32, device=A.device)
    native().score_candidates_shuf(ptr(A), A.stride(0), ptr(B_shuf), M, int(N), K, ptr(row_group), ptr(q_group),
                                   ptr(thr), ptr(cnt), ptr(cand_val), ptr(cand_idx), int(cap), stream(A),
                                   B_shuf.shape[0])
    return cand_val, cand_idx, cnt


def shuffled_scan_ok(M: int, K: int) -> bool:
    """Query counts / widths ``score_candidates_shuffled`` serves."""
    return M >= 1 and K % 128 == 0


def shuffle_rows_into(dst: torch.Tensor, rows: torch.Tensor, vals: torch.Tensor) -> None:
    """Writes ``vals`` [n, K] as rows ``rows`` of ``dst``, a [R, K] tensor in the ``shuffle_weights``
    layout (the incremental form of shuffle_weights, for copies that are updated in place)."""
    R, K = dst.shape
    v5 = dst.view(R // 16, K // 32, 4, 16, 8)
    rows = rows.to(dst.device, torch.long)
    v5[rows // 16, :, :, rows % 16, :] = vals.to(dst.dtype).reshape(-1, K // 32, 4, 8)


def _ref_stream_gemm(x, w, splits=1, epilogue=EPI_NONE, residual=None, norm_eps=0.0):
    """CPU semantics of ``stream_gemm`` (row-major ``w``): bf16 [M, N] / SwiGLU / fp32 slabs
    [S, M, N] whose sum is the product (slab 0 holds it, the others are zero).  ``norm_eps`` > 0:
    the product of the RMS-normalised rows of x (gains folded into w) before the epilogue."""
    if norm_eps > 0:
        xf = x.float()
        r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + norm_eps)
        y = xf @ w.float().t() * r
        if epilogue in (EPI_SWIGLU, EPI_SWIGLU8):
            grp = 16 if epilogue == EPI_SWIGLU else 8
            v = y.view(y.shape[0], -1, 2, grp)
            y = (torch.nn.functional.silu(v[:, :, 0]) * v[:, :, 1]).reshape(y.shape[0], -1)
        if splits > 1:
            return torch.cat([y[None], torch.zeros((splits - 1,) + tuple(y.shape))], 0)
        return y.to(torch.bfloat16)
    y = ref.gemm_bt(x, w, None, None, epilogue, out_f32=splits > 1)
    if splits > 1:
        return torch.cat([y[None], torch.zeros((splits - 1,) + tuple(y.shape), dtype=y.dtype)], 0)
    return y if residual is None else (y.float() + residual.float()).to(torch.bfloat16)


STREAM_KS = 128
STREAM_MAX_M = 256  # decode batches / prefill last-token LM heads up to this many rows stream the weights


def shuffle_weights(w: torch.Tensor, group: int = 1) -> torch.Tensor:
    """[N, K] row-major -> the same values in the fragment layout [N/16][K/32][64 lanes][8]: the
    16 x 32 tile an MFMA A fragment covers is 1 KB contiguous, in lane order (lane l = row l & 15,
    k 8 (l >> 4) .. + 8), so every weight load of the streaming kernel is one fully coalesced 1 KB
    read, and the prefill GEMMs' LDS-DMA copies whole blocks (gemm256 / gemm_bt ``shuffled``).
    ``group`` G > 1: the grouped form [N/(16G)][K/32][G][1 KB] -- the fragments of G consecutive
    16-row blocks adjacent for each 32-deep k chunk, so the decode GEMM's waves (one block each)
    stream neighbouring bytes (profiles/decode_stream_layout_r6.md); the kernels take it with
    ``w_group`` / ``b_group`` = G.  Returned with shape [N, K] (only the memory order changes)."""
    N, K = w.shape
    expect(N % (16 * group) == 0 and K % 32 == 0, "shuffle_weights needs N % (16 group) == 0 and K % 32 == 0")
    f = w.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4)
    if group > 1:
        f = f.reshape(N // (16 * group), group, K // 32, 512).permute(0, 2, 1, 3)
    return f.contiguous().view(N, K)


def unshuffle_weights(w: torch.Tensor, group: int = 1) -> torch.Tensor:
    """Inverse of ``shuffle_weights``."""
    N, K = w.shape
    if group > 1:
        w = w.reshape(N // (16 * group), K // 32, group, 512).permute(0, 2, 1, 3)
    return w.reshape(N // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).contiguous().view(N, K)


weight_quantize_fp8 = ref.weight_quantize_fp8
weight_dequantize_fp8 = ref.weight_dequantize_fp8


def shuffle_weights_fp8(data: torch.Tensor, group: int = 1) -> torch.Tensor:
    """e4m3fn bytes [N, K] (uint8, row-major) -> the FP8 fragment layout [N/16][K/64][64 lanes][16 B]
    the streaming decode GEMM's FP8 arm reads: lane l holds row l & 15, its bytes 0-7 are
    k = 64j + 8 (l >> 4) .. + 8 and its bytes 8-15 k = 64j + 32 + 8 (l >> 4) .. + 8, so one 16-byte lane
    load (a fully coalesced 1 KB wave read) feeds two 32-deep MFMA chunks.  ``group`` G > 1 as in
    ``shuffle_weights``: the fragments of G consecutive 16-row blocks adjacent per 64-deep k step.
    Returned with shape [N, K]."""
    N, K = data.shape
    expect(data.dtype == torch.uint8, "shuffle_weights_fp8 takes e4m3fn bytes (uint8)")
    expect(N % (16 * group) == 0 and K % 64 == 0, "shuffle_weights_fp8 needs N % (16 group) == 0 and K % 64 == 0")
    f = data.reshape(N // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5)  # [blk, j, l >> 4, l & 15, half, 8]
    if group > 1:
        f = f.reshape(N // (16 * group), group, K // 64, 1024).permute(0, 2, 1, 3)
    return f.contiguous().view(N, K)


def unshuffle_weights_fp8(data: torch.Tensor, group: int = 1) -> torch.Tensor:
    """Inverse of ``shuffle_weights_fp8``."""
    N, K = data.shape
    if group > 1:
        data = data.reshape(N // (16 * group), K // 64, group, 1024).permute(0, 2, 1, 3)
    return data.reshape(N // 16, K // 64, 4, 16, 2, 8).permute(0, 3, 1, 4, 2, 5).contiguous().view(N, K)


def shuffle_rows_into_fp8(dst: torch.Tensor, rows: torch.Tensor, data: torch.Tensor) -> None:
    """Writes e4m3fn bytes ``data`` [n, K] (uint8) as rows ``rows`` of ``dst``, a uint8 [R, K] tensor in
    the ``shuffle_weights_fp8`` layout (group 1): the incremental form of ``shuffle_weights_fp8``, the
    FP8 counterpart of ``shuffle_rows_into``."""
    R, K = dst.shape
    expect(dst.dtype == torch.uint8 and data.dtype == torch.uint8, "shuffle_rows_into_fp8 takes e4m3fn bytes (uint8)")
    expect(R % 16 == 0 and K % 64 == 0 and dst.is_contiguous(), "FP8 fragment copy: contiguous [R, K], R % 16, K % 64")
    v6 = dst.view(R // 16, K // 64, 4, 16, 2, 8)  # [blk, j, l >> 4, l & 15, half, 8]
    rows = rows.to(dst.device, torch.long)
    v6[rows // 16, :, :, rows % 16, :, :] = data.to(dst.device).reshape(-1, K // 64, 2, 4, 8).permute(0, 1, 3, 2, 4)


weight_quantize_mxfp4 = ref.weight_quantize_mxfp4
weight_dequantize_mxfp4 = ref.weight_dequantize_mxfp4


def shuffle_weights_mxfp4(codes: torch.Tensor, group: int = 1) -> torch.Tensor:
    """e2m1 codes [N, K/2] (uint8, two per byte, row-major: ``weight_quantize_mxfp4``) -> the MXFP4
    fragment layout [N/16][K/128][64 lanes][16 B] the streaming decode GEMM's MXFP4 arm reads: lane l
    holds row l & 15, its bytes 4c .. 4c + 3 are the 8 codes of k = 128j + 32c + 8 (l >> 4) .. + 8 -- the
    lane's operand of the c-th 32-deep MFMA chunk, and exactly one MX block of the row per chunk -- so
    one 16-byte lane load (a fully coalesced 1 KB wave read) feeds four chunks.  ``group`` G > 1 as in
    ``shuffle_weights``: the fragments of G consecutive 16-row blocks adjacent per 128-deep k step.
    Returned with shape [N, K/2]."""
    expect(codes.dtype == torch.uint8 and codes.dim() == 2, "shuffle_weights_mxfp4 takes e2m1 code bytes (uint8 [N, K/2])")
    N, K = codes.shape[0], codes.shape[1] * 2
    expect(N % (16 * group) == 0 and K % 128 == 0, "shuffle_weights_mxfp4 needs N % (16 group) == 0 and K % 128 == 0")
    f = codes.reshape(N // 16, 16, K // 128, 4, 4, 4).permute(0, 2, 4, 1, 3, 5)  # [blk, j, l >> 4, l & 15, c, 4 B]
    if group > 1:
        f = f.reshape(N // (16 * group), group, K // 128, 1024).permute(0, 2, 1, 3)
    return f.contiguous().view(N, K // 2)


def unshuffle_weights_mxfp4(codes: torch.Tensor, group: int = 1) -> torch.Tensor:
    """Inverse of ``shuffle_weights_mxfp4``."""
    N, K = codes.shape[0], codes.shape[1] * 2
    if group > 1:
        codes = codes.reshape(N // (16 * group), K // 128, group, 1024).permute(0, 2, 1, 3)
    return codes.reshape(N // 16, K // 128, 4, 16, 4, 4).permute(0, 3, 1, 4, 2, 5).contiguous().view(N, K // 2)


def shuffle_scales_mxfp4(scales: torch.Tensor) -> torch.Tensor:
    """MXFP4 scale bytes [N, K/32] (uint8, row-major) -> [N/16][K/128][16 rows][4 B]: the four scale
    bytes of row l & 15 for one 128-deep fragment are one aligned dword, which lane l of the wave
    that owns the 16-row block loads next to the fragment's codes (64 bytes per fragment, each read
    once per launch).  The same for every ``group`` of the codes.  Returned with shape [N, K/32]."""
    expect(scales.dtype == torch.uint8 and scales.dim() == 2, "shuffle_scales_mxfp4 takes scale bytes (uint8 [N, K/32])")
    N, KB = scales.shape
    expect(N % 16 == 0 and KB % 4 == 0, "shuffle_scales_mxfp4 needs N % 16 == 0 and K % 128 == 0")
    return scales.reshape(N // 16, 16, KB // 4, 4).permute(0, 2, 1, 3).contiguous().view(N, KB)


def unshuffle_scales_mxfp4(scales: torch.Tensor) -> torch.Tensor:
    """Inverse of ``shuffle_scales_mxfp4``."""
    N, KB = scales.shape
    return scales.reshape(N // 16, KB // 4, 16, 4).permute(0, 2, 1, 3).contiguous().view(N, KB)


def fp8_scan_max_m(K: int) -> int:
    """Most queries one ``score_candidates_fp8`` launch takes at width K (the scan's LDS budget)."""
    return 96 if K <= 768 else 64


def score_candidates_fp8(A, data_shuf, exps, N, thr, cap, row_group=None, q_group=None, wide: bool = False):
    """``score_candidates_shuffled`` over FP8 rows: ``data_shuf`` uint8 [R, K], e4m3fn bytes in the
    ``shuffle_weights_fp8`` layout (R >= round_up(N, 128), R % 16 == 0), ``exps`` uint8 [>= R] with one
    E8M0 exponent byte per row (``kv_quantize``).  A score is the fp32 sum over the bytes' values times
    2^(exponent byte - 127): bit-identical to ``score_candidates_shuffled`` on the dequantised rows.
    1..96 queries at K <= 768, 1..64 at K <= 1024 (K % 256 == 0): the persistent scan of
    index_scan.hip.  ``wide``: a larger batch (K % 128 == 0) is ONE launch of gemm256's candidate
    epilogue on its FP8 arm, whatever its size; without it a larger batch is refused (callers split)."""
    expect(A.is_cuda and A.dtype == torch.bfloat16, "bf16 CUDA queries required")
    M, K = A.shape
    wide = bool(wide) and M > fp8_scan_max_m(K) and K % 128 == 0
    expect(wide or (K % 256 == 0 and K <= 1024 and 1 <= M <= fp8_scan_max_m(K)),
           "FP8 scan: K % 256 == 0, 1..96 queries at K <= 768, 1..64 at K <= 1024 (wide=True: more, K % 128 == 0)")
    expect(A.stride(-1) == 1 and A.stride(0) % 8 == 0, "queries must be K-contiguous with a row stride % 8 == 0")
    expect(data_shuf.is_cuda and data_shuf.dtype == torch.uint8 and data_shuf.dim() == 2 and data_shuf.is_contiguous()
           and data_shuf.shape[1] == K, "FP8 fragment copy: contiguous uint8 [R, K]")
    expect(data_shuf.shape[0] % 16 == 0 and data_shuf.shape[0] >= -(-N // 128) * 128,
           "FP8 fragment copy needs round_up(N, 128) rows")
    expect(exps.is_cuda and exps.dtype == torch.uint8 and exps.dim() == 1 and exps.is_contiguous()
           and exps.numel() >= -(-N // 128) * 128 and exps.data_ptr() % 4 == 0,
           "exps: contiguous uint8 [>= round_up(N, 128)], 4-byte aligned")
    same_device(A, data_shuf, exps, thr)
    expect(thr.dtype == torch.float32 and thr.is_contiguous() and thr.numel() >= M, "thr must be fp32 [M]")
    if row_group is not None:
        _i32(row_group)
        expect(row_group.numel() >= N, "row_group shorter than N")
    if q_group is not None:
        _i32(q_group)
        expect(q_group.numel() >= M, "q_group shorter than M")
    cand_val = torch.full((M, cap), float("-inf"), dtype=torch.float32, device=A.device)
    cand_idx = torch.empty((M, cap), dtype=torch.int32, device=A.device)
    cnt = torch.zeros(M, dtype=torch.int32, device=A.device)
    if wide:
        native().gemm256_candidates_fp8(ptr(A), A.stride(0), ptr(data_shuf), ptr(exps), exps.numel(), M, int(N), K,
                                        ptr(row_group), ptr(q_group), ptr(thr), ptr(cnt), ptr(cand_val), ptr(cand_idx),
                                        int(cap), stream(A), data_shuf.shape[0])
        return cand_val, cand_idx, cnt
    native().score_candidates_fp8(ptr(A), A.stride(0), ptr(data_shuf), ptr(exps), M, int(N), K, ptr(row_group),
                                  ptr(q_group), ptr(thr), ptr(cnt), ptr(cand_val), ptr(cand_idx), int(cap), stream(A))
    return cand_val, cand_idx, cnt


def index_dequant_blocks(data_shuf, exps, b0: int, b1: int, out, out_block: int = 0):
    """16-row blocks [b0, b1) of an FP8 fragment copy (``data_shuf`` uint8 [R, K] in the
    ``shuffle_weights_fp8`` layout, ``exps`` uint8 [>= R]) -> the same rows as bf16 in the
    ``shuffle_weights`` layout, written to blocks [out_block, out_block + b1 - b0) of ``out`` (bf16
    [R2, K]); the rest of ``out`` is not touched.  Exact: every dequantised value is a bf16."""
    R, K = data_shuf.shape
    b0, b1, out_block = int(b0), int(b1), int(out_block)
    expect(data_shuf.dtype == torch.uint8 and data_shuf.is_contiguous() and R % 16 == 0 and K % 64 == 0,
           "FP8 fragment copy: contiguous uint8 [R, K], R % 16 == 0, K % 64 == 0")
    expect(exps.dtype == torch.uint8 and exps.dim() == 1 and exps.is_contiguous() and exps.numel() >= 16 * b1,
           "exps: contiguous uint8 with a byte for every row of the blocks")
    expect(0 <= b0 <= b1 <= R // 16, "blocks [b0, b1) must lie in the copy")
    expect(out.dtype == torch.bfloat16 and out.dim() == 2 and out.is_contiguous() and out.shape[1] == K
           and out.shape[0] % 16 == 0 and out_block >= 0 and out_block + (b1 - b0) <= out.shape[0] // 16,
           "out: contiguous bf16 [R2, K] that holds the blocks")
    same_device(data_shuf, exps, out)
    if b1 == b0:
        return out
    if not data_shuf.is_cuda:
        rows = unshuffle_weights_fp8(data_shuf[16 * b0:16 * b1])
        out[16 * out_block:16 * (out_block + b1 - b0)] = shuffle_weights(
            weight_dequantize_fp8(rows, exps[16 * b0:16 * b1]))
        return out
    native().index_dequant_blocks(ptr(data_shuf), ptr(exps), ptr(out), b0, b1, out_block, K, stream(data_shuf))
    return out


def weight_dequant_mxfp4(codes_shuf, scales_shuf, out, group: int = 1, grid_cap: int = 0):
    """MXFP4 weights -> their bf16 fragment image: ``codes_shuf`` uint8 [N, K/2] in the
    ``shuffle_weights_mxfp4(..., group)`` layout and ``scales_shuf`` uint8 [N, K/32] in the
    ``shuffle_scales_mxfp4`` layout -> ``shuffle_weights(weight_dequantize_mxfp4(codes, scales), group)``
    written to the first N K elements of ``out`` (contiguous bf16 with at least that many; the rest is
    not touched).  Exact: every dequantised value is a bf16.  Returns the [N, K] view of ``out``.
    K % 128 == 0, N % (16 group) == 0, 16-byte aligned codes / out, 4-byte aligned scales; ``group`` > 1
    needs N K 2 < 2^31 bytes (the bound of the grouped layouts).  ``grid_cap`` > 0 bounds the
    workgroups of the launch (tests: the grid-stride loop at a small shape)."""
    group, grid_cap = int(group), int(grid_cap)
    expect(codes_shuf.dtype == torch.uint8 and codes_shuf.dim() == 2 and codes_shuf.is_contiguous(),
           "codes: contiguous uint8 [N, K/2] (shuffle_weights_mxfp4)")
    N, K = codes_shuf.shape[0], codes_shuf.shape[1] * 2
    expect(group >= 1 and grid_cap >= 0, "group >= 1 and grid_cap >= 0")
    expect(N > 0 and K > 0 and K % 128 == 0 and N % (16 * group) == 0,
           "weight_dequant_mxfp4 needs K % 128 == 0 and N % (16 group) == 0")
    expect(group == 1 or N * K * 2 < (1 << 31), "grouped layouts need N K 2 < 2^31 bytes")
    expect(scales_shuf.dtype == torch.uint8 and scales_shuf.dim() == 2 and scales_shuf.is_contiguous()
           and tuple(scales_shuf.shape) == (N, K // 32), "scales: contiguous uint8 [N, K/32] (shuffle_scales_mxfp4)")
    expect(out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() >= N * K,
           "out: contiguous bf16 with at least N K elements")
    same_device(codes_shuf, scales_shuf, out)
    expect(codes_shuf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and scales_shuf.data_ptr() % 4 == 0,
           "codes / out must be 16-byte aligned, scales 4-byte aligned")
    view = out.view(-1)[:N * K].view(N, K)
    if not codes_shuf.is_cuda:
        rows = weight_dequantize_mxfp4(unshuffle_weights_mxfp4(codes_shuf, group), unshuffle_scales_mxfp4(scales_shuf))
        view.copy_(shuffle_weights(rows, group))
        return view
    native().weight_dequant_mxfp4(ptr(codes_shuf), ptr(scales_shuf), ptr(out), N, K, group, grid_cap, stream(out))
    return view


def stream_gemm(x, w, splits=1, epilogue=EPI_NONE, residual=None, out=None, nt=False, cfg=0, norm_eps: float = 0.0,
                slab_dtype=torch.float32, w_group: int = 1, w_exps=None, w_scales=None):
    """Decode GEMM y = x w^T on the warp-specialised streaming kernel (``stream_gemm.hip``): bf16
    [M, N] (optional residual add), SwiGLU [M, N/2] over 16- / 8-row interleaved [gate | up] rows, or
    fp32 K-slice slabs [S, M, N] (their sum is the product; consumers sum them in their prologue or
    ``slab_reduce`` does).  ``cfg`` picks the tile / ring configuration
    (``native().stream_gemm_bn(cfg)`` weight rows per workgroup); ``nt`` streams the weights with
    non-temporal loads.  ``norm_eps`` > 0: x is an un-normalised residual stream and w carries the
    RMSNorm gains in its columns; the kernel scales row m by rsqrt(mean(x[m]^2) + eps) (the
    consumer-side RMSNorm of small decode batches).  ``slab_dtype`` bf16: the split-K slabs are the
    partial sums rounded to bf16 (half the bytes for the producer and its consumer; the rounding the TP
    path's all-reduce input has).  On the CPU ``w`` is row-major.

    ``w_exps`` (FP8 weights, W8A16): ``w`` is the uint8 ``shuffle_weights_fp8`` copy of the e4m3fn
    bytes and ``w_exps`` [N] the rows' exponent bytes (``weight_quantize_fp8``); the result is, bit
    for bit, what the bf16 kernel gives on ``shuffle_weights(weight_dequantize_fp8(...))``.  Only
    the configurations with ``native().stream_gemm_fp8_ok(cfg)``; K % 64 == 0.

    ``w_scales`` (MXFP4 weights, W4A16; not together with ``w_exps``): ``w`` is the uint8
    ``shuffle_weights_mxfp4`` copy [N, K/2] of the e2m1 codes and ``w_scales`` the
    ``shuffle_scales_mxfp4`` copy [N, K/32] of the block scale bytes (``weight_quantize_mxfp4``); the
    result is, bit for bit, what the bf16 kernel gives on
    ``shuffle_weights(weight_dequantize_mxfp4(...))``.  Only the configurations with
    ``native().stream_gemm_mxfp4_ok(cfg)``; K % 128 == 0.  On the CPU both are row-major."""
    fp8, fp4 = w_exps is not None, w_scales is not None
    expect(not (fp8 and fp4), "w_exps (FP8 weights) and w_scales (MXFP4 weights) are mutually exclusive")
    if not x.is_cuda:
        if fp8:
            w = weight_dequantize_fp8(w, w_exps).to(x.dtype)
        if fp4:
            w = weight_dequantize_mxfp4(w, w_scales).to(x.dtype)
        y = _ref_stream_gemm(x, w, splits=splits, epilogue=epilogue, residual=residual, norm_eps=norm_eps)
        return y.to(slab_dtype) if splits > 1 else y
    expect(norm_eps <= 0 or residual is None, "the consumer RMSNorm takes no residual add")
    if fp8:
        expect(x.dtype == torch.bfloat16 and w.dtype == torch.uint8, "FP8 weights: bf16 x, uint8 fragment copy")
        expect(native().stream_gemm_fp8_ok(cfg), f"stream_gemm cfg {cfg} has no FP8-weight instantiation")
        expect(w.dim() == 2 and w.shape[1] % 64 == 0, "FP8 weights need K % 64 == 0")
        expect(w_exps.dtype == torch.uint8 and w_exps.is_cuda and w_exps.dim() == 1 and w_exps.shape[0] == w.shape[0]
               and w_exps.is_contiguous() and w_exps.data_ptr() % 4 == 0,
               "w_exps must be the uint8 [N] row exponents (contiguous, 4-byte aligned)")
    elif fp4:
        expect(x.dtype == torch.bfloat16 and w.dtype == torch.uint8 and w.is_cuda and w.dim() == 2 and w.is_contiguous()
               and w.data_ptr() % 16 == 0, "MXFP4 weights: bf16 x, contiguous 16-byte aligned uint8 fragment copy [N, K/2]")
        expect(native().stream_gemm_mxfp4_ok(cfg), f"stream_gemm cfg {cfg} has no MXFP4-weight instantiation")
        expect(w.shape[1] % 64 == 0, "MXFP4 weights need K % 128 == 0")
        expect(w_scales.dtype == torch.uint8 and w_scales.is_cuda and w_scales.dim() == 2
               and tuple(w_scales.shape) == (w.shape[0], w.shape[1] // 16) and w_scales.is_contiguous()
               and w_scales.data_ptr() % 4 == 0,
               "w_scales must be the uint8 [N, K/32] shuffle_scales_mxfp4 copy (contiguous, 4-byte aligned)")
        same_device(x, w, w_scales)
    else:
        expect(x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16, "bf16 operands required")
    expect(x.stride(-1) == 1 and w.stride(-1) == 1, "operands must be K-contiguous")
    M, K = x.shape
    N = w.shape[0]
    bn = native().stream_gemm_bn(cfg)
    expect(bn > 0 and M <= native().stream_gemm_max_m(cfg), f"stream_gemm cfg {cfg}: bad config or M too large")
    expect(w.shape[1] * (2 if fp4 else 1) == K and N % bn == 0 and K % (splits * STREAM_KS) == 0,
           f"stream_gemm needs N % {bn} == 0 and K % ({STREAM_KS}*splits) == 0")
    expect(x.stride(0) % 8 == 0 and w.stride(0) % 8 == 0, "row strides must be multiples of 8")
    if native().stream_gemm_shuffled(cfg):
        expect(w.is_contiguous(), "shuffled-layout configurations take a contiguous shuffle_weights() tensor")
    if splits > 1:
        expect(epilogue == EPI_NONE and residual is None, "split-K writes raw slabs")
        expect(slab_dtype in (torch.float32, torch.bfloat16), "slabs are fp32 or bf16")
        if out is None:
            out = torch.empty((splits, M, N), dtype=slab_dtype, device=x.device)
        expect(out.dtype == slab_dtype and out.is_contiguous() and tuple(out.shape) == (splits, M, N), "bad slabs")
        ldo = N
    else:
        n_out = N // 2 if epilogue in (EPI_SWIGLU, EPI_SWIGLU8) else N
        if residual is not None:
            expect(epilogue == EPI_NONE and residual.dtype == torch.bfloat16 and residual.stride(-1) == 1
                   and tuple(residual.shape) == (M, N), "residual must be bf16 [M, N]")
        if epilogue == EPI_SWIGLU:
            expect(bn % 32 == 0, f"stream_gemm cfg {cfg}: EPI_SWIGLU needs 32-row tiles (use EPI_SWIGLU8)")
        if out is None:
            out = torch.empty((M, n_out), dtype=torch.bfloat16, device=x.device)
        expect(out.dtype == torch.bfloat16 and out.stride(-1) == 1 and tuple(out.shape) == (M, n_out), "bad output")
        ldo = out.stride(0)
    if fp8:
        native().stream_gemm_fp8(ptr(x), x.stride(0), ptr(w), ptr(w_exps), ptr(out), ldo, ptr(residual),
                                 residual.stride(0) if residual is not None else 0, M, N, K, splits, int(epilogue),
                                 stream(x), int(bool(nt)), int(cfg), float(norm_eps),
                                 int(splits > 1 and out.dtype == torch.bfloat16), int(w_group))
        return out
    if fp4:
        native().stream_gemm_mxfp4(ptr(x), x.stride(0), ptr(w), ptr(w_scales), ptr(out), ldo, ptr(residual),
                                   residual.stride(0) if residual is not None else 0, M, N, K, splits, int(epilogue),
                                   stream(x), int(bool(nt)), int(cfg), float(norm_eps),
                                   int(splits > 1 and out.dtype == torch.bfloat16), int(w_group))
        return out
    native().stream_gemm(ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(out), ldo, ptr(residual),
                         residual.stride(0) if residual is not None else 0, M, N, K, splits, int(epilogue), stream(x),
                         int(bool(nt)), int(cfg), float(norm_eps), int(splits > 1 and out.dtype == torch.bfloat16),
                         int(w_group))
    return out


def slab_reduce(slabs, residual=None, out=None):
    """fp32 / bf16 slabs [S, M, N] -> bf16 [M, N] (fp32 sum rounded to bf16, then + residual)."""
    if not slabs.is_cuda:
        y = slabs.float().sum(0).to(torch.bfloat16)
        return y if residual is None else (y.float() + residual.float()).to(torch.bfloat16)
    S, M, N = slabs.shape
    expect(slabs.dtype in (torch.float32, torch.bfloat16) and slabs.is_contiguous() and N % 8 == 0, "bad slabs")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=slabs.device)
    if residual is not None:
        expect(residual.dtype == torch.bfloat16 and tuple(residual.shape) == (M, N) and residual.stride(-1) == 1,
               "residual must be bf16 [M, N]")
    native().slab_reduce(ptr(out), out.stride(0), ptr(slabs), S, M, N, ptr(residual),
                         residual.stride(0) if residual is not None else 0, stream(slabs),
                         int(slabs.dtype == torch.bfloat16))
    return out


def interleave_gate_up(w_gate: torch.Tensor, w_up: torch.Tensor, group: int = 16) -> torch.Tensor:
    """[F, H] gate and up weights -> [2F, H] interleaved in ``group``-row groups [g | u | g | u ...]
    (16: the layout the SWIGLU epilogue of gemm_bt / gemm256 consumes; 8: EPI_SWIGLU8)."""
    Fd, H = w_gate.shape
    assert Fd % group == 0
    g = w_gate.reshape(Fd // group, group, H)
    u = w_up.reshape(Fd // group, group, H)
    return torch.stack([g, u], dim=1).reshape(2 * Fd, H).contiguous()


def regroup_gate_up(w: torch.Tensor, src: int = 16, dst: int = 8) -> torch.Tensor:
    """Re-interleave [2F, H] gate|up weights from ``src``-row to ``dst``-row groups."""
    n2, H = w.shape
    v = w.reshape(n2 // (2 * src), 2, src, H)
    gate, up = v[:, 0].reshape(n2 // 2, H), v[:, 1].reshape(n2 // 2, H)
    return interleave_gate_up(gate, up, dst)


# ----------------------------------------------------------------------------------------------
# selection


SAMPLE_FAST_MAX_K = 64
_CHUNK = 256 * 32


def sample_workspace(rows: int, vocab: int, device) -> torch.Tensor:
    ncand = -(-vocab // _CHUNK) * SAMPLE_FAST_MAX_K
    return torch.empty((rows * ncand * 8,), dtype=torch.uint8, device=device)


def sample_tokens(logits, temperature, top_k, top_p, seed: int, counters, generator=None, out=None,
                  fast: bool | None = None, workspace: torch.Tensor | None = None):
    """temperature / top_k (int32) / top_p per row; counters int64 per row (advanced in-kernel).

    ``fast`` (every row has 0 < top_k <= 64, the reference's 50 included) selects the two-stage kernel:
    per-chunk register-resident top-64 over many workgroups, then a per-row merge + top-p + sample."""
    if not logits.is_cuda:
        return ref.sample_hf(logits, temperature, top_k, top_p, generator)
    rows, vocab = logits.shape
    expect(logits.stride(-1) == 1, "logits rows must be contiguous")
    expect(logits.dtype in (torch.float32, torch.bfloat16), "logits must be fp32 or bf16")
    expect(temperature.dtype == torch.float32 and temperature.numel() >= rows, "temperature")
    expect(top_p.dtype == torch.float32 and top_p.numel() >= rows, "top_p")
    _i32(top_k)
    expect(counters.dtype == torch.int64 and counters.numel() >= rows, "counters")
    out = torch.empty((rows,), dtype=torch.int32, device=logits.device) if out is None else out
    if fast is None:
        fast = False
    ncand = -(-vocab // _CHUNK) * SAMPLE_FAST_MAX_K
    if fast and ncand <= 1024:
        ws = workspace if workspace is not None else sample_workspace(rows, vocab, logits.device)
        expect(ws.numel() >= rows * ncand * 8, "sampling workspace too small")
        native().sample_tokens_2stage(ptr(logits), int(logits.dtype == torch.float32), logits.stride(0), rows, vocab,
                                      ptr(temperature), ptr(top_k), ptr(top_p), int(seed) & ((1 << 64) - 1),
                                      ptr(counters), ptr(out), ptr(ws), ws.numel(), stream(logits))
    else:
        native().sample_tokens(ptr(logits), int(logits.dtype == torch.float32), logits.stride(0), rows, vocab,
                               ptr(temperature), ptr(top_k), ptr(top_p), int(seed) & ((1 << 64) - 1), ptr(counters),
                               ptr(out), 0, stream(logits))
    return out


def mask_logits(logits, mask, row_flags, vocab: int | None = None, word_offset: int = 0):
    """In place: logits[r, t] = -inf where bit t of ``mask[r]`` (int32 words, bit t % 32 of word
    t // 32) is clear, for the rows whose ``row_flags[r]`` (int32) is non-zero (JSON-constrained
    decoding).  Vocab-parallel slices: the first ``vocab`` columns of ``logits`` are tokens
    32 * ``word_offset`` ... (mask words ``word_offset`` ...).  Returns ``logits``."""
    rows = logits.shape[0]
    vocab = logits.shape[1] if vocab is None else int(vocab)
    words = -(-vocab // 32)
    expect(mask.dtype == torch.int32 and mask.is_contiguous() and mask.shape[0] >= rows
           and mask.shape[1] >= word_offset + words, "mask: int32 [rows, >= ceil(vocab / 32) words past the offset]")
    if not logits.is_cuda:
        m = mask[:rows, word_offset:word_offset + words]
        bits = (m.view(torch.int32).unsqueeze(-1) >> torch.arange(32, dtype=torch.int32)) & 1
        allow = bits.reshape(rows, -1)[:, :vocab].bool() | (row_flags[:rows] == 0).unsqueeze(1)
        logits[:, :vocab].masked_fill_(~allow, float("-inf"))
        return logits
    expect(logits.stride(-1) == 1 and logits.dtype in (torch.float32, torch.bfloat16), "logits: fp32/bf16 rows")
    _i32(row_flags)
    native().mask_logits(ptr(logits), int(logits.dtype == torch.float32), logits.stride(0), rows, vocab,
                         ptr(mask) + 4 * int(word_offset), words, ptr(row_flags), stream(logits), mask.stride(0))
    return logits


def sample_candidates(logits, vocab: int, index_base: int = 0, out=None):
    """Stage 1 of vocab-parallel sampling: each 8192-token chunk's top-64 of the first ``vocab``
    columns of ``logits`` as (order-preserving uint32 key, token id + ``index_base``) -> int32
    [2, rows, ncand] (keys, then ids).  The TP ranks all-gather these and ``sample_merge`` draws
    from the union (GPU only)."""
    expect(logits.is_cuda and logits.stride(-1) == 1 and logits.dtype in (torch.float32, torch.bfloat16),
           "logits: CUDA fp32/bf16 rows")
    rows = logits.shape[0]
    ncand = sample_candidates_per_row(vocab)
    if out is None:
        out = torch.empty((2, rows, ncand), dtype=torch.int32, device=logits.device)
    # (a row slice of a larger [2, R, ncand] buffer is fine: each half is rows x ncand contiguous)
    expect(out.dtype == torch.int32 and tuple(out.shape) == (2, rows, ncand) and out.stride(2) == 1
           and out.stride(1) == ncand, "candidates: int32 [2, rows, ncand] with contiguous halves")
    native().sample_candidates(ptr(logits), int(logits.dtype == torch.float32), logits.stride(0), rows, int(vocab),
                               int(index_base), ptr(out[0]), ptr(out[1]), ncand, stream(logits))
    return out


def sample_candidates_per_row(vocab: int) -> int:
    return -(-int(vocab) // _CHUNK) * SAMPLE_FAST_MAX_K


def sample_merge(cands, temperature, top_k, top_p, seed: int, counters, vocab: int, out=None):
    """Stage 2 of vocab-parallel sampling: ``cands`` int32 [2, rows, n] (every rank's
    ``sample_candidates`` side by side along n, n <= 1024) -> sorted top-k -> HF top-p ->
    multinomial with the per-row counter RNG (advanced in-kernel): the replicated head's draw."""
    two, rows, n = cands.shape
    expect(two == 2 and n <= 1024 and cands.dtype == torch.int32 and cands.is_contiguous(),
           "candidates: contiguous int32 [2, rows, <= 1024]")
    out = torch.empty((rows,), dtype=torch.int32, device=cands.device) if out is None else out
    _i32(top_k)
    native().sample_merge(ptr(cands[0]), ptr(cands[1]), n, rows, int(vocab), ptr(temperature), ptr(top_k), ptr(top_p),
                          int(seed) & ((1 << 64) - 1), ptr(counters), ptr(out), stream(cands))
    return out


def topk_rows(scores, k, index_base=0, want_global=False):
    """Exact per-row top-k of fp32 scores, sorted descending.  Returns (values, idx int32) or, with
    ``want_global``, (values, idx + index_base as int64).  Long rows use the two-stage kernel."""
    rows, n = scores.shape
    expect(1 <= k <= min(n, 1024), "1 <= k <= min(n, 1024)")
    if rows == 0:  # e.g. a rank with no queries in a sharded search (an empty view's strides are arbitrary)
        return (torch.empty((0, k), dtype=torch.float32, device=scores.device),
                torch.empty((0, k), dtype=torch.int64 if want_global else torch.int32, device=scores.device))
    if not scores.is_cuda:
        v, i = ref.topk_rows(scores, k)
        return (v, i.long() + index_base) if want_global else (v, i)
    expect(scores.dtype == torch.float32 and scores.stride(-1) == 1, "scores must be fp32 with contiguous rows")
    vals = torch.empty((rows, k), dtype=torch.float32, device=scores.device)
    if want_global:
        idx = torch.empty((rows, k), dtype=torch.int64, device=scores.device)
        i32, i64 = 0, ptr(idx)
    else:
        idx = torch.empty((rows, k), dtype=torch.int32, device=scores.device)
        i32, i64 = ptr(idx), 0
    if n >= 4 * _CHUNK:
        kc = -(-k // 64) * 64
        ncand = -(-n // _CHUNK) * kc
        ws = torch.empty((rows * ncand * 8,), dtype=torch.uint8, device=scores.device)
        native().topk_rows_2stage(ptr(scores), scores.stride(0), rows, n, k, ptr(vals), i32, int(index_base), i64,
                                  ptr(ws), ws.numel(), stream(scores))
    else:
        native().topk_rows(ptr(scores), scores.stride(0), rows, n, k, ptr(vals), i32, int(index_base), i64,
                           stream(scores))
    return vals, idx


def linear(x, w, b=None, residual=None, act=None):
    """y = x W^T (+b) (+act) (+residual) on the native MFMA GEMMs (``gemm_bt``: the phased 256x256
    kernel for large token counts, the 128x128 kernel otherwise), epilogues fused.

    Widths the kernels do not tile (K % 64, N % 4) are zero-padded to the next native shape (zero
    k-columns add nothing to a dot product; padded output columns are sliced off), so every GPU
    call runs the native kernel -- there is no torch fallback (``ops/_lib.py`` dispatch rule)."""
    epi = {None: EPI_NONE, "gelu": EPI_GELU, "swiglu": EPI_SWIGLU}[act]
    if not x.is_cuda:
        return ref.gemm_bt(x, w, b, residual, epi)
    K, N = x.shape[-1], w.shape[0]
    expect(epi != EPI_SWIGLU or N % 32 == 0, "swiglu linear needs 16-row [gate | up] groups (N % 32 == 0)")
    x2 = x.reshape(-1, K)
    r2 = residual.reshape(x2.shape[0], -1) if residual is not None else None
    pk, pn = (-K) % 64, (-N) % 4
    if pk or pn:
        x2 = F.pad(x2, (0, pk)) if pk else x2
        w = F.pad(w, (0, pk, 0, pn))
        b = F.pad(b, (0, pn)) if (b is not None and pn) else b
        r2 = F.pad(r2, (0, pn)) if (r2 is not None and pn) else r2
    y = gemm_bt(x2, w, b, r2, epi)
    if pn:
        y = y[:, :N].contiguous()
    return y.view(*x.shape[:-1], y.shape[-1])
