"""Llama-3 family decoder on the native kernels with a paged KV cache and tensor parallelism.

Replaces HF ``AutoModelForCausalLM.generate`` of the reference (ai/providers/transformers.py:35-94).
One forward serves both phases:

  * prefill (packed variable-length prompt chunks; flash attention reads K/V from the paged cache,
    so chunked prefill and cached shared prefixes need no special path);
  * decode (one token per running sequence; split-K paged decode attention), capturable in a HIP
    graph because every op enqueues on the current stream with fixed shapes.

Per layer:  RMSNorm(+residual) -> QKV GEMM -> RoPE + KV-cache write -> attention -> O GEMM
[-> TP all-reduce] -> RMSNorm(+residual) -> gate|up GEMM (+fused SwiGLU) -> down GEMM
[-> TP all-reduce].  Under TP each rank owns Hq/tp query heads, Hkv/tp KV heads and F/tp MLP
columns (Megatron split); the two all-reduces per layer run on the RCCL process group.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import ops
from ..ops import reference as ref
from .configs import DecoderConfig


@dataclass
class DecoderLayer:
    """One layer's tensors.  On the GPU the four projections are held ONCE, in the
    ``ops.shuffle_weights`` fragment layout, which the decode GEMM (stream_gemm) streams and the
    prefill GEMMs (gemm256 / gemm_bt ``shuffled``) stage by LDS-DMA; on the CPU they are row-major.
    Under ``weight_dtype="fp8"`` (GPU, fragment layout) each projection is an ``Fp8Proj``, under
    ``weight_dtype="mxfp4"`` an ``Mxfp4Proj``."""

    attn_norm: torch.Tensor
    qkv_w: torch.Tensor
    o_w: torch.Tensor
    mlp_norm: torch.Tensor
    gate_up_w: torch.Tensor  # [gate 8 | up 8] row groups (interleaved) or [gate; up] (stacked)
    down_w: torch.Tensor


class Fp8Proj:
    """One projection of a ``weight_dtype="fp8"`` decoder on the GPU, held twice: ``data`` / ``exps``,
    the e4m3fn bytes in the ``ops.shuffle_weights_fp8`` layout and one power-of-two exponent byte per
    output row, streamed by the decode GEMM (stream_gemm's FP8 arm), and ``w``, a bf16
    ``ops.shuffle_weights`` copy of the DEQUANTISED values for the MFMA GEMMs (gemm256 / gemm_mid /
    gemm_bt).  Both hold the same numbers, so prefill, mixed steps and every decode batch compute
    with identical weights.  ``group``: the row-block group of both copies.

    ``fp8_weights_only``: ``w`` is None and the FP8 bytes are the ONLY copy; the MFMA GEMMs then run
    the FP8 arm of gemm256 (``ops.gemm_bt(..., w_exps=)``), which gives the same numbers."""

    __slots__ = ("w", "data", "exps", "group")

    def __init__(self, w: torch.Tensor | None, data: torch.Tensor, exps: torch.Tensor, group: int = 1):
        self.w, self.data, self.exps, self.group = w, data, exps, group

    @classmethod
    def from_rows(cls, data: torch.Tensor, exps: torch.Tensor, group: int = 1, bf16_copy: bool = True) -> "Fp8Proj":
        """From row-major e4m3fn bytes [N, K] and row exponents [N] (``ops.weight_quantize_fp8``)."""
        w = ops.shuffle_weights(ops.weight_dequantize_fp8(data, exps), group) if bf16_copy else None
        return cls(w, ops.shuffle_weights_fp8(data, group), exps.contiguous(), group)

    @property
    def shape(self):
        return self.data.shape  # [N, K], as the bf16 copy's

    def nbytes(self) -> int:
        """Bytes resident for this projection, counted from its tensors."""
        return sum(t.numel() * t.element_size() for t in (self.w, self.data, self.exps) if t is not None)

    def regroup(self, group: int) -> None:
        """Re-lay both copies for ``group``, in place (pointers stay valid)."""
        if self.w is not None:
            self.w.copy_(ops.shuffle_weights(ops.unshuffle_weights(self.w, self.group), group))
        self.data.copy_(ops.shuffle_weights_fp8(ops.unshuffle_weights_fp8(self.data, self.group), group))
        self.group = group


class Mxfp4Proj:
    """One projection of a ``weight_dtype="mxfp4"`` decoder on the GPU, held twice: ``data`` / ``scales``,
    the e2m1 codes in the ``ops.shuffle_weights_mxfp4`` layout and one E8M0 scale byte per 32 k of a
    row in the ``ops.shuffle_scales_mxfp4`` layout, streamed by the decode GEMM (stream_gemm's MXFP4
    arm), and ``w``, a bf16 ``ops.shuffle_weights`` copy of the DEQUANTISED values for the MFMA GEMMs
    and every stream_gemm configuration without an MXFP4 arm.  Both hold the same numbers.
    ``group``: the row-block group of the codes and of the bf16 copy (the scales have one layout).

    ``mxfp4_weights_only``: ``w`` is None and the codes and scales are the ONLY copy; a call without an
    MXFP4 arm reads a bf16 image that ``ops.weight_dequant_mxfp4`` writes into the model's scratch right
    before it (``LlamaModel._bf16_w``): the same bytes ``w`` would hold."""

    __slots__ = ("w", "data", "scales", "group")

    def __init__(self, w: torch.Tensor | None, data: torch.Tensor, scales: torch.Tensor, group: int = 1):
        self.w, self.data, self.scales, self.group = w, data, scales, group

    @classmethod
    def from_rows(cls, codes: torch.Tensor, scales: torch.Tensor, group: int = 1,
                  bf16_copy: bool = True) -> "Mxfp4Proj":
        """From row-major codes [N, K/2] and scale bytes [N, K/32] (``ops.weight_quantize_mxfp4``)."""
        w = ops.shuffle_weights(ops.weight_dequantize_mxfp4(codes, scales), group) if bf16_copy else None
        return cls(w, ops.shuffle_weights_mxfp4(codes, group), ops.shuffle_scales_mxfp4(scales), group)

    @property
    def shape(self):
        return torch.Size((self.data.shape[0], 2 * self.data.shape[1]))  # [N, K], as the bf16 copy's

    def nbytes(self) -> int:
        """Bytes resident for this projection, counted from its tensors."""
        return sum(t.numel() * t.element_size() for t in (self.w, self.data, self.scales) if t is not None)

    def regroup(self, group: int) -> None:
        """Re-lay both copies for ``group``, in place (pointers stay valid)."""
        if self.w is not None:
            self.w.copy_(ops.shuffle_weights(ops.unshuffle_weights(self.w, self.group), group))
        self.data.copy_(ops.shuffle_weights_mxfp4(ops.unshuffle_weights_mxfp4(self.data, self.group), group))
        self.group = group


def _bf16_copy(w):
    """The bf16 tensor of a projection (a tensor, or an ``Fp8Proj``'s / ``Mxfp4Proj``'s dequantised copy)."""
    return w.w if isinstance(w, (Fp8Proj, Mxfp4Proj)) else w


@dataclass
class AttnMeta:
    """Per-forward batch description (device tensors, fixed shapes in decode graphs)."""

    decode: bool
    positions: torch.Tensor  # int32 [T]
    slots: torch.Tensor  # int64 [T] cache slot of each token (<0 = padding)
    block_tables: torch.Tensor  # int32 [B, max_blocks]
    ctx_lens: torch.Tensor  # int32 [B] total tokens in cache after this step
    cu_q: torch.Tensor | None = None  # int32 [B+1] (prefill)
    max_q: int = 1
    workspace: ops.DecodeWorkspace | None = None
    part_size: int = 512
    # mixed step: the LAST n_decode tokens are single-token decode rows (one per sequence) with their
    # own block tables / context lengths; the tokens before them are prefill chunks described above
    n_decode: int = 0
    dec_block_tables: torch.Tensor | None = None
    dec_ctx_lens: torch.Tensor | None = None
    order: torch.Tensor | None = None  # int32 [B] decode attention dispatch order (longest context first;
    # of the decode rows in a mixed step)
    # FP8 KV cache, prefill rows (``ops.kv_prefill_plan``, built once per step on the host): the
    # step's context blocks group after group, the block table into the bf16 scratch they are
    # dequantised to, and the groups of whole sequences that fit the scratch
    kv_blocks: torch.Tensor | None = None
    kv_scratch_bt: torch.Tensor | None = None
    kv_groups: list | None = None


class _Partial:
    """This rank's un-reduced TP partial sum of a row-parallel projection (fp32 split-K slabs or
    bf16): the all-reduce is still due and runs fused into the RMSNorm that consumes it
    (``LlamaModel._norm``: one launch instead of slab_reduce + all-reduce + rmsnorm)."""

    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        self.t = t


class KVCache:
    """Paged KV cache: per layer [num_blocks, Hkv_local, block_size, D] for K and for V.

    ``kv_dtype="fp8"`` (opt-in, D = 128 on the GPU): ``k`` / ``v`` hold OCP e4m3fn bytes (uint8) and
    ``k_exp`` / ``v_exp`` [layers, num_blocks, Hkv, block_size] one power-of-two exponent byte per
    (token, kv head) row (docs/ARCHITECTURE.md "FP8 KV cache").  The prefill attention reads a bf16
    image of the step's context blocks from ``scratch_k`` / ``scratch_v`` [scratch_blocks, Hkv,
    block_size, D], one layer at a time; the scratch belongs to the cache (hence to the engine): two
    engines sharing one model on two streams each dequantise into their own.

    Every cache touch of the model goes through ``write``, ``decode_attention`` and
    ``prefill_attention``."""

    def __init__(self, layers, num_blocks, kv_heads, block_size, head_dim, device, dtype=torch.bfloat16,
                 kv_dtype: str = "bf16", scratch_blocks: int = 0):
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"kv_dtype must be 'bf16' or 'fp8', got {kv_dtype!r}")
        self.num_blocks, self.block_size = num_blocks, block_size
        self.kv_dtype = kv_dtype
        self.fp8 = kv_dtype == "fp8"
        self.k_exp = self.v_exp = self.scratch_k = self.scratch_v = None
        self.scratch_blocks = 0
        if not self.fp8:
            self.k = torch.zeros((layers, num_blocks, kv_heads, block_size, head_dim), device=device, dtype=dtype)
            self.v = torch.zeros_like(self.k)
            return
        dev = torch.device(device)
        if dev.type == "cuda" and head_dim != 128:
            raise ValueError("the FP8 KV cache kernels take head_dim 128 only")
        self.k = torch.zeros((layers, num_blocks, kv_heads, block_size, head_dim), device=dev, dtype=torch.uint8)
        self.v = torch.zeros_like(self.k)
        # exponent 127 (scale 1) over zero bytes: an untouched slot reads as 0.0
        self.k_exp = torch.full((layers, num_blocks, kv_heads, block_size), 127, device=dev, dtype=torch.uint8)
        self.v_exp = torch.full_like(self.k_exp, 127)
        if dev.type == "cuda":
            self.scratch_blocks = max(1, int(scratch_blocks) or num_blocks)
            self.scratch_k = torch.zeros((self.scratch_blocks, kv_heads, block_size, head_dim), device=dev, dtype=dtype)
            self.scratch_v = torch.zeros_like(self.scratch_k)

    @staticmethod
    def bytes_per_block(layers, kv_heads, block_size, head_dim, dtype=torch.bfloat16, kv_dtype: str = "bf16"):
        if kv_dtype == "fp8":  # data + one exponent byte per row
            return 2 * layers * kv_heads * block_size * (head_dim + 1)
        return 2 * layers * kv_heads * block_size * head_dim * torch.finfo(dtype).bits // 8

    @staticmethod
    def scratch_bytes(scratch_blocks, kv_heads, block_size, head_dim, dtype=torch.bfloat16):
        return 2 * scratch_blocks * kv_heads * block_size * head_dim * torch.finfo(dtype).bits // 8

    def write(self, li, qkv, positions, cos_sin, slots, Hq, Hkv, D, write_q=True):
        """RoPE on q / k and the cache write of layer ``li``: -> q [T, Hq, D] (None: ``write_q`` off)."""
        if self.fp8:
            return ops.rope_kv_write_fp8(qkv, positions, cos_sin, self.k[li], self.k_exp[li], self.v[li], self.v_exp[li],
                                         slots, Hq, Hkv, D, write_q=write_q)
        return ops.rope_kv_write(qkv, positions, cos_sin, self.k[li], self.v[li], slots, Hq, Hkv, D, write_q=write_q)

    def decode_attention(self, li, q, block_tables, ctx_lens, part_size, workspace, out=None, order=None, warm=None):
        if self.fp8:  # (``warm``: refused by the FP8 op)
            return ops.paged_decode_fp8(q, self.k[li], self.k_exp[li], self.v[li], self.v_exp[li], block_tables, ctx_lens,
                                        part_size, workspace, out=out, order=order, warm=warm)
        return ops.paged_decode(q, self.k[li], self.v[li], block_tables, ctx_lens, part_size, workspace, out=out,
                                order=order, warm=warm)

    def prefill_attention(self, li, q, meta, out=None, rope=None):
        """Causal prefill attention of the step's prefill rows ``q`` over layer ``li``."""
        if not self.fp8:
            return ops.flash_attention_paged(q, self.k[li], self.v[li], meta.block_tables, meta.cu_q, meta.ctx_lens,
                                             meta.max_q, causal=True, out=out, rope=rope)
        plan = None
        if q.is_cuda:
            if meta.kv_groups is None:  # a caller without a host plan (tests, tools): built once, synchronises
                p = ops.kv_prefill_plan(meta.block_tables, meta.ctx_lens, meta.cu_q, self.block_size,
                                        self.scratch_blocks, q.device)
                meta.kv_blocks, meta.kv_scratch_bt, meta.kv_groups = p.blocks, p.scratch_bt, p.groups
            plan = ops.KVPrefillPlan(meta.kv_blocks, meta.kv_scratch_bt, meta.kv_groups)
        return ops.flash_attention_paged_fp8(q, self.k[li], self.k_exp[li], self.v[li], self.v_exp[li], meta.block_tables,
                                             meta.cu_q, meta.ctx_lens, meta.max_q, causal=True, out=out, rope=rope,
                                             scratch=(self.scratch_k, self.scratch_v), plan=plan)


class LlamaModel:
    # rows of a vocab-parallel LM head shard are padded to a multiple of this (every stream_gemm
    # tile height and the fragment layout divide it); the pad rows are zero and never sampled
    VOCAB_PAD = 384

    def __init__(self, cfg: DecoderConfig, weights: dict, device, tp_group=None, tp_size: int = 1,
                 interleaved_mlp: bool = False, fragment_layout: bool = True, consume: bool = False,
                 tp_rank: int | None = None, vocab_parallel: bool = True, small_norm_fused: bool | None = None,
                 weight_dtype: str = "bf16", fp8_weights_only: bool = False, mxfp4_weights_only: bool = False,
                 mxfp4_mid: bool = False):
        """``weight_dtype="fp8"`` (opt-in, TP 1): the qkv / o / gate_up / down weights are quantised at
        load time to e4m3fn bytes with one power-of-two exponent per output row
        (``ops.weight_quantize_fp8``) and the model computes with the dequantised values everywhere.
        On the GPU with the fragment layout each projection is an ``Fp8Proj``: the decode GEMM
        streams the FP8 bytes (half the weight traffic of a decode step), the prefill GEMMs read a
        bf16 copy of the same values.  A bandwidth feature, not a capacity one: the projections take
        1.5x the bf16 model's memory.  Embedding, norms and LM head stay bf16.  On the CPU (or
        without the fragment layout) the weights are the dequantised row-major tensors.

        ``fp8_weights_only`` (opt-in on top of ``weight_dtype="fp8"``, TP 1, fragment layout): the FP8
        bytes are the only copy of every projection (half the bf16 model's projection memory, a third
        of the two-copy FP8 model's).  Streamed calls read them through stream_gemm's FP8 arm, every
        other call through the FP8 arm of gemm256 (``ops.gemm_bt(..., w_exps=)``) at any M, so
        gemm_mid and the 128 x 128 kernel are never reached and every projection needs N % 256 == 0
        and K % 128 == 0 on the GPU (ValueError otherwise).  The numbers are those of the two-copy model
        wherever that one takes gemm256 or stream_gemm; elsewhere they differ in accumulation order only.
        On the CPU it changes nothing (the model already runs on dequantised row-major weights).

        ``weight_dtype="mxfp4"`` (opt-in, TP 1, not with ``fp8_weights_only``): the same projections are
        quantised at load time to OCP MXFP4 (``ops.weight_quantize_mxfp4``: e2m1 codes and one
        power-of-two scale per 32 k of a row, 4.25 bits per weight) and the model computes with the
        dequantised values everywhere.  On the GPU with the fragment layout and K % 128 == 0 each
        projection is an ``Mxfp4Proj``: the decode GEMM streams the codes and scales wherever its
        configuration has an MXFP4 arm, everything else reads a bf16 copy of the same values
        (1.27x the bf16 model's projection memory).  Otherwise the weights are the dequantised tensors.

        ``mxfp4_weights_only`` (opt-in on top of ``weight_dtype="mxfp4"``, TP 1, fragment layout, not with
        ``fp8_weights_only``): the codes and scales are the only copy of every projection (4.25 / 16 of
        the bf16 model's projection memory).  Dispatch does not change: a streamed call whose
        configuration has an MXFP4 arm reads the codes, every other call takes the kernel the two-copy
        model takes, on a bf16 image that ``ops.weight_dequant_mxfp4`` writes right before it into one
        scratch the size of the largest projection (``_bf16_w``; ``mxfp4_scratch_bytes``).  The image
        holds the bytes the two-copy model keeps resident, so every step is bit-identical to that
        model's.  Every projection must become an ``Mxfp4Proj`` on the GPU (K % 128 == 0, fragment
        layout; ValueError otherwise).  On the CPU it changes nothing.

        ``mxfp4_mid`` (opt-in on top of ``weight_dtype="mxfp4"``, TP 1, fragment layout; with or without
        ``mxfp4_weights_only``): an ``Mxfp4Proj`` call that would take ``gemm_mid`` (``ops.kernels.use_gemm_mid``)
        runs that kernel's MXFP4 arm on the codes and scales (``ops.gemm_bt(..., w_scales=)``) instead of
        its bf16 copy, or, in the one-copy mode, instead of the dequantiser and the scratch image.  Bit for
        bit the same result; projections named in ``MXFP4_MID_OFF`` and every other call keep today's
        path.  On the CPU it changes nothing.

        ``consume``: the entries of ``weights`` are popped as the model takes them over, so each
        original is freed as soon as its fragment-layout copy exists (peak HBM = model + one
        tensor: 70B at TP 1 needs it, 2 x 140 GB would not fit in 288 GB).

        ``vocab_parallel`` (TP > 1): the LM head is split by vocabulary rows, rank r keeping tokens
        [r V/tp, (r+1) V/tp) (a replicated head streamed the whole 2.1 GB 70B head
        on every rank every step).  Each rank then produces the logits of its slice only; the engine
        samples from the all-gathered per-slice candidates (``ops.sample_candidates`` /
        ``sample_merge``).  Needs V % (32 tp) == 0 (whole JSON-mask words per slice); otherwise the
        head stays replicated."""
        if weight_dtype not in ("bf16", "fp8", "mxfp4"):
            raise ValueError(f"weight_dtype must be 'bf16', 'fp8' or 'mxfp4', got {weight_dtype!r}")
        if weight_dtype != "bf16" and tp_size > 1:
            raise ValueError(f"weight_dtype={weight_dtype!r} is not supported under tensor parallelism (tp_size > 1)")
        self.weight_dtype = weight_dtype
        self.fp8_weights_only = bool(fp8_weights_only)
        if self.fp8_weights_only:
            if weight_dtype != "fp8":
                raise ValueError("fp8_weights_only needs weight_dtype='fp8'")
            if not fragment_layout:
                raise ValueError("fp8_weights_only needs the fragment layout (fragment_layout=True)")
            if not self.fp8_stream or self.FP8_STREAM_OFF:
                raise ValueError("fp8_weights_only keeps no bf16 copy for fp8_stream=False / FP8_STREAM_OFF to stream")
        self.mxfp4_weights_only = bool(mxfp4_weights_only)
        if self.mxfp4_weights_only:
            if self.fp8_weights_only:
                raise ValueError("mxfp4_weights_only and fp8_weights_only are mutually exclusive")
            if weight_dtype != "mxfp4":
                raise ValueError("mxfp4_weights_only needs weight_dtype='mxfp4'")
            if not fragment_layout:
                raise ValueError("mxfp4_weights_only needs the fragment layout (fragment_layout=True)")
        self.mxfp4_mid = bool(mxfp4_mid)
        if self.mxfp4_mid:
            if weight_dtype != "mxfp4":
                raise ValueError("mxfp4_mid needs weight_dtype='mxfp4'")
            if not fragment_layout:
                raise ValueError("mxfp4_mid needs the fragment layout (fragment_layout=True)")
        self.cfg = cfg
        self.device = torch.device(device)
        if tp_rank is None:
            tp_rank = 0
            if tp_size > 1:
                import torch.distributed as dist

                tp_rank = dist.get_rank(tp_group) if dist.is_initialized() else 0
        self.tp_group, self.tp_size, self.tp_rank = tp_group, tp_size, tp_rank
        V = cfg.vocab_size
        # (the merged candidate set, tp x 64 per 8192-token chunk of a slice, must fit the merge
        # kernel's 1024 entries: true for Llama-3's 128256 tokens at tp 2 / 4 / 8)
        self.vocab_parallel = (bool(vocab_parallel) and tp_size > 1 and V % (32 * tp_size) == 0
                               and tp_size * -(-(V // tp_size) // 8192) * 64 <= 1024)
        self.vocab_local = V // tp_size if self.vocab_parallel else V
        self.vocab_start = tp_rank * self.vocab_local if self.vocab_parallel else 0
        self.hq = cfg.heads // tp_size
        self.hkv = cfg.kv_heads // tp_size
        self.interleaved_mlp = interleaved_mlp  # gate_up rows in 8-row [gate | up] groups (EPI_SWIGLU8)
        # One copy of every projection, in the fragment layout both GEMM families read (VERDICT r2
        # "stop paying HBM twice": the decode-only shuffled copies were +15 GB for Llama-3-8B and
        # disabled the streaming decode for 70B at TP 1).  The LM head too; a tied embedding table
        # keeps its row-major copy for the gather.
        # (``fragment_layout=False``: row-major weights on the GPU too, every projection on the
        # 128x128 / phased 256x256 GEMMs -- the comparison path of tests/test_models_gpu.py)
        self.frag = fragment_layout and self.device.type == "cuda" and self._fragment_ok(weights)
        if self.fp8_weights_only and self.device.type == "cuda":
            if not self.frag:
                raise ValueError("fp8_weights_only: the weights do not take the fragment layout")
            for n in ("qkv_w", "o_w", "gate_up_w", "down_w"):
                N, K = weights[f"l0.{n}"].shape
                if N % 256 or K % 128:
                    raise ValueError(f"fp8_weights_only: {n} [{N}, {K}] needs N % 256 == 0 and K % 128 == 0 "
                                     "(the FP8 arm of gemm256 is its only MFMA kernel)")
        if self.mxfp4_weights_only and self.device.type == "cuda":
            if not self.frag:
                raise ValueError("mxfp4_weights_only: the weights do not take the fragment layout")
            for i in range(cfg.layers):
                for n in ("qkv_w", "o_w", "gate_up_w", "down_w"):
                    N, K = weights[f"l{i}.{n}"].shape
                    if K % 128:
                        raise ValueError(f"mxfp4_weights_only: l{i}.{n} [{N}, {K}] needs K % 128 == 0 (it would keep "
                                         "no MXFP4 codes, only dequantised values)")
        take = weights.pop if consume else weights.__getitem__

        self.proj_group = {}

        def fmt(name, t):
            """The decoder's one copy of projection ``name``: the fragment layout, grouped per
            ``PROJ_GROUPS`` where the shape allows (layer 0 decides for every layer)."""
            fp8 = self.weight_dtype == "fp8"
            if self.weight_dtype == "mxfp4":
                codes, scales = ops.weight_quantize_mxfp4(t)
                if not (self.frag and t.shape[1] % 128 == 0):
                    t = ops.weight_dequantize_mxfp4(codes, scales).to(t.dtype)
                    codes = None  # (no MXFP4 fragment layout: the dequantised values alone)
            if fp8:
                data, exps = ops.weight_quantize_fp8(t)
            if not self.frag:
                return ops.weight_dequantize_fp8(data, exps).to(t.dtype) if fp8 else t
            if name not in self.proj_group:
                g = self.PROJ_GROUPS.get(name, 1)
                self.proj_group[name] = g if (t.shape[0] % (16 * g) == 0 and t.numel() * 2 < (1 << 31)) else 1
            if fp8:
                return Fp8Proj.from_rows(data, exps, self.proj_group[name], bf16_copy=not self.fp8_weights_only)
            if self.weight_dtype == "mxfp4" and codes is not None:
                only = self.mxfp4_weights_only and self.device.type == "cuda"
                return Mxfp4Proj.from_rows(codes, scales, self.proj_group[name], bf16_copy=not only)
            return ops.shuffle_weights(t, self.proj_group[name])

        def load(i, name, norm=None):
            """Projection ``name`` of layer i, built and its bf16 source released before the next one
            is taken (the peak during load holds one projection's source, never a layer's)."""
            t = take(f"l{i}.{name}_w").to(self.device)
            if norm is not None:
                t = self._fold(t, norm)
            return fmt(name, t)

        self.embed = take("embed").to(self.device)
        self.final_norm = take("final_norm").to(self.device)
        head = take("lm_head").to(self.device) if "lm_head" in weights else self.embed
        if self.vocab_parallel:
            head = head[self.vocab_start:self.vocab_start + self.vocab_local]
            pad = (-self.vocab_local) % self.VOCAB_PAD if self.frag else 0
            if pad:
                head = torch.cat([head, head.new_zeros((pad, head.shape[1]))])
            head = head.contiguous()
        self.lm_head = ops.shuffle_weights(head) if self.frag else head
        del head
        # ``small_norm_fused`` (opt-in, measured slower: profiles/decode_small_r5.md): the attention /
        # MLP RMSNorm gains move into the columns of the projection each norm feeds
        # (rmsnorm(x) g W^T = rmsnorm(x) (W diag g)^T) and the norms run with unit gains, so small
        # decode batches can normalise inside the consumer GEMM (``_layer_small``).  The fold is one
        # more bf16 rounding of W diag(g), so the default model keeps the reference norm -> GEMM
        # order and does not fold.
        if small_norm_fused is not None:
            self.small_norm_fused = bool(small_norm_fused)
        self.fold_norms = self.frag and self.small_norm_fused
        self.layers = []
        for i in range(cfg.layers):
            an = take(f"l{i}.attn_norm").to(self.device)
            mn = take(f"l{i}.mlp_norm").to(self.device)
            fold = self.fold_norms
            qkv_w, gu_w = load(i, "qkv", an if fold else None), load(i, "gate_up", mn if fold else None)
            if fold:
                an, mn = torch.ones_like(an), torch.ones_like(mn)
            self.layers.append(DecoderLayer(an, qkv_w, load(i, "o"), mn, gu_w, load(i, "down")))
        if self.frag and consume:
            torch.cuda.empty_cache()
        # ``mxfp4_weights_only``: the bf16 image scratch of ``_bf16_w``, one per stream, keyed by the
        # stream's handle; the constructing stream's exists before the engine sizes the KV pool
        self._mxfp4_scratch = {}
        self._mxfp4_scratch_elems = 0
        if self.mxfp4_weights_only and self.device.type == "cuda":
            self._mxfp4_scratch_elems = max(w.shape[0] * w.shape[1] for L in self.layers
                                            for w in (L.qkv_w, L.o_w, L.gate_up_w, L.down_w))
            with torch.cuda.device(self.device):
                self._scratch_for_stream()

        self.custom_ar = None  # parallel.custom_allreduce.CustomAllReduce (set by the engine)
        # TP all-reduces issued from Python: one-shot IPC vs the process group (RCCL / gloo); a call
        # captured into a decode graph counts once, at capture, not per replay
        self.ar_counts = {"ipc": 0, "ipc_fused_norm": 0, "group": 0}
        inv = ref.llama3_inv_freq(cfg.head_dim, cfg.rope_theta, cfg.rope_scaling)
        self.cos_sin = ref.rope_cos_sin(inv, cfg.max_position).to(self.device)

    @staticmethod
    def _fold(w: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
        """W diag(g) (unit gains, e.g. random init: W itself)."""
        if bool(torch.all(g == 1)):
            return w
        return (w.float() * g.float()[None, :]).to(w.dtype)

    def full_logits(self, local: torch.Tensor) -> torch.Tensor:
        """All-gather the vocab-parallel slices of every TP rank -> [n, V] (the CPU sampling path
        and tests; the GPU path gathers candidates instead)."""
        if not self.vocab_parallel:
            return local
        import torch.distributed as dist

        src = local[:, :self.vocab_local].contiguous()
        staged = src.is_cuda and dist.get_backend(self.tp_group) != "nccl"  # gloo rehearsals on one GPU
        if staged:
            src = src.cpu()
        parts = [torch.empty_like(src) for _ in range(self.tp_size)]
        dist.all_gather(parts, src, group=self.tp_group)
        return torch.cat(parts, 1).to(local.device)

    def projection_bytes(self) -> int:
        """Bytes of the qkv / o / gate_up / down weights resident, every copy, counted from the tensors."""
        total = 0
        for L in self.layers:
            for w in (L.qkv_w, L.o_w, L.gate_up_w, L.down_w):
                total += w.nbytes() if isinstance(w, (Fp8Proj, Mxfp4Proj)) else w.numel() * w.element_size()
        return total

    def set_proj_group(self, name: str, group: int) -> None:
        """Re-lay every layer's copy of projection ``name`` (qkv / o / gate_up / down) as
        ``shuffle_weights(w, group)``, in place (captured graphs keep their pointers but bake the group
        in: re-capture after a change).  A/B harness."""
        old = self.proj_group.get(name, 1)
        if not self.frag or group == old:
            return
        for L in self.layers:
            w = getattr(L, name + "_w")
            if w.shape[0] % (16 * group):
                raise ValueError(f"{name}: {w.shape[0]} rows are not whole groups of {group}")
            if isinstance(w, (Fp8Proj, Mxfp4Proj)):
                w.regroup(group)
            else:
                w.copy_(ops.shuffle_weights(ops.unshuffle_weights(w, old), group))
        self.proj_group[name] = group

    def _fragment_ok(self, weights: dict) -> bool:
        keys = ["lm_head" if "lm_head" in weights else "embed"] + [
            f"l{i}.{n}" for i in range(self.cfg.layers) for n in ("qkv_w", "o_w", "gate_up_w", "down_w")]
        return self.interleaved_mlp and all(weights[k].shape[0] % 16 == 0 and weights[k].shape[1] % 64 == 0
                                            for k in keys)

    @property
    def dtype(self):
        return self.embed.dtype

    def _all_reduce(self, x):
        """TP partial sums: the one-shot IPC all-reduce for decode-sized messages when the engine
        attached one (``custom_ar``), RCCL otherwise (prefill, CPU/gloo)."""
        if self.tp_size > 1:
            ar = self.custom_ar
            if ar is not None and ar.eligible(x):
                self.ar_counts["ipc"] += 1
                return ar.all_reduce(x)
            import torch.distributed as dist

            self.ar_counts["group"] += 1
            dist.all_reduce(x, group=self.tp_group)
        return x

    # stream_gemm.hip configurations (shuffled weights): BN 128 rows per workgroup at M <= 64 (13)
    # and M <= 128 (10).  Whole-chip tilings at M 65..128: gate_up's 28672 rows / 112 make exactly
    # 256 workgroups where BN 128 left 32 of the 256 CUs idle (cfg 20: 54.9 -> 51.5 us cold); the LM
    # head uses 192-row tiles (cfg 28: 2/3 of the X staging per weight byte, 228.7 -> 221.3 us).
    # qkv at 96 rows x 4 K-slices (cfg 21) measured slower than BN 128 x 4 (17.1 vs 15.8 us).
    # Decode batches of 129..256 rows: 64-row tiles, 2 k-groups x 4 row groups (cfg 27; M = 256:
    # qkv 27.4 / o 18.6 / gate_up 98.7 / down 49.2 us against 32.4 / 25.8 / 104 / 55 for two
    # M = 128 passes, profiles/decode_round2.md).
    STREAM_CFG_M16, STREAM_CFG_M32, STREAM_CFG_M64, STREAM_CFG_M128, STREAM_CFG_M256 = 30, 31, 13, 10, 27
    STREAM_WIDE = {"gate_up": 20, "lm_head": 28}
    STREAM_MAX_M = ops.STREAM_MAX_M
    PREFILL_STREAM_MAX_M = 128  # prefill steps of at most this many tokens stream too (0: off)

    def _stream_cfg(self, name: str, M: int, N: int) -> int:
        nat = ops.native()
        if M > 128 and name == "gate_up":
            # decode batches of 129..256: gate_up (+SwiGLU8) on the mid-M GEMM, 67-72 us against 90-96
            # on the M <= 256 streaming tiles (profiles/small_prefill_r6.md); qkv / o / down stream
            return -1
        if M > 128:
            cfg = self.STREAM_CFG_M256
        elif M <= 16 and N % nat.stream_gemm_bn(self.STREAM_CFG_M16) == 0:
            cfg = self.STREAM_CFG_M16
        elif M <= 32 and N % nat.stream_gemm_bn(self.STREAM_CFG_M32) == 0:
            cfg = self.STREAM_CFG_M32
        elif M <= 64:
            cfg = self.STREAM_CFG_M64
        else:
            cfg = self.STREAM_WIDE.get(name)
            if cfg is None or N % nat.stream_gemm_bn(cfg):
                cfg = self.STREAM_CFG_M128
        return cfg if N % nat.stream_gemm_bn(cfg) == 0 else -1

    @staticmethod
    def _stream_splits(N: int, K: int, bn: int = 128) -> int:
        """K-slices for stream_gemm: the fewest that give >= 192 workgroups of ``bn`` weight rows."""
        tiles, best = N // bn, 1
        for s in (1, 2, 4, 8, 16):
            if K % (128 * s):
                break
            best = s
            if tiles * s >= 192:
                break
        return best

    def _stream_choice(self, name: str, M: int, N: int, K: int) -> tuple[int, int]:
        """(stream_gemm cfg, K-slices) of a decode projection; cfg -1 = not streamable.  (The tuning
        harness benchmarks/decode_ab.py overrides this in a subclass.)"""
        cfg = self._stream_cfg(name, M, N)
        if cfg < 0 or K % 128:
            return -1, 1
        return cfg, self._stream_splits(N, K, ops.native().stream_gemm_bn(cfg))

    # Projections held in the grouped fragment layout (shuffle_weights(w, G): the G row blocks of
    # each 16 G-row group adjacent per 32-deep k chunk), so the decode GEMM's waves (one block each)
    # stream neighbouring bytes; every GEMM reading a copy takes its group (``proj_group``).  gate_up
    # at 8: batch-128 decode step 7.31 -> 7.23 ms (profiles/decode_stream_layout_r6.md)
    PROJ_GROUPS = {"gate_up": 8}

    # Split-K slabs of the decode projections as bf16 (the partial sums rounded once, as the TP path
    # hands them to its all-reduce) instead of fp32: half the bytes the producer writes and the
    # RMSNorm / RoPE consumers read; batch-128 decode step 7.503 -> 7.351 ms (benchmarks/decode_ab.py
    # slab32,slab16; profiles/decode_slab_r6.md).  TP keeps fp32: its fused all-reduce + norm sums
    # fp32 slabs.
    slab_bf16 = True

    # FP8 KV cache: the qkv projection keeps fp32 split-K slabs.  A bf16 slab rounds every partial sum, which
    # leaves ~40 % of the K / V values one bf16 step away from the MFMA GEMM's; the quantiser turns such a step
    # into a whole FP8 step (16 bf16 steps) wherever it crosses a rounding boundary, so a streamed step and a
    # GEMM step (a short prefill against a mixed step, a decode step against a prefill) would cache visibly
    # different bytes for the same token: ~1.8k of 31k K bytes against 0-1 with fp32 slabs (profiles/kv_fp8.md).
    fp8_qkv_slab_f32 = True

    def _proj(self, x, w, dec: bool, allow_slabs: bool = True, name: str = "", epilogue=ops.EPI_NONE,
              slab_f32: bool = False):
        """One projection.  Decode-sized batches (``dec``) stream the fragment-layout weights
        through stream_gemm, as fp32 split-K slabs when a consumer sums them (RMSNorm, the decode
        attention's RoPE prologue) and ``allow_slabs``; everything else runs the MFMA GEMM on the
        same copy (gemm256 for large token counts, the 128x128 kernel below that)."""
        if not x.is_cuda:
            if epilogue == ops.EPI_SWIGLU8 or (epilogue == ops.EPI_NONE and name == "gate_up"):
                y = ops.linear(x, w)
                return ops.silu_mul(y, group=8 if self.interleaved_mlp else 0)
            return ops.linear(x, w)
        grp = self.proj_group.get(name, 1)
        if dec and self.frag:
            cfg, s = self._stream_choice(name, x.shape[0], w.shape[0], w.shape[1])
            if cfg >= 0 and self.fp8_weights_only and not ops.native().stream_gemm_fp8_ok(cfg):
                cfg = -1  # no FP8 instantiation of this tiling and no bf16 copy to stream: gemm256's FP8 arm
            if cfg >= 0:
                sw, e = self._stream_w(w, name, cfg)
                if epilogue != ops.EPI_NONE:
                    return ops.stream_gemm(x, sw, epilogue=epilogue, nt=True, cfg=cfg, w_group=grp, **e)
                sd = torch.bfloat16 if (self.slab_bf16 and self.tp_size == 1 and not slab_f32) else torch.float32
                out = ops.stream_gemm(x, sw, splits=s, cfg=cfg, nt=True, slab_dtype=sd, w_group=grp, **e)
                return ops.slab_reduce(out) if (s > 1 and not allow_slabs) else out
        return self._mfma(x, w, name=name, epilogue=epilogue, shuffled=self.frag, b_group=grp)

    # ``mxfp4_mid``: projections that keep the bf16 path although their call would take gemm_mid's
    # MXFP4 arm: the opt-out for projections that measure slower (profiles/gemm_mid_mxfp4.md)
    MXFP4_MID_OFF: frozenset = frozenset()

    def _mfma(self, x, w, name: str = "", **kw):
        """``ops.gemm_bt`` on a projection: its bf16 copy, or (``fp8_weights_only``: there is none) the
        FP8 bytes on the FP8 arm of gemm256, which takes every M.  ``mxfp4_mid``: the codes of an
        ``Mxfp4Proj`` on gemm_mid's MXFP4 arm wherever the bf16 call would take gemm_mid."""
        if isinstance(w, Fp8Proj) and w.w is None:
            return ops.gemm_bt(x, w.data, w_exps=w.exps, **kw)
        if (self.mxfp4_mid and isinstance(w, Mxfp4Proj) and x.is_cuda and name not in self.MXFP4_MID_OFF
                and kw.get("rows") is None and kw.get("as_m") is None):
            (M, K), N, lda = x.shape, w.shape[0], x.stride(0)
            if ops.kernels.use_gemm_mid(M, N, K, lda) and ops.kernels.gemm_mid_mxfp4_ok(M, N, K, lda):
                return ops.gemm_bt(x, w.data, w_scales=w.scales, **kw)
        return ops.gemm_bt(x, self._bf16_w(w), **kw)

    def mxfp4_scratch_bytes(self) -> int:
        """Bytes of ONE bf16 image scratch of ``mxfp4_weights_only`` (0 without it): the largest
        projection.  Every stream that runs the model holds one (``_scratch_for_stream``)."""
        return 2 * self._mxfp4_scratch_elems

    def _scratch_for_stream(self) -> torch.Tensor:
        """The current stream's image scratch.  One per stream: two engines sharing this model on two
        streams each dequantise into their own, and a captured graph keeps the pointer of the stream
        it was captured on, so a scratch is never freed or moved.  A stream's first use allocates,
        which a graph capture cannot do: warm the stream up before capturing on it."""
        key = torch.cuda.current_stream(self.device).cuda_stream
        buf = self._mxfp4_scratch.get(key)
        if buf is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("mxfp4_weights_only: this stream has no weight scratch yet and a graph capture "
                                   "cannot allocate one (run the step once on the stream before capturing)")
            buf = self._mxfp4_scratch[key] = torch.empty(self._mxfp4_scratch_elems, dtype=torch.bfloat16,
                                                         device=self.device)
        return buf

    def _bf16_w(self, w):
        """The bf16 fragment tensor of a projection: the tensor itself, the resident copy of an
        ``Fp8Proj`` / ``Mxfp4Proj``, or (``mxfp4_weights_only``: there is none) the image
        ``ops.weight_dequant_mxfp4`` writes into the current stream's scratch, as an [N, K] view.  The
        view is valid until the next call on this stream: stream order puts the next dequantiser behind
        the GEMM that reads it, so a caller takes it right before its GEMM and holds one at a time."""
        if isinstance(w, Mxfp4Proj) and w.w is None:
            return ops.weight_dequant_mxfp4(w.data, w.scales, self._scratch_for_stream(), w.group)
        return _bf16_copy(w)

    # FP8 weights: (projection, stream_gemm cfg) pairs that stream the bf16 copy although the cfg has
    # an FP8 instantiation: the per-shape opt-out for ranges that measure slower (profiles/weight_fp8.md)
    FP8_STREAM_OFF: frozenset = frozenset()
    fp8_stream = True  # off: every stream_gemm call reads the bf16 copies (benchmarks/decode_ab.py A/B)

    # MXFP4 weights: the same opt-out (profiles/weight_mxfp4.md)
    MXFP4_STREAM_OFF: frozenset = frozenset()
    mxfp4_stream = True  # off: every stream_gemm call reads the bf16 copies (benchmarks/decode_ab.py A/B)

    def _stream_w(self, w, name: str, cfg: int):
        """(weights, stream_gemm keyword arguments) for a stream_gemm call at ``cfg``: the FP8 copy of
        an ``Fp8Proj`` with ``w_exps`` (the MXFP4 copy of an ``Mxfp4Proj`` with ``w_scales``) where
        the kernel has such an arm for ``cfg``, else the bf16 copy (same values) and nothing."""
        if isinstance(w, Mxfp4Proj):
            if (self.mxfp4_stream and ops.native().stream_gemm_mxfp4_ok(cfg)
                    and (name, cfg) not in self.MXFP4_STREAM_OFF):
                return w.data, {"w_scales": w.scales}
            return self._bf16_w(w), {}  # (``mxfp4_weights_only``: the scratch image; one at a time)
        if not isinstance(w, Fp8Proj):
            return w, {}
        if self.fp8_stream and ops.native().stream_gemm_fp8_ok(cfg) and (name, cfg) not in self.FP8_STREAM_OFF:
            return w.data, {"w_exps": w.exps}
        if w.w is None:
            raise RuntimeError(f"fp8_weights_only: stream_gemm cfg {cfg} ({name}) has no FP8 arm (or FP8 streaming "
                               "was switched off) and there is no bf16 copy to stream")
        return w.w, {}

    # Pure prefill steps whose caller reads only ``out_rows`` (the last token of each finished
    # prompt, ~30 rows of 32k): everything after the LAST layer's attention is row-wise -- o + residual,
    # MLP norm, gate_up + SwiGLU, down + residual, final norm -- so it runs on those rows alone (one
    # layer's o / gate_up / down GEMMs and two norm passes less per step).  The rows go through the
    # kernels the full step would have taken (gemm256 ``rows`` / ``as_m``: an element's arithmetic
    # depends neither on M nor on its tile row), so the result is bit-identical; steps whose full
    # call takes another kernel (mid-M, streamed, TP, CPU, mixed) run whole and select afterwards.
    # Switch for the A/B and the equality tests.
    prune_last_tail = True

    def _tail_prunable(self, T: int, meta: AttnMeta, x: torch.Tensor, sk: bool) -> bool:
        if not (self.prune_last_tail and x.is_cuda and not sk and not meta.decode and not meta.n_decode
                and self.tp_size == 1 and self.frag):
            return False
        if self.fp8_weights_only:
            return True  # every call that is not streamed is gemm256 (its FP8 arm), at any T
        if T < ops.kernels.GEMM256_MIN_M:
            return False
        L = self.layers[-1]
        for N, K in (L.o_w.shape, L.gate_up_w.shape, L.down_w.shape):  # (contiguous activations: lda = K)
            if ops.kernels.use_gemm_mid(T, N, K, K) or not ops.kernels.use_gemm256(T, N, K, K, K):
                return False
        return True

    def forward(self, ids: torch.Tensor, meta: AttnMeta, kv: KVCache,
                out_rows: torch.Tensor | None = None) -> torch.Tensor:
        """ids int32 [T] -> final hidden states [T, H] (after the last RMSNorm); with ``out_rows``
        (int32 / int64 [n] row ids, on the device of ``ids``) only those rows, [n, H]."""
        cfg = self.cfg
        D = cfg.head_dim
        T = ids.numel()
        x = ops.embed_gather(ids, self.embed)
        # decode-sized batches stream the weights through the split-K MFMA kernel; its fp32 slabs
        # are summed by the consumers (RoPE/KV write, RMSNorm) instead of a separate reduction.  So
        # do short prefill steps (an interactive prompt, the tail of a batch): at T <= 128 the MFMA
        # tiles read every weight for a handful of rows (qkv / o / gate_up / down 54 / 54 / 65 /
        # 183 us against 16-21 / 15-19 / 42-49 / 27-32 streamed, profiles/small_prefill_r6.md)
        small_pf = (not meta.decode and not meta.n_decode and T <= self.PREFILL_STREAM_MAX_M and self.frag
                    and self.tp_size == 1)
        sk = (meta.decode and T <= self.STREAM_MAX_M or small_pf) and x.is_cuda
        if sk and meta.decode and T <= self.SMALL_FUSED_MAX_M and self.small_norm_fused and self.fold_norms and self.tp_size == 1:
            h = x  # the residual stream itself: no RMSNorm launches (``_layer_small``)
            for li, L in enumerate(self.layers):
                h = self._layer_small(li, L, h, meta, kv)
            h = ops.rmsnorm(h, self.final_norm, self.cfg.eps)[0]
            return h if out_rows is None else h.index_select(0, out_rows)
        residual = None
        prune = out_rows is not None and self._tail_prunable(T, meta, x, sk)
        for li, L in enumerate(self.layers):
            rows = out_rows if prune and li == len(self.layers) - 1 else None
            x, residual = self._layer(li, L, x, residual, meta, kv, sk, rows)
        if prune and out_rows.numel() == 0:  # no prompt ends in this chunk: only the K / V writes were due
            return residual
        h = self._final_norm(x, residual)
        return h if out_rows is None or prune else h.index_select(0, out_rows)

    # Small decode batches (the interactive case): the residual stream h is the
    # only activation between layers.  The o / down projections stream their weights without split-K
    # (16-row tiles fill the chip at M <= 16) and add the residual in their epilogue, so h leaves them
    # complete; the qkv / gate_up projections read h as X and apply the RMSNorm as a per-row scale in
    # their epilogue (gains folded into their weights).  The two slab-summing RMSNorm launches per
    # layer are gone.  Switch: ``small_norm_fused`` (benchmarks/decode_ab.py A/B).  Measured SLOWER
    # (B=1 3.88 vs 3.65 ms/token, B=8 4.25 vs 3.81 ms/step, profiles/decode_small_r5.md): the whole-K
    # o / down tiles launch only N/16 workgroups, one per CU, and lose the split-K latency hiding
    # that the two norm launches cost less than -- so it is off by default.
    SMALL_FUSED_MAX_M = 16
    STREAM_CFG_RES16 = 32  # stream_gemm.hip cfg 32: BN 16, whole K
    small_norm_fused = False

    def _layer_small(self, li: int, L: DecoderLayer, h, meta: AttnMeta, kv: KVCache):
        cfg, D = self.cfg, self.cfg.head_dim
        T = h.shape[0]
        c, s = self._stream_choice("qkv", T, L.qkv_w.shape[0], L.qkv_w.shape[1])
        pg = self.proj_group
        R = self.STREAM_CFG_RES16
        # (each ``_stream_w`` right before its GEMM: under ``mxfp4_weights_only`` two of them may be
        # views of the one scratch)
        qw, qe = self._stream_w(L.qkv_w, "qkv", c)
        qkv = ops.stream_gemm(h, qw, splits=s, cfg=c, nt=True, norm_eps=cfg.eps, w_group=pg.get("qkv", 1), **qe)
        q = kv.write(li, qkv, meta.positions, self.cos_sin, meta.slots, self.hq, self.hkv, D)
        a = kv.decode_attention(li, q, meta.block_tables, meta.ctx_lens, meta.part_size, meta.workspace,
                                order=meta.order)
        ow, oe = self._stream_w(L.o_w, "o", R)
        h1 = ops.stream_gemm(a.view(T, self.hq * D), ow, residual=h, cfg=R, nt=True, w_group=pg.get("o", 1), **oe)
        gc, _ = self._stream_choice("gate_up", T, L.gate_up_w.shape[0], L.gate_up_w.shape[1])
        gw, ge = self._stream_w(L.gate_up_w, "gate_up", gc)
        act = ops.stream_gemm(h1, gw, epilogue=ops.EPI_SWIGLU8, cfg=gc, nt=True, norm_eps=cfg.eps,
                              w_group=pg.get("gate_up", 1), **ge)
        dw, de = self._stream_w(L.down_w, "down", R)
        return ops.stream_gemm(act, dw, residual=h1, cfg=R, nt=True, w_group=pg.get("down", 1), **de)

    # Small decode batches: the paged attention is a chain of dependent memory round trips on a few
    # dozen CUs (~15 us per layer at batch 1 while HBM idles).  ``l3_warm_mb`` > 0 appends
    # ``l3_warm_blocks`` workgroups to that launch which read the first MB of the layer's o and
    # gate_up weights into the Infinity Cache, so those projections stream part of their weights
    # on-die.  A/B: benchmarks/decode_ab.py arms warm*.
    L3_WARM_MAX_M = 16
    l3_warm_mb = 0
    l3_warm_blocks = 192

    def _warm(self, L: DecoderLayer, T: int, ref):
        if not self.l3_warm_mb or T > self.L3_WARM_MAX_M or not ref.is_cuda:
            return None
        o_w, gu_w = L.o_w, L.gate_up_w
        if isinstance(o_w, (Fp8Proj, Mxfp4Proj)):  # the bytes the decode GEMM streams
            o_w, gu_w = o_w.data, gu_w.data
        budget = int(self.l3_warm_mb * 2 ** 20) & ~15
        ob = o_w.numel() * o_w.element_size()
        ranges = [(o_w, min(ob, budget))]
        if budget > ob:
            ranges.append((gu_w, min(budget - ob, gu_w.numel() * gu_w.element_size()) & ~15))
        return ranges, self.l3_warm_blocks

    def _final_norm(self, x, residual):
        if x is None:  # the residual stream holds the last layer's output
            return ops.rmsnorm(residual, self.final_norm, self.cfg.eps)[0]
        return self._norm(x, self.final_norm, residual)[0]

    def _norm(self, x, w, residual):
        """RMSNorm(x + residual) -> (normed, new residual); x may be a ``_Partial`` whose TP
        all-reduce runs inside the same launch (``CustomAllReduce.all_reduce_rmsnorm``)."""
        if isinstance(x, _Partial):
            self.ar_counts["ipc_fused_norm"] += 1
            return self.custom_ar.all_reduce_rmsnorm(x.t, residual, w, self.cfg.eps)
        return ops.rmsnorm(x, w, self.cfg.eps, residual=residual)

    # TP decode all-reduce sites fused with their consumer RMSNorm; off: the
    # separate slab_reduce / all-reduce / rmsnorm launches (A/B and the bit-exactness test)
    tp_fused_norm = True

    def _tp_partial(self, x, cols: int):
        """A row-parallel projection's output under TP: a ``_Partial`` when the fused all-reduce +
        norm can take it, else the all-reduced bf16 tensor."""
        ar = self.custom_ar
        if self.tp_fused_norm and ar is not None and x.is_cuda and ar.norm_eligible(x, cols):
            return _Partial(x)
        if x.dtype == torch.float32 and x.dim() == 3:
            x = ops.slab_reduce(x)
        return self._all_reduce(x)

    def _layer(self, li: int, L: DecoderLayer, x, residual, meta: AttnMeta, kv: KVCache, sk: bool, rows=None):
        """One decoder layer: (layer input, residual stream) -> (next layer input, residual stream).
        ``rows`` (``forward``'s ``out_rows``, last layer of a prunable step): the part after the
        attention runs on these rows only and the residual stream returned is compact [n, H]."""
        cfg, D, T = self.cfg, self.cfg.head_dim, meta.positions.numel()  # x may be [S, T, H] split-K slabs
        slabs_ok = self.tp_size == 1  # under TP the partial sums go through the all-reduce as bf16
        # prefill (TP 1): the o / down GEMMs add the residual in their epilogue (gemm256 RES, rounded
        # like the separate bf16 add), so the RMSNorms read and write one tensor instead of two each;
        # x is None then: the residual stream already holds the layer input
        fuse = not sk and self.tp_size == 1 and (x if x is not None else residual).is_cuda
        if x is None:
            h, _ = ops.rmsnorm(residual, L.attn_norm, cfg.eps)
        elif residual is None:
            h, _ = ops.rmsnorm(x, L.attn_norm, cfg.eps)
            residual = x
        else:
            h, residual = self._norm(x, L.attn_norm, residual)
        qkv = self._proj(h, L.qkv_w, sk, name="qkv", slab_f32=kv.fp8 and self.fp8_qkv_slab_f32)
        if (not meta.decode and not meta.n_decode and qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 2
                and ops.kernels.flash_rope_ok(D, kv.block_size)):
            # prefill: the RoPE/KV-write kernel writes only K / V; the attention rotates Q on load
            # straight from the projection (a [T, Hq*D] write and read less per layer)
            kv.write(li, qkv, meta.positions, self.cos_sin, meta.slots, self.hq, self.hkv, D, write_q=False)
            q = qkv[:, :self.hq * D].view(T, self.hq, D)
            a = kv.prefill_attention(li, q, meta, rope=(meta.positions, self.cos_sin))
            if rows is not None:
                return self._layer_tail_rows(L, a, residual, rows, T, D)
            return self._layer_tail(L, a, residual, sk, fuse, slabs_ok, T, D)
        q = kv.write(li, qkv, meta.positions, self.cos_sin, meta.slots, self.hq, self.hkv, D)
        if meta.decode:
            a = kv.decode_attention(li, q, meta.block_tables, meta.ctx_lens, meta.part_size, meta.workspace,
                                    order=meta.order, warm=self._warm(L, T, q))
        elif meta.n_decode:
            a = self._mixed_attention(q, kv, li, meta)
        else:
            a = kv.prefill_attention(li, q, meta)
        if rows is not None:
            return self._layer_tail_rows(L, a, residual, rows, T, D)
        return self._layer_tail(L, a, residual, sk, fuse, slabs_ok, T, D)

    def _layer_tail_rows(self, L, a, residual, rows, T, D):
        """``_layer_tail`` (its ``fuse`` form) for the rows ``rows`` of a T-token step whose o / gate_up
        / down run on gemm256 (``_tail_prunable``): the o projection gathers its rows of ``a`` and of
        the residual stream inside the kernel, the rest runs on the compact rows as a T-row call would."""
        n = rows.numel()
        if n == 0:
            return None, residual.new_empty((0, residual.shape[1]))
        if rows.dtype != torch.int32:
            rows = rows.to(torch.int32)
        pg = self.proj_group
        res = self._mfma(a.view(T, self.hq * D), L.o_w, name="o", residual=residual, shuffled=True,
                         b_group=pg.get("o", 1), rows=rows)
        h, _ = ops.rmsnorm(res, L.mlp_norm, self.cfg.eps)
        act = self._mfma(h, L.gate_up_w, name="gate_up", epilogue=ops.EPI_SWIGLU8, shuffled=True,
                         b_group=pg.get("gate_up", 1), as_m=T)
        return None, self._mfma(act, L.down_w, name="down", residual=res, shuffled=True, b_group=pg.get("down", 1),
                                as_m=T)

    def _layer_tail(self, L, a, residual, sk, fuse, slabs_ok, T, D):
        """o projection, MLP norm, gate_up (+SwiGLU), down: -> (next layer input, residual stream)."""
        cfg = self.cfg
        if fuse:
            residual = self._mfma(a.view(T, self.hq * D), L.o_w, name="o", residual=residual, shuffled=self.frag,
                                  b_group=self.proj_group.get("o", 1))
            h, _ = ops.rmsnorm(residual, L.mlp_norm, cfg.eps)
        elif sk and self.tp_size > 1:
            # TP decode: the o partial (split-K slabs) meets its all-reduce inside the MLP norm's launch
            o = self._tp_partial(self._proj(a.view(T, self.hq * D), L.o_w, sk, True, name="o"), cfg.hidden)
            h, residual = self._norm(o, L.mlp_norm, residual)
        else:
            o = self._all_reduce(self._proj(a.view(T, self.hq * D), L.o_w, sk, slabs_ok, name="o"))
            h, residual = ops.rmsnorm(o, L.mlp_norm, cfg.eps, residual=residual)
        # SwiGLU in the GEMM epilogue (8-row [gate | up] groups) on the GPU
        epi = ops.EPI_SWIGLU8 if (self.interleaved_mlp and h.is_cuda) else ops.EPI_NONE
        act = self._proj(h, L.gate_up_w, sk, name="gate_up", epilogue=epi)
        if h.is_cuda and epi == ops.EPI_NONE:
            act = ops.silu_mul(act)
        if fuse:
            return None, self._mfma(act, L.down_w, name="down", residual=residual, shuffled=self.frag,
                                    b_group=self.proj_group.get("down", 1))
        if sk and self.tp_size > 1:  # reduced inside the next layer's (or the final) norm launch
            return self._tp_partial(self._proj(act, L.down_w, sk, True, name="down"), cfg.hidden), residual
        x = self._all_reduce(self._proj(act, L.down_w, sk, slabs_ok, name="down"))
        return x, residual

    @staticmethod
    def _mixed_attention(q, kv: KVCache, li: int, meta: AttnMeta) -> torch.Tensor:
        """Prefill rows through flash attention, decode rows through the split-K paged decode kernel
        (flash's 64-query tiles would be 1/64 full for them and re-read the KV per query head); both
        write disjoint row ranges of one output, so the projections around stay single GEMMs."""
        Tp = q.shape[0] - meta.n_decode
        if not q.is_cuda:
            parts = []
            if Tp:
                parts.append(kv.prefill_attention(li, q[:Tp], meta))
            parts.append(kv.decode_attention(li, q[Tp:], meta.dec_block_tables, meta.dec_ctx_lens, meta.part_size,
                                             meta.workspace))
            return torch.cat(parts)
        a = torch.empty_like(q)
        if Tp:
            kv.prefill_attention(li, q[:Tp], meta, out=a[:Tp])
        kv.decode_attention(li, q[Tp:], meta.dec_block_tables, meta.dec_ctx_lens, meta.part_size, meta.workspace,
                            out=a[Tp:], order=meta.order)
        return a

    def logits(self, h: torch.Tensor) -> torch.Tensor:
        """[n, H] -> [n, V] logits (bf16; the sampler reads bf16 or fp32).  Up to 256 rows (decode
        steps, prefill last tokens) stream the fragment-layout LM head through ``stream_gemm``;
        larger batches run the MFMA GEMM on the same copy.  Vocab-parallel: [n, padded slice] with
        the first ``vocab_local`` columns valid (tokens ``vocab_start`` ...)."""
        if not h.is_cuda:
            return ops.linear(h, self.lm_head)
        return self._proj(h, self.lm_head, h.shape[0] <= self.STREAM_MAX_M, False, name="lm_head")
