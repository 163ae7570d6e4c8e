"""Plain-PyTorch fp32 reference implementations of every native op.

They define the semantics the gfx950 kernels must match (tests compare kernel output against these)
and they are what runs when the engine is driven with CPU tensors (unit tests, the CPU plumbing
config of BASELINE.json).  Inputs/outputs use the same dtypes and layouts as the kernels.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

EPI_NONE, EPI_GELU, EPI_SWIGLU, EPI_SCORES = 0, 1, 2, 3
EPI_SWIGLU8 = 4  # SwiGLU over 8-row [gate | up] groups (decode copies of whole-chip stream_gemm tilings)


def rmsnorm(x, w, eps, residual=None):
    xf = x.float()
    res_out = None
    if residual is not None:
        xf = (xf + residual.float()).to(x.dtype).float()
        res_out = xf.to(x.dtype)
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * inv * w.float()).to(x.dtype), res_out


def layernorm(x, gamma, beta, eps, residual=None):
    xf = x.float()
    if residual is not None:
        xf = xf + residual.float()
    return F.layer_norm(xf, (x.shape[-1],), gamma.float(), beta.float(), eps).to(x.dtype)


def bert_embed(ids, pos_ids, type_ids, word, pos, typ, gamma, beta, eps):
    t = type_ids.long() if type_ids is not None else torch.zeros_like(ids, dtype=torch.long)
    e = word[ids.long()].float() + pos[pos_ids.long()].float() + typ[t].float()
    return F.layer_norm(e, (e.shape[-1],), gamma.float(), beta.float(), eps).to(word.dtype)


def embed_gather(ids, table):
    return table[ids.long()]


def mean_pool(hidden, cu_seqlens, normalize):
    cu = cu_seqlens.tolist()
    outs = []
    for i in range(len(cu) - 1):
        seg = hidden[cu[i]:cu[i + 1]].float()
        m = seg.mean(0) if seg.shape[0] else torch.zeros(hidden.shape[-1], device=hidden.device)
        outs.append(m)
    out = torch.stack(outs) if outs else hidden.new_zeros((0, hidden.shape[-1]), dtype=torch.float32)
    if normalize:
        out = F.normalize(out, dim=-1)
    return out


def gelu(x, bias=None):
    xf = x.float()
    if bias is not None:
        xf = xf + bias.float()
    return F.gelu(xf, approximate="none").to(x.dtype)


def silu_mul(x):
    F_ = x.shape[-1] // 2
    xf = x.float()
    return (F.silu(xf[..., :F_]) * xf[..., F_:]).to(x.dtype)


def rope_kv_write(qkv, positions, cos_sin, k_cache, v_cache, slots, Hq, Hkv, D, block_size):
    """Returns rotated q [T, Hq, D]; rotates k and writes k/v into the paged caches in place."""
    T = qkv.shape[0]
    x = qkv[:, : (Hq + 2 * Hkv) * D].float().view(T, Hq + 2 * Hkv, D)
    cs = cos_sin[positions.long()]  # [T, D/2, 2]
    cos, sin = cs[..., 0].unsqueeze(1), cs[..., 1].unsqueeze(1)
    half = D // 2
    qk = x[:, : Hq + Hkv]
    x1, x2 = qk[..., :half], qk[..., half:]
    rot = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)
    q = rot[:, :Hq].to(qkv.dtype)
    k = rot[:, Hq:].to(qkv.dtype)
    v = x[:, Hq + Hkv:].to(qkv.dtype)
    for t in range(T):
        s = int(slots[t])
        if s < 0:
            continue
        blk, off = divmod(s, block_size)
        k_cache[blk, :, off] = k[t]
        v_cache[blk, :, off] = v[t]
    return q.contiguous()


def rope_q(q, positions, cos_sin):
    """Rotate-half RoPE of q [T, Hq, D] at ``positions`` (what rope_kv_write returns as q)."""
    D = q.shape[-1]
    half = D // 2
    cs = cos_sin[positions.long()]
    cos, sin = cs[..., 0].unsqueeze(1), cs[..., 1].unsqueeze(1)
    x = q.float()
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1).to(q.dtype)


def _attend(q, k, v, scale, causal, q_offset):
    # q [Sq, H, D], k/v [Sk, Hkv, D] -> [Sq, H, D] (fp32 math)
    H, Hkv = q.shape[1], k.shape[1]
    rep = H // Hkv
    kf = k.float().repeat_interleave(rep, dim=1)
    vf = v.float().repeat_interleave(rep, dim=1)
    s = torch.einsum("qhd,khd->hqk", q.float(), kf) * scale
    if causal:
        Sq, Sk = q.shape[0], k.shape[0]
        qpos = torch.arange(Sq, device=q.device)[:, None] + q_offset
        kpos = torch.arange(Sk, device=q.device)[None, :]
        s = s.masked_fill((kpos > qpos)[None], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("hqk,khd->qhd", p, vf)


def flash_attention_packed(q, k, v, cu_q, cu_k, causal, scale):
    """q [Tq, Hq, D], k/v [Tk, Hkv, D] packed by cu_seqlens -> [Tq, Hq, D] (q dtype)."""
    out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    cq, ck = cu_q.tolist(), cu_k.tolist()
    for b in range(len(cq) - 1):
        qs, ks = q[cq[b]:cq[b + 1]], k[ck[b]:ck[b + 1]]
        vs = v[ck[b]:ck[b + 1]]
        off = ks.shape[0] - qs.shape[0]
        out[cq[b]:cq[b + 1]] = _attend(qs, ks, vs, scale, causal, off).to(q.dtype)
    return out


def gather_paged(cache, block_table, n):
    """cache [num_blocks, Hkv, bs, D] -> the first n tokens of a sequence as [n, Hkv, D]."""
    bs = cache.shape[2]
    nb = (n + bs - 1) // bs
    blocks = cache[block_table[:nb].long()]  # [nb, Hkv, bs, D]
    return blocks.permute(0, 2, 1, 3).reshape(nb * bs, cache.shape[1], cache.shape[3])[:n]


def flash_attention_paged(q, k_cache, v_cache, block_tables, cu_q, ctx_lens, causal, scale):
    out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    cq = cu_q.tolist()
    for b in range(len(cq) - 1):
        n = int(ctx_lens[b])
        ks = gather_paged(k_cache, block_tables[b], n)
        vs = gather_paged(v_cache, block_tables[b], n)
        qs = q[cq[b]:cq[b + 1]]
        out[cq[b]:cq[b + 1]] = _attend(qs, ks, vs, scale, causal, n - qs.shape[0]).to(q.dtype)
    return out


def paged_decode(q, k_cache, v_cache, block_tables, ctx_lens, scale):
    """q [B, Hq, D] one token per sequence -> [B, Hq, D]."""
    out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    for b in range(q.shape[0]):
        n = int(ctx_lens[b])
        ks = gather_paged(k_cache, block_tables[b], n)
        vs = gather_paged(v_cache, block_tables[b], n)
        out[b] = _attend(q[b:b + 1], ks, vs, scale, False, 0)[0].to(q.dtype)
    return out


# ----------------------------------------------------------------------------------------------
# FP8 KV cache (opt-in): per (token, kv head) row of D values, OCP e4m3fn data bytes and one E8M0
# exponent byte b (scale 2^(b - 127)), K and V alike.  docs/ARCHITECTURE.md "FP8 KV cache".

KV_FP8_MAX = 448.0


def kv_quantize(x):
    """bf16 (or bf16-exact) rows [..., D] -> (e4m3fn bytes uint8 [..., D], exponent bytes uint8 [...]).

    The scale is the smallest power of two 2^e with amax / 2^e <= 448, found with integer operations
    on the bits of amax (so the GPU writer agrees bit for bit): with amax = 1.M x 2^(E - 127) it is
    e = E - 135, or E - 134 when 1.M > 1.75.  b = clamp(e + 127, 1, 254); a zero row has b = 127 and
    zero bytes.  Data: x / 2^(b - 127) (exact), clamped to +-448, rounded to nearest-even."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    bits = amax.contiguous().view(torch.int32)
    E, M = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    b = (E - 8 + (M > 0x600000).to(torch.int32)).clamp(1, 254)
    b = torch.where(amax == 0, torch.full_like(b, 127), b)
    inv = ((254 - b) << 23).view(torch.float32)  # 2^-(b - 127)
    y = (xf * inv[..., None]).clamp(-KV_FP8_MAX, KV_FP8_MAX)
    data = y.to(torch.float8_e4m3fn).view(torch.uint8)
    data = torch.where((amax == 0)[..., None], torch.zeros_like(data), data)
    return data, b.to(torch.uint8)


def kv_dequantize(data, exps):
    """(bytes [..., D], exponent bytes [...]) -> fp32 [..., D]; every value is bf16-exact."""
    scale = (exps.to(torch.int32) << 23).view(torch.float32)
    return data.view(torch.float8_e4m3fn).float() * scale[..., None]


def weight_quantize_fp8(w):
    """Projection weights [N, K] -> (e4m3fn bytes uint8 [N, K], exponent bytes uint8 [N]): the KV
    cache's row rule (``kv_quantize``) along K, one power-of-two scale per output row.  Load-time,
    in torch.  docs/ARCHITECTURE.md "FP8 weights"."""
    return kv_quantize(w)


def weight_dequantize_fp8(data, exps):
    """(bytes [N, K], exponent bytes [N]) -> bf16 [N, K]; exact (every value is bf16-exact)."""
    return kv_dequantize(data, exps).to(torch.bfloat16)


MXFP4_BLOCK = 32  # k per E8M0 scale byte (OCP MX)
# magnitudes of the e2m1 codes 0..7 (bit 3 of a code is the sign)
MXFP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def weight_quantize_mxfp4(w):
    """Projection weights [N, K] (K % 32 == 0) -> (e2m1 codes uint8 [N, K/2], scale bytes uint8 [N, K/32]):
    OCP MXFP4 along K, one E8M0 byte b (scale 2^(b - 127)) per block of 32 consecutive k of a row.

    The scale is the smallest power of two 2^e with amax / 2^e <= 6 (nothing clips), found with
    integer operations on the bits of the block's amax, as ``kv_quantize`` does: with amax =
    1.M x 2^(E - 127) it is b = E - 2, or E - 1 when 1.M > 1.5.  b is clamped to [2, 252], so every
    dequantised value is a finite normal bf16 (amax beyond 6 x 2^125 then clips to 6); a zero block has
    b = 127 and zero codes.  Codes: x / 2^(b - 127) (exact) rounded to the grid 0, 0.5, 1, 1.5, 2, 3, 4, 6
    with ties to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4);
    a zero is code 0, never -0.  Byte i of a row holds k = 2i in its low nibble and k = 2i + 1 in its
    high one (the order in which v_cvt_scalef32_pk_bf16_fp4 delivers them)."""
    N, K = w.shape
    if K % MXFP4_BLOCK:
        raise ValueError("weight_quantize_mxfp4 needs K % 32 == 0")
    xf = w.float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = xf.abs().amax(-1)
    bits = amax.contiguous().view(torch.int32)
    E, M = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    b = (E - 2 + (M > 0x400000).to(torch.int32)).clamp(2, 252)
    b = torch.where(amax == 0, torch.full_like(b, 127), b)
    inv = ((254 - b) << 23).view(torch.float32)  # 2^-(b - 127)
    y = xf * inv[..., None]
    a = y.abs().clamp(max=MXFP4_GRID[-1])
    code = torch.zeros(a.shape, dtype=torch.int32, device=a.device)
    for i in range(7):  # the midpoint between codes i and i + 1 goes to the even one
        mid = (MXFP4_GRID[i] + MXFP4_GRID[i + 1]) / 2
        code += (a > mid if i % 2 == 0 else a >= mid).to(torch.int32)
    code |= ((y < 0) & (code > 0)).to(torch.int32) << 3
    code = code.reshape(N, K // 2, 2)
    return (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8), b.to(torch.uint8)


def weight_dequantize_mxfp4(codes, scales):
    """(codes [N, K/2], scale bytes [N, K/32]) -> bf16 [N, K]; exact (a code's magnitude has at most two
    significant bits and the scale bytes of ``weight_quantize_mxfp4`` keep every product normal)."""
    N, K = codes.shape[0], codes.shape[1] * 2
    lut = torch.tensor(MXFP4_GRID + tuple(-v for v in MXFP4_GRID), dtype=torch.float32, device=codes.device)
    c = codes.to(torch.int64)
    vals = lut[torch.stack([c & 15, c >> 4], -1).reshape(N, K)]
    scale = (scales.to(torch.int32) << 23).view(torch.float32)
    return (vals.reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK) * scale[..., None]).reshape(N, K).to(torch.bfloat16)


def rope_kv_write_fp8(qkv, positions, cos_sin, k_data, k_exp, v_data, v_exp, slots, Hq, Hkv, D, block_size):
    """``rope_kv_write`` into an FP8 cache: what the bf16 cache would hold is quantised per row."""
    T = qkv.shape[0]
    kb = torch.zeros((1, Hkv, T, D), dtype=qkv.dtype, device=qkv.device)
    vb = torch.zeros_like(kb)
    q = rope_kv_write(qkv, positions, cos_sin, kb, vb, torch.arange(T, device=qkv.device), Hq, Hkv, D, T)
    # (an fp32 model on the CPU: the bf16 rounding the GPU cache would hold is quantised)
    kd, ke = kv_quantize(kb[0].to(torch.bfloat16))  # [Hkv, T, D], [Hkv, T]
    vd, ve = kv_quantize(vb[0].to(torch.bfloat16))
    for t in range(T):
        s = int(slots[t])
        if s < 0:
            continue
        blk, off = divmod(s, block_size)
        k_data[blk, :, off], k_exp[blk, :, off] = kd[:, t], ke[:, t]
        v_data[blk, :, off], v_exp[blk, :, off] = vd[:, t], ve[:, t]
    return q


def kv_dequant_blocks(data, exps, block_ids, out):
    """out[i] = bf16 image of block ``block_ids[i]`` (data [blocks, Hkv, bs, D], exps [blocks, Hkv, bs])."""
    idx = block_ids.long()
    out[: idx.numel()] = kv_dequantize(data[idx], exps[idx]).to(out.dtype)
    return out


def gather_paged_fp8(data, exps, block_table, n):
    """The first n tokens of a sequence, dequantised on gather: fp32 [n, Hkv, D]."""
    bs = data.shape[2]
    idx = block_table[: (n + bs - 1) // bs].long()
    blocks = kv_dequantize(data[idx], exps[idx])  # [nb, Hkv, bs, D]
    return blocks.permute(0, 2, 1, 3).reshape(idx.numel() * bs, data.shape[1], data.shape[3])[:n]


def flash_attention_paged_fp8(q, k_data, k_exp, v_data, v_exp, block_tables, cu_q, ctx_lens, causal, scale):
    out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    cq = cu_q.tolist()
    for b in range(len(cq) - 1):
        n = int(ctx_lens[b])
        ks = gather_paged_fp8(k_data, k_exp, block_tables[b], n)
        vs = gather_paged_fp8(v_data, v_exp, block_tables[b], n)
        qs = q[cq[b]:cq[b + 1]]
        out[cq[b]:cq[b + 1]] = _attend(qs, ks, vs, scale, causal, n - qs.shape[0]).to(q.dtype)
    return out


def paged_decode_fp8(q, k_data, k_exp, v_data, v_exp, block_tables, ctx_lens, scale):
    out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    for b in range(q.shape[0]):
        n = int(ctx_lens[b])
        ks = gather_paged_fp8(k_data, k_exp, block_tables[b], n)
        vs = gather_paged_fp8(v_data, v_exp, block_tables[b], n)
        out[b] = _attend(q[b:b + 1], ks, vs, scale, False, 0)[0].to(q.dtype)
    return out


def gemm_bt(A, B, bias=None, residual=None, epilogue=EPI_NONE, out_f32=False, row_group=None, q_group=None,
            allow=None):
    c = A.float() @ B.float().t()
    if epilogue == EPI_SCORES:
        ok = torch.ones_like(c, dtype=torch.bool)
        if row_group is not None:
            rg = row_group.long()[None, :]
            ok &= rg >= 0
            if q_group is not None:
                qg = q_group.long()[:, None]
                ok &= (qg < 0) | (rg == qg)
        if allow is not None:
            n = c.shape[1]
            idx = torch.arange(n, device=c.device)
            bits = (allow[:, idx // 32].long() >> (idx % 32)) & 1
            ok &= bits.bool()
        c = c.masked_fill(~ok, float("-inf"))
        return c if out_f32 else c.to(A.dtype)
    if bias is not None:
        c = c + bias.float()
    if epilogue == EPI_GELU:
        c = F.gelu(c)
    elif epilogue in (EPI_SWIGLU, EPI_SWIGLU8):
        N, hg = c.shape[1], 16 if epilogue == EPI_SWIGLU else 8
        c = c.view(c.shape[0], N // (2 * hg), 2, hg)
        c = (F.silu(c[:, :, 0]) * c[:, :, 1]).reshape(c.shape[0], N // 2)
    if residual is not None:
        # a bf16 output is the rounded projection plus the residual, rounded again (HF's
        # `hidden + dense(x)` in bf16)
        c = (c if out_f32 else c.to(A.dtype).float()) + residual.float()
    return c if out_f32 else c.to(A.dtype)


def sample_hf(logits, temperature, top_k, top_p, generator=None):
    """HF generate() logits-warper semantics: temperature -> top-k -> top-p -> multinomial."""
    out = []
    for r in range(logits.shape[0]):
        x = logits[r].float()
        t = float(temperature[r])
        if t <= 0:
            out.append(int(torch.argmax(x)))
            continue
        x = x / t
        k = int(top_k[r])
        if 0 < k < x.numel():
            kth = torch.topk(x, k).values[-1]
            x = x.masked_fill(x < kth, float("-inf"))
        p = float(top_p[r])
        if p < 1.0:
            sl, si = torch.sort(x, descending=False)
            cum = torch.softmax(sl, -1).cumsum(-1)
            remove = cum <= (1 - p)
            remove[-1] = False
            x = x.masked_fill(torch.zeros_like(remove).scatter(0, si, remove), float("-inf"))
        probs = torch.softmax(x, -1)
        out.append(int(torch.multinomial(probs, 1, generator=generator)))
    return torch.tensor(out, dtype=torch.int32, device=logits.device)


def topk_rows(scores, k):
    v, i = torch.topk(scores.float(), k, dim=-1, largest=True, sorted=True)
    return v, i.to(torch.int32)


def rope_cos_sin(inv_freq: torch.Tensor, max_pos: int) -> torch.Tensor:
    t = torch.arange(max_pos, dtype=torch.float32)
    f = torch.outer(t, inv_freq.float())
    return torch.stack([f.cos(), f.sin()], dim=-1).contiguous()  # [max_pos, D/2, 2]


def llama3_inv_freq(D, theta, scaling=None):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    if not scaling:
        return inv
    factor = scaling.get("factor", 8.0)
    lo = scaling.get("low_freq_factor", 1.0)
    hi = scaling.get("high_freq_factor", 4.0)
    orig = scaling.get("original_max_position_embeddings", 8192)
    lo_wl, hi_wl = orig / lo, orig / hi
    wl = 2 * math.pi / inv
    out = torch.where(wl > lo_wl, inv / factor, inv)
    smooth = (orig / wl - lo) / (hi - lo)
    mid = (1 - smooth) * out / factor + smooth * out
    is_mid = (wl >= hi_wl) & (wl <= lo_wl)
    return torch.where(is_mid, mid, out)
