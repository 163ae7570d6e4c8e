"""The opt-in FP8 KV cache on the GPU (csrc/kernels/kv_fp8.hip): the quantising RoPE + cache writer bit
for bit against ``ref.kv_quantize`` of what the bf16 writer stores, the FP8 paged decode kernel (both
dispatch arms) on the needle cases of tests/attn_cases.py, the block dequantiser and the prefill
attention over its scratch bit for bit against the bf16 kernels on the dequantised values, and the
model / engine with ``kv_dtype="fp8"``.

The decode and prefill cases are checked by ``attn_cases.check`` against the fp64 reference of the
DEQUANTISED values (tests/kv_fp8_cases.py), with its own bound tau = 4 f.

Largest observed relative error / f per kernel family on an MI355X (the bound is 4, tau_factor is left at its
default; f is 2.4e-3 to 3.0e-3 on the plain cases).  Every needle row returned its code exactly (deviation 0.0):

    fp8 decode two-slot DMA             1.00   (dec_d-bs128-s8 plain, unsplit)
    fp8 decode one-slot DMA             0.99   (dec_b-p512 plain, split)
    fp8 prefill (dequantised scratch)   1.26   (pre_f-n plain; bit-equal to the bf16 kernel on the same values)
"""
import math

import pytest
import torch

import attn_cases as ac
import kv_fp8_cases as fc
from django_assistant_bot_amd import ops
from django_assistant_bot_amd.models.configs import DecoderConfig
from django_assistant_bot_amd.models.llama import AttnMeta, KVCache, LlamaModel
from django_assistant_bot_amd.models.weights import random_decoder_weights
from django_assistant_bot_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x5A


# ---------------------------------------------------------------------------------------------- writer

T_W, HQ, HKV, D, BS, NBLK = 67, 4, 2, 128, 64, 3


def _writer_inputs():
    g = torch.Generator().manual_seed(11)
    W = (HQ + 2 * HKV) * D
    # per-head magnitudes from 2^-6 to 2^5: many different exponent bytes
    mag = torch.exp2(torch.randint(-6, 6, (T_W, HQ + 2 * HKV, 1), generator=g).float())
    qkv = (torch.randn(T_W, HQ + 2 * HKV, D, generator=g) * mag).reshape(T_W, W)
    qkv[9] = 0  # an all-zero token
    slabs32 = torch.randn(4, T_W, W, generator=g) * 0.25 + qkv[None] / 4
    slabs32[:, 9] = 0
    perm = torch.randperm(NBLK * BS, generator=g)
    must = torch.tensor([0, BS - 1, BS, 2 * BS - 1, 2 * BS, 3 * BS - 1])  # first / last slot of every block
    rest = perm[~torch.isin(perm, must)]
    slots = torch.cat([must, rest[:T_W - must.numel()]])[torch.randperm(T_W, generator=g)]
    slots[[4, 40]] = -1
    pos = torch.randint(0, 500, (T_W,), generator=g, dtype=torch.int32)
    cs = ref.rope_cos_sin(ref.llama3_inv_freq(D, 500000.0, None), 512)
    forms = {"bf16": qkv.bfloat16(), "slabs32": slabs32.contiguous(), "slabs16": slabs32.bfloat16().contiguous()}
    return {k: v.to(DEV) for k, v in forms.items()}, pos.to(DEV), cs.to(DEV), slots.to(DEV)


@pytest.mark.parametrize("form,write_q", [("bf16", True), ("bf16", False), ("slabs32", True), ("slabs16", True)])
def test_writer_is_the_bf16_writer_quantised(form, write_q):
    forms, pos, cs, slots = _writer_inputs()
    x = forms[form]
    kb = torch.zeros(NBLK, HKV, BS, D, dtype=torch.bfloat16, device=DEV)
    vb = torch.zeros_like(kb)
    q0 = ops.rope_kv_write(x, pos, cs, kb, vb, slots, HQ, HKV, D, write_q=write_q)
    cache = [torch.full((NBLK, HKV, BS, D), SENT, dtype=torch.uint8, device=DEV),
             torch.full((NBLK, HKV, BS), SENT, dtype=torch.uint8, device=DEV),
             torch.full((NBLK, HKV, BS, D), SENT, dtype=torch.uint8, device=DEV),
             torch.full((NBLK, HKV, BS), SENT, dtype=torch.uint8, device=DEV)]
    q1 = ops.rope_kv_write_fp8(x, pos, cs, *cache, slots, HQ, HKV, D, write_q=write_q)
    torch.cuda.synchronize()
    if write_q:
        assert torch.equal(q0, q1)
    else:
        assert q0 is None and q1 is None
    written = torch.zeros(NBLK * BS, dtype=torch.bool)
    sl = slots.cpu()
    written[sl[sl >= 0]] = True
    assert int(written.sum()) == T_W - 2
    w = written.view(NBLK, 1, BS).expand(NBLK, HKV, BS)
    nexp = set()
    for name, (data, exps), bf in (("k", cache[:2], kb), ("v", cache[2:], vb)):
        d, e = ref.kv_quantize(bf.cpu())
        data, exps = data.cpu(), exps.cpu()
        bad = (data[w] != d[w]).nonzero()
        assert torch.equal(exps[w], e[w]), name
        assert bad.numel() == 0, (name, bad[:4].tolist(), data[w][bad[0, 0]].tolist(), d[w][bad[0, 0]].tolist())
        assert bool((data[~w] == SENT).all()) and bool((exps[~w] == SENT).all()), name
        nexp |= set(e[w].tolist())
    assert len(nexp) >= 8 and 127 in nexp  # (127: the all-zero token)


# ---------------------------------------------------------------------------------------------- decode

RATIOS = {}


def _assert(view, out, family, tag, tau_factor=ac.TAU_FACTOR):
    rep = ac.check(view, out, tau_factor)
    print(f"KVFP8 family={family!r} case={tag} err/f={rep.ratio} f={rep.f} tau={rep.tau} "
          f"needle_dev={rep.needle_dev} max_abs={rep.close_err}")
    if rep.ratio is not None:
        RATIOS[family] = max(RATIOS.get(family, 0.0), rep.ratio)
    assert torch.isfinite(out.float()).all()
    assert rep.ok, str(rep)
    assert rep.tau is None or rep.tau <= ac.TAU_CAP
    return rep


def _forms(name, scaled=False):
    forms = [(fc.get_fp8(name, DEV, True), f"{name}/needles"), (fc.get_fp8(name, DEV, False), f"{name}/plain")]
    if scaled:
        forms.append((fc.get_fp8(name, DEV, False, True), f"{name}/plain-rowscaled"))
    return forms


def _decode(view, cache, tag, family, split, **kw):
    ws = None
    if split:
        ws = ops.DecodeWorkspace(view.B, view.Hq, view.D, math.ceil(max(view.klens) / view.part), DEV)
    out = fc.run_fp8(view, cache, ops, workspace=ws, **kw)
    rep = _assert(view, out, family, f"{tag}/{'split' if split else 'unsplit'}")
    if view.n_row is not None:
        assert rep.needle_dev == 0.0
    if split:  # the in-launch combine leaves its arrival counters at rest, and a relaunch agrees
        assert int(ws.cnt.abs().sum()) == 0
        assert torch.equal(fc.run_fp8(view, cache, ops, workspace=ws, **kw), out)
        assert int(ws.cnt.abs().sum()) == 0
    return out


TWO_SLOT, ONE_SLOT = "fp8 decode two-slot DMA", "fp8 decode one-slot DMA"


@pytest.mark.parametrize("split", [True, False])
def test_decode_two_slot(split):
    """dec_a-s8 -- paged_decode_fp8_kernel<2>: batch * Hkv = 32 <= 64; 16 partitions of 512 / one of 8192
    (64 sub-tiles per wave); plus the row-scaled plain form (a different exponent byte on every row)."""
    for (view, cache), tag in _forms("dec_a-s8", scaled=True):
        assert view.B * view.Hkv <= 64 and view.bt.shape[1] * view.bs <= 8192
        _decode(view, cache, tag, TWO_SLOT, split)


def test_decode_two_slot_scale_order_out():
    order = torch.tensor([2, 0, 3, 1], dtype=torch.int32, device=DEV)
    for (view, cache), tag in _forms("dec_a-scale"):
        assert view.scale != 1 / math.sqrt(view.D)
        for split in (True, False):
            out = torch.full_like(view.q, 7.0)
            assert _decode(view, cache, tag, TWO_SLOT, split, order=order, out=out) is out


@pytest.mark.parametrize("name,split", [("dec_b-p512", True), ("dec_b-p512", False), ("dec_b-p2048", True)])
def test_decode_one_slot(name, split):
    """dec_b -- paged_decode_fp8_kernel<1>: batch * Hkv = 72 > 64; p2048 split: the direct-store partition."""
    for (view, cache), tag in _forms(name, scaled=name == "dec_b-p512"):
        assert view.B * view.Hkv > 64
        _decode(view, cache, tag, ONE_SLOT, split)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", [n for n in sorted(ac.CASES) if n.startswith(("dec_d", "dec_e"))])
def test_decode_block_sizes_and_gqa_groups(name, split):
    """32- / 128-slot blocks under the 32-key sub-tiles, GQA groups of 16 and 2; split: 3 partitions of 128."""
    for (view, cache), tag in _forms(name):
        _decode(view, cache, tag, TWO_SLOT, split)


def test_decode_refuses_head_dim_64_and_warm():
    view, cache = fc.get_fp8("dec_e-g2-s0", DEV, True)
    with pytest.raises(ValueError, match="warm"):
        fc.run_fp8(view, cache, ops, warm=([(view.q, 16)], 4))
    q = torch.zeros(2, 4, 64, dtype=torch.bfloat16, device=DEV)
    data = torch.zeros(4, 2, 64, 64, dtype=torch.uint8, device=DEV)
    exps = torch.zeros(4, 2, 64, dtype=torch.uint8, device=DEV)
    bt = torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    ctx = torch.ones(2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="head dim 128"):
        ops.paged_decode_fp8(q, data, exps, data, exps, bt, ctx)
    with pytest.raises(ValueError, match="head dim 128"):
        ops.rope_kv_write_fp8(torch.zeros(2, 8 * 64, dtype=torch.bfloat16, device=DEV), ctx, torch.zeros(8, 32, 2, device=DEV),
                              data, exps, data, exps, torch.zeros(2, dtype=torch.int64, device=DEV), 4, 2, 64)
    with pytest.raises(TypeError, match="uint8"):
        ops.paged_decode_fp8(view.q, cache[0].to(torch.int8), *cache[1:], view.bt, view.ctx)


# ---------------------------------------------------------------------------------------------- dequantiser, prefill


def _scratch(view, cap, fill=None):
    shape = (cap, view.Hkv, view.bs, view.D)
    if fill is None:
        return torch.zeros(shape, dtype=torch.bfloat16, device=DEV), torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    return (torch.full(shape, fill, dtype=torch.bfloat16, device=DEV), torch.full(shape, fill, dtype=torch.bfloat16, device=DEV))


def test_dequantiser_listed_blocks_only():
    view, cache = fc.get_fp8("pre_f-c", DEV, False, True)
    nb = cache[0].shape[0]
    ids = torch.tensor([nb - 1, 0, 3, 3, 5], dtype=torch.int32, device=DEV)
    sk, sv = _scratch(view, 8, fill=9.0)
    ops.kv_dequant_blocks(*cache, ids, sk, sv)
    kd, ke, vd, ve = (t.cpu() for t in cache)
    want_k, want_v = ref.kv_dequantize(kd, ke)[ids.cpu().long()], ref.kv_dequantize(vd, ve)[ids.cpu().long()]
    assert torch.equal(sk[:5].float().cpu(), want_k) and torch.equal(sv[:5].float().cpu(), want_v)
    assert torch.equal(sk[:5].cpu(), view.k[ids.long()].cpu())
    assert bool((sk[5:] == 9).all()) and bool((sv[5:] == 9).all())
    assert len({int(x) for x in ke.unique()}) >= 3  # row-scaled: several exponent bytes in play


@pytest.mark.parametrize("name", ["pre_f-c", "pre_f-n", "pre_g", "pre_long"])
def test_prefill_is_the_bf16_kernel_on_the_dequantised_values(name):
    """One group: the scratch holds the dequantised blocks, so the output equals, bit for bit, the bf16
    prefill attention over a bf16 cache of the dequantised values (the same kernel on the same numbers)."""
    for (view, cache), tag in _forms(name):
        nblk = sum(-(-n // view.bs) for n in view.klens)
        out = fc.run_fp8(view, cache, ops, scratch=_scratch(view, nblk))
        rep = _assert(view, out, "fp8 prefill (dequantised scratch)", tag)
        if view.n_row is not None:
            assert rep.needle_dev == 0.0
        assert torch.equal(out, ac.run(view, ops))


def test_prefill_in_groups_of_whole_sequences():
    """pre_g through a scratch of 12 blocks: >= 3 groups; scratch rows past the plan's blocks keep a sentinel."""
    for (view, cache), tag in _forms("pre_g"):
        plan = ops.kv_prefill_plan(view.bt, view.ctx, view.cu_q, view.bs, 12, DEV)
        assert len(plan.groups) >= 3 and all(g[3] - g[2] <= 12 for g in plan.groups)
        sk, sv = _scratch(view, 14, fill=9.0)
        out = fc.run_fp8(view, cache, ops, scratch=(sk, sv), plan=plan)
        _assert(view, out, "fp8 prefill (dequantised scratch)", f"{tag}/groups")
        assert torch.equal(out, ac.run(view, ops))
        assert bool((sk[12:] == 9).all()) and bool((sv[12:] == 9).all())
    with pytest.raises(ValueError, match="exceeds the FP8 prefill scratch"):
        ops.kv_prefill_plan(view.bt, view.ctx, view.cu_q, view.bs, 4, DEV)


def test_prefill_rope_on_load_over_the_scratch():
    """``rope=`` (q rotated on load) through the FP8 helper == the bf16 kernel with ``rope=`` on the dequantised cache."""
    view, cache = fc.get_fp8("pre_f-c", DEV, False)
    pos = torch.cat([torch.arange(n - m, n, dtype=torch.int32) for n, m in zip(view.klens, view.qlens)]).to(DEV)
    cs = ref.rope_cos_sin(ref.llama3_inv_freq(view.D, 500000.0, None), 512).to(DEV)
    nblk = sum(-(-n // view.bs) for n in view.klens)
    a = fc.run_fp8(view, cache, ops, scratch=_scratch(view, nblk), rope=(pos, cs))
    assert torch.equal(a, ac.run(view, ops, rope=(pos, cs)))
    plan = ops.kv_prefill_plan(view.bt, view.ctx, view.cu_q, view.bs, 5, DEV)
    assert len(plan.groups) > 1
    assert torch.equal(a, fc.run_fp8(view, cache, ops, scratch=_scratch(view, 5), rope=(pos, cs), plan=plan))


# ---------------------------------------------------------------------------------------------- model and engine

TOY = DecoderConfig("toy-d128", vocab_size=1024, hidden=512, layers=2, heads=4, kv_heads=2, intermediate=1024,
                    max_position=2048, bos_id=1000, eos_ids=(1001,), rope_scaling=None, rope_theta=10000.0)


def _run(model, cfg, prompts, device, dtype, kv_dtype):
    """tests/test_models_gpu.py ``_run``: prefill every prompt but its last token, then one decode step."""
    bs, nb_per = 64, 4
    B = len(prompts)
    kv = KVCache(cfg.layers, B * nb_per, cfg.kv_heads, bs, cfg.head_dim, device, dtype=dtype, kv_dtype=kv_dtype,
                 scratch_blocks=nb_per)
    bt = torch.arange(B * nb_per, dtype=torch.int32, device=device).view(B, nb_per)
    for b, ids in enumerate(prompts):
        T = len(ids) - 1
        meta = AttnMeta(decode=False, positions=torch.arange(T, dtype=torch.int32, device=device),
                        slots=(bt[b, 0].long() * bs + torch.arange(T, device=device)),
                        block_tables=bt[b:b + 1], ctx_lens=torch.tensor([T], dtype=torch.int32, device=device),
                        cu_q=torch.tensor([0, T], dtype=torch.int32, device=device), max_q=T)
        model.forward(torch.tensor(ids[:-1], dtype=torch.int32, device=device), meta, kv)
    pos = torch.tensor([len(p) - 1 for p in prompts], dtype=torch.int32, device=device)
    slots = bt[:, 0].long() * bs + pos.long()
    ws = ops.DecodeWorkspace(B, cfg.heads, cfg.head_dim, nb_per * bs // 512 + 1, device) if device != "cpu" else None
    meta = AttnMeta(decode=True, positions=pos, slots=slots, block_tables=bt, ctx_lens=pos + 1, workspace=ws)
    return model.forward(torch.tensor([p[-1] for p in prompts], dtype=torch.int32, device=device), meta, kv)


@pytest.mark.parametrize("B", [3, 128])
def test_forward_matches_the_cpu_fp8_oracle(B):
    cfg = TOY
    w32 = random_decoder_weights(cfg, dtype=torch.float32, seed=5, interleave_mlp=True)
    gen = torch.Generator().manual_seed(B)
    prompts = [torch.randint(0, cfg.vocab_size, (int(n),), generator=gen).tolist()
               for n in torch.randint(10, 150, (B,), generator=gen)]
    wbf = {k: v.to(torch.bfloat16) for k, v in w32.items()}
    m = LlamaModel(cfg, wbf, DEV, interleaved_mlp=True)
    assert m.frag
    h8 = _run(m, cfg, prompts, DEV, torch.bfloat16, "fp8")
    h16 = _run(m, cfg, prompts, DEV, torch.bfloat16, "bf16")
    m_ref = LlamaModel(cfg, {k: v.bfloat16().float() for k, v in w32.items()}, "cpu", interleaved_mlp=True)
    r8 = _run(m_ref, cfg, prompts, "cpu", torch.float32, "fp8")
    r16 = _run(m_ref, cfg, prompts, "cpu", torch.float32, "bf16")
    err8 = (h8.float().cpu() - r8).abs().max().item()
    err16 = (h16.float().cpu() - r16).abs().max().item()
    print(f"KVFP8 model B={B}: fp8 GPU vs fp8 oracle {err8:.4f}; bf16 GPU vs fp32 oracle {err16:.4f}; "
          f"fp8 oracle vs fp32 oracle {(r8 - r16).abs().max().item():.4f}")
    assert err8 < 0.15, err8


def test_mixed_forward_matches_separate_prefill_and_decode_fp8():
    """tests/test_models_gpu.py test_mixed_forward_matches_separate_prefill_and_decode on an FP8 cache, under
    that test's assertion (atol 5e-2, rtol 5e-2).

    The separate prefill step (123 tokens <= PREFILL_STREAM_MAX_M) streams its projections through the split-K
    decode GEMM, the mixed step (128 rows) runs the MFMA GEMMs.  The qkv projection keeps fp32 slabs under an
    FP8 cache (``LlamaModel.fp8_qkv_slab_f32``), so the two schedules cache the same layer-0 bytes (0-1 of 31k K
    bytes differ) and agree as closely as with a bf16 cache.  Measured on an MI355X over three weight seeds:
    prefill rows largest |mixed - separate| 0.047-0.055, none of 62,976 elements over the bound, mean 0.0059
    (bf16 cache: 0.047-0.0625, mean 0.0056-0.0060); decode rows 0.031.  With bf16 qkv slabs the quantiser turned
    their last-bit differences into 1.7-1.8k differing layer-0 K bytes and the same comparison gave 0.070-0.102
    with 9-54 elements over (mean 0.014)."""
    cfg = TOY
    w = {k: v.to(torch.bfloat16) for k, v in
         random_decoder_weights(cfg, dtype=torch.float32, seed=9, interleave_mlp=True).items()}
    model = LlamaModel(cfg, w, DEV, interleaved_mlp=True)
    bs, nbp = 64, 4
    gen = torch.Generator().manual_seed(0)
    dec_prompts = [torch.randint(0, 900, (int(n),), generator=gen).tolist() for n in (40, 130, 77)]
    pre_prompts = [torch.randint(0, 900, (int(n),), generator=gen).tolist() for n in (90, 33)]
    nd, npf = len(dec_prompts), len(pre_prompts)
    i32 = dict(dtype=torch.int32, device=DEV)

    def fresh_cache():
        kv = KVCache(cfg.layers, (nd + npf + 1) * nbp, cfg.kv_heads, bs, cfg.head_dim, DEV, kv_dtype="fp8")
        for b, ids in enumerate(dec_prompts):
            T = len(ids) - 1
            bt = torch.arange(b * nbp, (b + 1) * nbp, **i32)[None]
            meta = AttnMeta(decode=False, positions=torch.arange(T, **i32), slots=bt[0, 0].long() * bs +
                            torch.arange(T, device=DEV), block_tables=bt, ctx_lens=torch.tensor([T], **i32),
                            cu_q=torch.tensor([0, T], **i32), max_q=T)
            model.forward(torch.tensor(ids[:-1], **i32), meta, kv)
        return kv

    dbt = torch.arange(nd * nbp, **i32).view(nd, nbp)
    dpos = torch.tensor([len(p) - 1 for p in dec_prompts], **i32)
    dslots = dbt[:, 0].long() * bs + dpos.long()
    dids = torch.tensor([p[-1] for p in dec_prompts], **i32)
    pbt = torch.arange(nd * nbp, (nd + npf) * nbp, **i32).view(npf, nbp)
    pids = torch.tensor([t for p in pre_prompts for t in p], **i32)
    ppos = torch.cat([torch.arange(len(p), **i32) for p in pre_prompts])
    pslots = torch.cat([pbt[i, 0].long() * bs + torch.arange(len(p), device=DEV) for i, p in enumerate(pre_prompts)])
    cu = torch.tensor([0, len(pre_prompts[0]), len(pre_prompts[0]) + len(pre_prompts[1])], **i32)
    pctx = torch.tensor([len(p) for p in pre_prompts], **i32)
    ws = ops.DecodeWorkspace(8, cfg.heads, cfg.head_dim, nbp * bs // 512 + 1, DEV)
    kv = fresh_cache()
    h_pre = model.forward(pids, AttnMeta(decode=False, positions=ppos, slots=pslots, block_tables=pbt,
                                         ctx_lens=pctx, cu_q=cu, max_q=90), kv)
    h_dec = model.forward(dids, AttnMeta(decode=True, positions=dpos, slots=dslots, block_tables=dbt,
                                         ctx_lens=dpos + 1, workspace=ws), kv)
    kv2 = fresh_cache()
    pad = 2
    mbt = torch.cat([dbt, torch.zeros((pad, nbp), **i32)])
    mctx = torch.cat([dpos + 1, torch.ones(pad, **i32)])
    ids = torch.cat([pids, dids, torch.zeros(pad, **i32)])
    pos = torch.cat([ppos, dpos, torch.zeros(pad, **i32)])
    slots = torch.cat([pslots, dslots, torch.full((pad,), -1, dtype=torch.int64, device=DEV)])
    meta = AttnMeta(decode=False, positions=pos, slots=slots, block_tables=pbt, ctx_lens=pctx, cu_q=cu, max_q=90,
                    workspace=ws, n_decode=nd + pad, dec_block_tables=mbt, dec_ctx_lens=mctx)
    h_mix = model.forward(ids, meta, kv2)
    Tp = pids.numel()
    torch.testing.assert_close(h_mix[:Tp].float(), h_pre.float(), atol=5e-2, rtol=5e-2)
    torch.testing.assert_close(h_mix[Tp:Tp + nd].float(), h_dec.float(), atol=5e-2, rtol=5e-2)
    assert kv2.k.dtype == torch.uint8 and meta.kv_groups is not None


def test_engine_greedy_graphs_on_equals_graphs_off():
    from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams

    w = {k: v.to(torch.bfloat16) for k, v in random_decoder_weights(TOY, dtype=torch.float32, seed=4,
                                                                    interleave_mlp=True).items()}
    prompts = [list(range(10, 10 + n)) for n in (10, 77, 150, 300)]
    greedy = SamplingParams(max_new_tokens=24, do_sample=False, temperature=0.0, ignore_eos=True)
    outs = {}
    for graphs in (True, False):
        eng = LLMEngine(TOY, device=DEV, weights=dict(w), max_batch=8, block_size=64, num_blocks=64,
                        max_prefill_tokens=256, max_model_len=384, use_graphs=graphs, kv_cache_dtype="fp8",
                        kv_scratch_blocks=6)  # 6 blocks: the first prefill step (7 context blocks) runs in two groups
        assert eng.kv.scratch_blocks == 6
        assert eng.kv_cache_dtype == "fp8" and eng.kv.k.dtype == torch.uint8 and eng.stats["kv_cache_bits"] == 8
        rids = [eng.add_request(p, greedy) for p in prompts]
        while eng.has_unfinished():
            eng.step()
        outs[graphs] = [eng.pop_output(r).token_ids for r in rids]
        assert (eng.stats["graph_replays"] > 0) == graphs
        assert eng.blocks.num_free_blocks() == eng.blocks.num_blocks()
    assert outs[True] == outs[False] and all(len(t) == 24 for t in outs[True])
