"""Opt-in FP8 projection weights (W8A16) on the GPU: the FP8 arm of the streaming decode GEMM
(``ops.stream_gemm(..., w_exps=...)``), ``LlamaModel(weight_dtype="fp8")`` and ``LLMEngine(weight_dtype="fp8")``.

Power-of-two row scales make every dequantised weight bf16-exact and commute with every rounding, so
the FP8 kernel must EQUAL the bf16 kernel run on the dequantised weights; the one-hot tests pin the
layout and the exponents without the bf16 kernel."""
import math

import pytest
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.models import llama
from django_assistant_bot_amd.models.configs import DecoderConfig
from django_assistant_bot_amd.models.llama import AttnMeta, Fp8Proj, KVCache, LlamaModel
from django_assistant_bot_amd.models.weights import random_decoder_weights

pytestmark = pytest.mark.gpu

DEV = "cuda"
# what the decoder can dispatch for qkv / o / gate_up / down: _stream_cfg (30, 31, 13, 10, 27), the
# wide gate_up tiling (20) and the small-batch residual producers (32)
FP8_CFGS = [10, 13, 20, 27, 30, 31, 32]
PROJ = ("qkv_w", "o_w", "gate_up_w", "down_w")


@pytest.fixture
def ring(request):
    """The FP8 arm's ring depth mode for one test (0: the bf16 configuration's, 1: twice that)."""
    nat = ops.native()
    old = nat.stream_gemm_fp8_deep()
    nat.stream_gemm_fp8_set_deep(request.param)
    yield request.param
    nat.stream_gemm_fp8_set_deep(old)


def _weights(N, K, seed):
    """bf16 [N, K] with row magnitudes 2^-10 .. 2^2, both signs, one zero row (row 3)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-10, 3, (N, 1), generator=g).float())
    w[3] = 0
    return w.bfloat16()


def _quantised(N, K, seed, group=1):
    """(FP8 fragment copy, exponents, bf16 fragment copy of the dequantised values, dequantised [N, K])."""
    data, exps = ops.weight_quantize_fp8(_weights(N, K, seed))
    dq = ops.weight_dequantize_fp8(data, exps)
    return (ops.shuffle_weights_fp8(data, group).to(DEV), exps.to(DEV), ops.shuffle_weights(dq, group).to(DEV), dq)


def test_fp8_ok_names_the_dispatched_configurations():
    nat = ops.native()
    assert [c for c in range(64) if nat.stream_gemm_fp8_ok(c)] == FP8_CFGS
    assert not nat.stream_gemm_fp8_ok(-1) and not nat.stream_gemm_fp8_ok(28)  # (the LM head's is not)
    m = LlamaModel
    assert {m.STREAM_CFG_M16, m.STREAM_CFG_M32, m.STREAM_CFG_M64, m.STREAM_CFG_M128, m.STREAM_CFG_M256,
            m.STREAM_WIDE["gate_up"], m.STREAM_CFG_RES16} == set(FP8_CFGS)
    for c in FP8_CFGS:
        assert nat.stream_gemm_shuffled(c)


# ----------------------------------------------------------------------------------------- kernel: one-hot


@pytest.mark.parametrize("ring", [0, 1], indirect=True)
@pytest.mark.parametrize("cfg", FP8_CFGS)
def test_one_hot_rows_read_the_dequantised_weights(cfg, ring):
    """X rows with a single 1.0: the output row is column k of the dequantised weights, exactly
    (one exact product, zeros added).  A wrong lane map, k half, exponent row or slice offset fails."""
    nat = ops.native()
    N, K, S = 2 * nat.stream_gemm_bn(cfg), 512, 2
    kc = K // S
    # both k halves of a 64-step, every lane quadrant, first / last k of a K-slice, the last k of K
    ks = [0, 9, 18, 27, 36, 45, 54, 63, 64, 127, 128, kc - 1, kc, kc + 33, K - 64, K - 1]
    w8, e, _, dq = _quantised(N, K, 11 + cfg)
    x = torch.zeros((len(ks), K), dtype=torch.bfloat16)
    x[torch.arange(len(ks)), torch.tensor(ks)] = 1.0
    x = x.to(DEV)
    want = dq[:, ks].t().contiguous()  # [M, N]
    assert bool((want[:, 3] == 0).all()) and bool((want < 0).any()) and float(want.abs().max()) > 0
    y = ops.stream_gemm(x, w8, w_exps=e, cfg=cfg, nt=True)
    assert y.dtype == torch.bfloat16 and torch.equal(y.cpu(), want)
    slabs = ops.stream_gemm(x, w8, w_exps=e, cfg=cfg, nt=False, splits=S).cpu()
    assert slabs.dtype == torch.float32 and slabs.shape == (S, len(ks), N)
    for m, k in enumerate(ks):
        own = k // kc
        assert torch.equal(slabs[own, m], want[m].float()), (m, k)
        assert not bool(slabs[1 - own, m].any()), (m, k)


# ------------------------------------------------------------------- kernel: bit equality with the bf16 kernel


def _forms(x, w, e, cfg, S, res, **kw):
    """Every output form of one (x, weights) pair; ``e`` None: the bf16 kernel."""
    a = dict(cfg=cfg, nt=True, w_exps=e, **kw)
    eps = 1e-5
    return {
        "plain": ops.stream_gemm(x, w, **a),
        "residual": ops.stream_gemm(x, w, residual=res, **a),
        "swiglu8": ops.stream_gemm(x, w, epilogue=ops.EPI_SWIGLU8, **a),
        "slabs32": ops.stream_gemm(x, w, splits=S, **a),
        "slabs16": ops.stream_gemm(x, w, splits=S, slab_dtype=torch.bfloat16, **a),
        "norm_slabs32": ops.stream_gemm(x, w, splits=S, norm_eps=eps, **a),
        "norm_swiglu8": ops.stream_gemm(x, w, epilogue=ops.EPI_SWIGLU8, norm_eps=eps, **a),
        "plain_cached_loads": ops.stream_gemm(x, w, **{**a, "nt": False}),
    }


@pytest.mark.parametrize("ring", [0, 1], indirect=True)
@pytest.mark.parametrize("cfg", FP8_CFGS)
def test_bit_equal_to_the_bf16_kernel_on_the_dequantised_weights(cfg, ring):
    """stream_gemm(x, w8, w_exps=e) == stream_gemm(x, shuffle_weights(dq)) for every form the
    configuration serves, at M = 1, 16, 17, an odd value and the maximum, and K-slices shorter than
    the weight ring (clamped spare loads), whole multiples of it and with tail stages."""
    nat = ops.native()
    bn, max_m = nat.stream_gemm_bn(cfg), nat.stream_gemm_max_m(cfg)
    nwin = nat.stream_gemm_fp8_nwin(cfg)
    assert nwin > 0 and nat.stream_gemm_fp8_deep() == ring
    S = 2
    Ms = sorted({m for m in (1, 16, 17, 5 if max_m <= 32 else 2 * (max_m // 3) + 1, max_m) if m <= max_m})
    g = torch.Generator().manual_seed(cfg)
    for nst in (2, nwin, 2 * nwin, nwin + 1):  # stages per K-slice
        K = 128 * nst * S
        for group, N in ((1, 2 * bn), (8, math.lcm(2 * bn, 128))):
            if group == 8 and nst != nwin + 1:
                continue  # (the grouped copy: one K, every form and M)
            w8, e, w16, _ = _quantised(N, K, 100 * cfg + nst, group)
            for M in Ms:
                x = torch.randn(M, K, generator=g).bfloat16().to(DEV)
                res = torch.randn(M, N, generator=g).bfloat16().to(DEV)
                got = _forms(x, w8, e, cfg, S, res, w_group=group)
                want = _forms(x, w16, None, cfg, S, res, w_group=group)
                for name in want:
                    assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape
                    assert torch.equal(got[name], want[name]), (cfg, ring, nst, group, M, name)
                assert bool(want["plain"].float().abs().sum() > 0)


# ------------------------------------------------------------------------------------ kernel: invalid launches


def test_invalid_launches_are_refused_without_a_launch(monkeypatch):
    nat = ops.native()
    cfg = 13
    N, K = 2 * nat.stream_gemm_bn(cfg), 256
    w8, e, w16, _ = _quantised(N, K, 5)
    x = torch.randn(4, K).bfloat16().to(DEV)
    ok = ops.stream_gemm(x, w8, w_exps=e, cfg=cfg)
    launched = []
    real = nat.stream_gemm_fp8
    monkeypatch.setattr(nat, "stream_gemm_fp8", lambda *a, **k: launched.append(1) or real(*a, **k))
    assert torch.equal(ops.stream_gemm(x, w8, w_exps=e, cfg=cfg), ok) and launched == [1]
    with pytest.raises(ValueError, match="K % 64"):
        ops.stream_gemm(x[:, :96].contiguous(), w8[:, :96].contiguous(), w_exps=e, cfg=cfg)
    with pytest.raises(ValueError, match="bf16 operands"):  # FP8 bytes without their exponents
        ops.stream_gemm(x, w8, cfg=cfg)
    for bad in (e[:-1], e[None].expand(2, N), e.to(torch.int32), e.cpu(), e.float()):
        with pytest.raises(ValueError, match="w_exps"):
            ops.stream_gemm(x, w8, w_exps=bad, cfg=cfg)
    with pytest.raises(ValueError, match="uint8 fragment copy"):
        ops.stream_gemm(x, w16, w_exps=e, cfg=cfg)
    for c in (11, 28, 17):  # a fragment-layout cfg without an FP8 arm, the LM head's, an ablation
        assert not nat.stream_gemm_fp8_ok(c)
        with pytest.raises(ValueError, match="no FP8-weight instantiation"):
            ops.stream_gemm(x, w8, w_exps=e, cfg=c)
    assert launched == [1]
    monkeypatch.undo()
    # the entry point itself: hipErrorInvalidValue before any launch
    out = torch.full((4, N), 7.0, dtype=torch.bfloat16, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def raw(K_=K, exps=e.data_ptr(), cfg_=cfg):
        nat.stream_gemm_fp8(x.data_ptr(), K, w8.data_ptr(), exps, out.data_ptr(), N, 0, 0, 4, N, K_, 1, 0, s, 1, cfg_)

    for kw in (dict(K_=K + 32), dict(exps=0), dict(cfg_=11), dict(cfg_=99)):
        with pytest.raises(RuntimeError, match="stream_gemm_fp8"):
            raw(**kw)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    raw()
    assert torch.equal(out, ok)


# -------------------------------------------------------------------------------------------------- model

# every projection streams at decode batches <= 128 and in a 64-token prefill: N % 128 == 0 (cfg 30 /
# 13 / 10), gate_up's 1792 rows are also whole 112-row tiles (cfg 20 at M 65..128), K % 128 == 0
TOY = DecoderConfig("toy-w8", vocab_size=1024, hidden=512, layers=2, heads=4, kv_heads=2, intermediate=896,
                    max_position=2048, bos_id=1000, eos_ids=(1001,), rope_scaling=None, rope_theta=10000.0)


def _toy_weights(seed):
    return {k: v.to(torch.bfloat16) for k, v in random_decoder_weights(TOY, dtype=torch.float32, seed=seed,
                                                                       interleave_mlp=True).items()}


def _dequantised(weights):
    return {k: (ops.weight_dequantize_fp8(*ops.weight_quantize_fp8(v)) if k.endswith(PROJ) else v)
            for k, v in weights.items()}


@pytest.fixture(scope="module")
def toy_models():
    w = _toy_weights(6)
    m8 = LlamaModel(TOY, dict(w), DEV, interleaved_mlp=True, weight_dtype="fp8")
    m16 = LlamaModel(TOY, _dequantised(w), DEV, interleaved_mlp=True)
    assert m8.frag and m16.frag and m8.proj_group == m16.proj_group and m8.proj_group["gate_up"] == 8
    for L8, L16 in zip(m8.layers, m16.layers):
        for n in PROJ:
            p8, p16 = getattr(L8, n), getattr(L16, n)
            assert isinstance(p8, Fp8Proj) and p8.data.dtype == torch.uint8 and p8.shape == p16.shape
            assert torch.equal(p8.w, p16)  # the bf16 copy holds the dequantised values
    assert torch.equal(m8.lm_head, m16.lm_head) and m8.lm_head.dtype == torch.bfloat16
    return m8, m16


def _streams(model, M):
    """{projection: stream_gemm cfg} the model chooses at M rows."""
    L = model.layers[0]
    return {n: model._stream_choice(n[:-2], M, *getattr(L, n).shape)[0] for n in PROJ}


class _Calls:
    """Counts ops.stream_gemm calls of the model by weight type."""

    def __init__(self, monkeypatch):
        self.fp8 = self.bf16 = 0
        real = ops.stream_gemm

        def spy(x, w, *a, **k):
            if k.get("w_exps") is not None:
                assert w.dtype == torch.uint8
                self.fp8 += 1
            else:
                self.bf16 += 1
            return real(x, w, *a, **k)

        monkeypatch.setattr(llama.ops, "stream_gemm", spy)


def _prefill_meta(T, bt, bs):
    i32 = dict(dtype=torch.int32, device=DEV)
    return AttnMeta(decode=False, positions=torch.arange(T, **i32), slots=bt[0, 0].long() * bs + torch.arange(T, device=DEV),
                    block_tables=bt, ctx_lens=torch.tensor([T], **i32), cu_q=torch.tensor([0, T], **i32), max_q=T)


def _decode(model, B, seed):
    """Prefill B short prompts but their last token, then one decode step: (hidden, logits, K cache)."""
    bs, nbp = 64, 2
    i32 = dict(dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(50, 100, (B,), generator=g).tolist()  # (>= 3 x 49 prefill tokens: a GEMM step)
    prompts = [torch.randint(0, TOY.vocab_size, (n,), generator=g).tolist() for n in lens]
    kv = KVCache(TOY.layers, B * nbp, TOY.kv_heads, bs, TOY.head_dim, DEV)
    bt = torch.arange(B * nbp, **i32).view(B, nbp)
    # one packed prefill of every prompt's head (a GEMM step: the same bf16 copy in both models)
    ids = torch.tensor([t for p in prompts for t in p[:-1]], **i32)
    pos = torch.cat([torch.arange(len(p) - 1, **i32) for p in prompts])
    slots = torch.cat([bt[b, 0].long() * bs + torch.arange(len(p) - 1, device=DEV) for b, p in enumerate(prompts)])
    cu = torch.tensor([0] + torch.tensor([len(p) - 1 for p in prompts]).cumsum(0).tolist(), **i32)
    model.forward(ids, AttnMeta(decode=False, positions=pos, slots=slots, block_tables=bt,
                                ctx_lens=torch.tensor([len(p) - 1 for p in prompts], **i32), cu_q=cu,
                                max_q=max(lens) - 1), kv)
    dpos = torch.tensor([len(p) - 1 for p in prompts], **i32)
    ws = ops.DecodeWorkspace(B, TOY.heads, TOY.head_dim, nbp * bs // 512 + 1, DEV)
    meta = AttnMeta(decode=True, positions=dpos, slots=bt[:, 0].long() * bs + dpos.long(), block_tables=bt,
                    ctx_lens=dpos + 1, workspace=ws)
    h = model.forward(torch.tensor([p[-1] for p in prompts], **i32), meta, kv)
    return h, model.logits(h), kv.k


@pytest.mark.parametrize("B", [3, 40, 100, 130])
def test_model_decode_step_is_bit_equal(B, toy_models, monkeypatch):
    m8, m16 = toy_models
    cfgs = _streams(m8, B)
    nat = ops.native()
    # precondition: the projections stream, on FP8-capable configurations (at 129..256 rows gate_up
    # runs the mid-M GEMM by the model's dispatch -- on the bf16 copy of the same values)
    streamed = [n for n in PROJ if not (B > 128 and n == "gate_up_w")]
    assert all(cfgs[n] >= 0 and nat.stream_gemm_fp8_ok(cfgs[n]) for n in streamed), cfgs
    assert cfgs == _streams(m16, B)
    if 64 < B <= 128:
        assert cfgs["gate_up_w"] == LlamaModel.STREAM_WIDE["gate_up"]
    calls = _Calls(monkeypatch)
    got = _decode(m8, B, B)
    assert calls.fp8 == TOY.layers * len(streamed) and calls.bf16 == 1  # (+ the bf16 LM head)
    calls.fp8 = calls.bf16 = 0
    want = _decode(m16, B, B)
    assert calls.fp8 == 0 and calls.bf16 == TOY.layers * len(streamed) + 1
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert bool(got[0].float().abs().sum() > 0)


def test_model_small_batch_fused_norm_path_is_bit_equal(monkeypatch):
    """``_layer_small`` (consumer RMSNorm, residual producers on cfg 32) on the FP8 copies."""
    w = _toy_weights(8)
    m8 = LlamaModel(TOY, dict(w), DEV, interleaved_mlp=True, weight_dtype="fp8", small_norm_fused=True)
    m16 = LlamaModel(TOY, _dequantised(w), DEV, interleaved_mlp=True, small_norm_fused=True)
    calls = _Calls(monkeypatch)
    got = _decode(m8, 5, 1)
    assert calls.fp8 == TOY.layers * 4
    want = _decode(m16, 5, 1)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    m8.set_proj_group("qkv", 8)  # re-lays both copies in place
    m8.set_proj_group("gate_up", 1)
    assert m8.layers[0].qkv_w.group == 8 and m8.layers[0].gate_up_w.group == 1
    again = _decode(m8, 5, 1)
    for a, b in zip(again, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("T", [64, 300])
def test_model_prefill_is_bit_equal(T, toy_models, monkeypatch):
    """64 tokens: the streamed short-prefill path (FP8 copies); 300: the MFMA GEMMs (bf16 copies)."""
    m8, m16 = toy_models
    bs = 64
    nb = -(-T // bs)
    ids = torch.randint(0, TOY.vocab_size, (T,), generator=torch.Generator().manual_seed(T), dtype=torch.int32).to(DEV)
    bt = torch.arange(nb, dtype=torch.int32, device=DEV).view(1, nb)
    calls = _Calls(monkeypatch)
    out = []
    for m in (m8, m16):
        kv = KVCache(TOY.layers, nb, TOY.kv_heads, bs, TOY.head_dim, DEV)
        out.append((m.forward(ids, _prefill_meta(T, bt, bs), kv), kv.k, kv.v))
    if T <= LlamaModel.PREFILL_STREAM_MAX_M:
        cfgs = _streams(m8, T)
        assert all(c >= 0 and ops.native().stream_gemm_fp8_ok(c) for c in cfgs.values()), cfgs
        assert calls.fp8 == TOY.layers * 4 and calls.bf16 == TOY.layers * 4
    else:
        assert calls.fp8 == 0 and calls.bf16 == 0
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_model_mixed_step_is_bit_equal(toy_models):
    m8, m16 = toy_models
    bs, nbp = 64, 4
    i32 = dict(dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(2)
    dec = [torch.randint(0, 900, (n,), generator=g).tolist() for n in (40, 130, 77)]
    pre = [torch.randint(0, 900, (n,), generator=g).tolist() for n in (90, 33)]
    nd, npf = len(dec), len(pre)
    dbt = torch.arange(nd * nbp, **i32).view(nd, nbp)
    dpos = torch.tensor([len(p) - 1 for p in dec], **i32)
    pbt = torch.arange(nd * nbp, (nd + npf) * nbp, **i32).view(npf, nbp)
    ids = torch.tensor([t for p in pre for t in p] + [p[-1] for p in dec], **i32)
    pos = torch.cat([torch.arange(len(p), **i32) for p in pre] + [dpos])
    slots = torch.cat([pbt[i, 0].long() * bs + torch.arange(len(p), device=DEV) for i, p in enumerate(pre)]
                      + [dbt[:, 0].long() * bs + dpos.long()])
    out = []
    for m in (m8, m16):
        kv = KVCache(TOY.layers, (nd + npf) * nbp, TOY.kv_heads, bs, TOY.head_dim, DEV)
        for b, p in enumerate(dec):
            m.forward(torch.tensor(p[:-1], **i32), _prefill_meta(len(p) - 1, dbt[b:b + 1], bs), kv)
        ws = ops.DecodeWorkspace(8, TOY.heads, TOY.head_dim, nbp * bs // 512 + 1, DEV)
        meta = AttnMeta(decode=False, positions=pos, slots=slots, block_tables=pbt,
                        ctx_lens=torch.tensor([len(p) for p in pre], **i32),
                        cu_q=torch.tensor([0, len(pre[0]), len(pre[0]) + len(pre[1])], **i32), max_q=90, workspace=ws,
                        n_decode=nd, dec_block_tables=dbt, dec_ctx_lens=dpos + 1)
        out.append((m.forward(ids, meta, kv), kv.k))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_model_refuses_tensor_parallelism():
    with pytest.raises(ValueError, match="tensor parallelism"):
        LlamaModel(TOY, {}, DEV, weight_dtype="fp8", tp_size=2, tp_rank=0)


# ------------------------------------------------------------------------------------------------- engine


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_engine_greedy_tokens_equal_the_dequantised_engine(kv_dtype, monkeypatch):
    from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams

    w = _toy_weights(4)
    prompts = [list(range(10, 10 + n)) for n in (10, 77, 150, 300)]
    greedy = SamplingParams(max_new_tokens=24, do_sample=False, temperature=0.0, ignore_eos=True)
    calls = _Calls(monkeypatch)
    outs = {}
    for name, weights, wd, graphs in (("fp8_graphs", w, "fp8", True), ("fp8_eager", w, "fp8", False),
                                      ("dequantised", _dequantised(w), None, True)):
        eng = LLMEngine(TOY, device=DEV, weights=dict(weights), max_batch=8, block_size=64, num_blocks=64,
                        max_prefill_tokens=256, max_model_len=384, use_graphs=graphs, weight_dtype=wd,
                        kv_cache_dtype=kv_dtype)
        assert eng.weight_dtype == (wd or "bf16") and eng.stats["weight_bits"] == (8 if wd else 16)
        assert eng.stats["kv_cache_bits"] == (8 if kv_dtype == "fp8" else 16)
        calls.fp8 = 0
        rids = [eng.add_request(p, greedy) for p in prompts]
        while eng.has_unfinished():
            eng.step()
        outs[name] = [eng.pop_output(r).token_ids for r in rids]
        assert (eng.stats["graph_replays"] > 0) == graphs
        assert (calls.fp8 > 0) == (wd == "fp8")
    assert all(len(t) == 24 for t in outs["fp8_graphs"])
    assert outs["fp8_graphs"] == outs["fp8_eager"] == outs["dequantised"]
