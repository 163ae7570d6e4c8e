"""FP8 as the only weight copy on the GPU: ``LlamaModel(weight_dtype="fp8", fp8_weights_only=True)`` and
``LLMEngine(fp8_weights_only=True)`` on ``tiny-llama``.

The FP8-only model streams the FP8 bytes (stream_gemm's FP8 arm) and runs every other projection on the FP8 arm of
gemm256; both give, bit for bit, what the bf16 kernels give on the dequantised values.  So it must EQUAL the
two-copy FP8 model wherever that model's call lands on gemm256 or stream_gemm: the ``forced`` fixture sends every
MFMA call of the two-copy model to gemm256 (no gemm_mid, no 128 x 128 kernel), which makes that everywhere.  Against
the two-copy model's own dispatch the difference is accumulation order only: the tolerance tests/test_models_gpu.py
uses between the streamed and the GEMM step (atol 6e-2, rtol 5e-2)."""
import pytest
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams
from django_assistant_bot_amd.models.configs import DecoderConfig, decoder_config
from django_assistant_bot_amd.models.llama import AttnMeta, Fp8Proj, KVCache, LlamaModel
from django_assistant_bot_amd.models.weights import random_decoder_weights

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFG = decoder_config("tiny-llama")
PROJ = ("qkv_w", "o_w", "gate_up_w", "down_w")
TOL = dict(atol=6e-2, rtol=5e-2)
# the engine runs (FP8 KV cache included, whose GPU kernels take head_dim 128 only; tiny-llama's is 64): the toy
# decoder of tests/test_weight_fp8_gpu.py, every projection N % 256 == 0 and K % 128 == 0
TOY = DecoderConfig("toy-w8", vocab_size=1024, hidden=512, layers=2, heads=4, kv_heads=2, intermediate=896,
                    max_position=2048, bos_id=1000, eos_ids=(1001,), rope_scaling=None, rope_theta=10000.0)


def _weights(seed, cfg=CFG):
    return {k: v.to(torch.bfloat16) for k, v in random_decoder_weights(cfg, dtype=torch.float32, seed=seed,
                                                                       interleave_mlp=True).items()}


@pytest.fixture(scope="module")
def models():
    """(FP8-only model, two-copy FP8 model, allocated bytes of each) from the same weights."""
    w = _weights(6)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    m2 = LlamaModel(CFG, dict(w), DEV, interleaved_mlp=True, weight_dtype="fp8")
    two = torch.cuda.memory_allocated() - base
    m1 = LlamaModel(CFG, dict(w), DEV, interleaved_mlp=True, weight_dtype="fp8", fp8_weights_only=True)
    one = torch.cuda.memory_allocated() - base - two
    assert m1.frag and m2.frag and m1.proj_group == m2.proj_group
    return m1, m2, one, two


@pytest.fixture
def forced(monkeypatch):
    """Every MFMA call of a bf16 / two-copy model on gemm256."""
    monkeypatch.setattr(ops.kernels, "GEMM256_MIN_M", 1)
    monkeypatch.setattr(ops.kernels, "use_gemm_mid", lambda *a, **k: False)


def test_one_copy_and_its_bytes(models):
    m1, m2, one, two = models
    want = 0
    for L1, L2 in zip(m1.layers, m2.layers):
        for n in PROJ:
            p1, p2 = getattr(L1, n), getattr(L2, n)
            assert isinstance(p1, Fp8Proj) and p1.w is None and p2.w is not None
            assert p1.shape == p2.shape == p2.w.shape and p1.group == p2.group
            assert torch.equal(p1.data, p2.data) and torch.equal(p1.exps, p2.exps)
            N, K = p1.shape
            want += N * K + N
    assert m1.projection_bytes() == want
    assert m2.projection_bytes() == want + 2 * (want - sum(getattr(L, n).shape[0] for L in m1.layers for n in PROJ))
    bf16_layer = sum(2 * getattr(m2.layers[0], n).w.numel() for n in PROJ)
    assert one <= two - bf16_layer, (one, two, bf16_layer)
    assert m1.lm_head.dtype == torch.bfloat16 and m1.embed.dtype == torch.bfloat16


def _prefill_meta(T, bt, bs):
    i32 = dict(dtype=torch.int32, device=DEV)
    return AttnMeta(decode=False, positions=torch.arange(T, **i32), slots=bt[0, 0].long() * bs + torch.arange(T, device=DEV),
                    block_tables=bt, ctx_lens=torch.tensor([T], **i32), cu_q=torch.tensor([0, T], **i32), max_q=T)


def _decode(model, B, seed):
    """Prefill B short prompts but their last token, then one decode step: (hidden, logits, K cache)."""
    bs, nbp = 64, 2
    i32 = dict(dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(50, 100, (B,), generator=g).tolist()
    prompts = [torch.randint(0, CFG.vocab_size - 30, (n,), generator=g).tolist() for n in lens]
    kv = KVCache(CFG.layers, B * nbp, CFG.kv_heads, bs, CFG.head_dim, DEV)
    bt = torch.arange(B * nbp, **i32).view(B, nbp)
    ids = torch.tensor([t for p in prompts for t in p[:-1]], **i32)
    pos = torch.cat([torch.arange(len(p) - 1, **i32) for p in prompts])
    slots = torch.cat([bt[b, 0].long() * bs + torch.arange(len(p) - 1, device=DEV) for b, p in enumerate(prompts)])
    cu = torch.tensor([0] + torch.tensor([len(p) - 1 for p in prompts]).cumsum(0).tolist(), **i32)
    model.forward(ids, AttnMeta(decode=False, positions=pos, slots=slots, block_tables=bt,
                                ctx_lens=torch.tensor([len(p) - 1 for p in prompts], **i32), cu_q=cu,
                                max_q=max(lens) - 1), kv)
    dpos = torch.tensor([len(p) - 1 for p in prompts], **i32)
    ws = ops.DecodeWorkspace(B, CFG.heads, CFG.head_dim, nbp * bs // 512 + 1, DEV)
    meta = AttnMeta(decode=True, positions=dpos, slots=bt[:, 0].long() * bs + dpos.long(), block_tables=bt,
                    ctx_lens=dpos + 1, workspace=ws)
    h = model.forward(torch.tensor([p[-1] for p in prompts], **i32), meta, kv)
    return h, model.logits(h), kv.k


def _prefill(model, T, out_rows=None):
    bs = 64
    nb = -(-T // bs)
    ids = torch.randint(0, CFG.vocab_size - 30, (T,), generator=torch.Generator().manual_seed(T), dtype=torch.int32).to(DEV)
    bt = torch.arange(nb, dtype=torch.int32, device=DEV).view(1, nb)
    kv = KVCache(CFG.layers, nb, CFG.kv_heads, bs, CFG.head_dim, DEV)
    return model.forward(ids, _prefill_meta(T, bt, bs), kv, out_rows=out_rows), kv.k, kv.v


def _mixed(model):
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
    kv = KVCache(CFG.layers, (nd + npf) * nbp, CFG.kv_heads, bs, CFG.head_dim, DEV)
    for b, p in enumerate(dec):
        model.forward(torch.tensor(p[:-1], **i32), _prefill_meta(len(p) - 1, dbt[b:b + 1], bs), kv)
    ws = ops.DecodeWorkspace(8, CFG.heads, CFG.head_dim, nbp * bs // 512 + 1, DEV)
    meta = AttnMeta(decode=False, positions=pos, slots=slots, block_tables=pbt,
                    ctx_lens=torch.tensor([len(p) for p in pre], **i32),
                    cu_q=torch.tensor([0, len(pre[0]), len(pre[0]) + len(pre[1])], **i32), max_q=90, workspace=ws,
                    n_decode=nd, dec_block_tables=dbt, dec_ctx_lens=dpos + 1)
    return model.forward(ids, meta, kv), kv.k


def _equal(got, want):
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b)
    assert bool(got[0].float().abs().sum() > 0)


def _close(got, want):
    for a, b in zip(got, want):
        torch.testing.assert_close(a.float(), b.float(), **TOL)


@pytest.mark.parametrize("B", [3, 130])
def test_decode_step_equals_the_two_copy_model(B, models, forced):
    m1, m2, _, _ = models
    _equal(_decode(m1, B, B), _decode(m2, B, B))


@pytest.mark.parametrize("T", [64, 300, 1100])
def test_prefill_equals_the_two_copy_model(T, models, forced):
    m1, m2, _, _ = models
    _equal(_prefill(m1, T), _prefill(m2, T))


def test_mixed_step_equals_the_two_copy_model(models, forced):
    m1, m2, _, _ = models
    _equal(_mixed(m1), _mixed(m2))


def test_pruned_last_layer_tail_equals_the_two_copy_model(models, forced):
    """The tail on ``out_rows`` alone (gemm256 ``rows`` / ``as_m`` on the FP8 arm) equals the two-copy model's and the
    rows of the FP8-only model's own full step."""
    m1, m2, _, _ = models
    T = 1100
    rows = torch.tensor([1099, 3, 512, 3], device=DEV)
    h1 = _prefill(m1, T, out_rows=rows)
    full = _prefill(m1, T)
    _equal((h1[0],), (full[0][rows],))
    _equal(h1, _prefill(m2, T, out_rows=rows))
    assert m1._tail_prunable(300, _prefill_meta(300, torch.zeros((1, 5), dtype=torch.int32, device=DEV), 64), full[0], False)


@pytest.mark.parametrize("what", ["decode130", "prefill300", "mixed"])
def test_close_to_the_two_copy_models_own_dispatch(what, models):
    """Where the two-copy model takes gemm_mid or the 128 x 128 kernel the numbers differ in accumulation order."""
    m1, m2, _, _ = models
    run = {"decode130": lambda m: _decode(m, 130, 130), "prefill300": lambda m: _prefill(m, 300), "mixed": _mixed}[what]
    _close(run(m1), run(m2))


def test_never_reaches_gemm_mid_or_the_128_kernel(models, monkeypatch):
    m1 = models[0]
    nat = ops.native()
    for name in ("gemm_mid", "gemm_bt", "gemm256"):  # (the LM head streams at these row counts)
        monkeypatch.setattr(nat, name, lambda *a, **k: pytest.fail("a bf16 MFMA kernel was launched"))
    arm = []
    real = nat.gemm256_fp8
    monkeypatch.setattr(nat, "gemm256_fp8", lambda *a, **k: arm.append(1) or real(*a, **k))
    _prefill(m1, 300)
    assert len(arm) == 4 * CFG.layers
    _mixed(m1)
    assert len(arm) >= 8 * CFG.layers
    n = len(arm)
    _decode(m1, 130, 1)  # (its 130-prompt prefill: 4 per layer; the step: gate_up, the others stream)
    assert len(arm) >= n + 5 * CFG.layers


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_engine_greedy_tokens_equal_the_two_copy_engine(kv_dtype, forced):
    w = _weights(4, TOY)
    prompts = [list(range(10, 10 + n)) for n in (10, 77, 150, 300)]
    greedy = SamplingParams(max_new_tokens=24, do_sample=False, temperature=0.0, ignore_eos=True)
    outs, stats = {}, {}
    for only in (True, False):
        eng = LLMEngine(TOY, device=DEV, weights=dict(w), max_batch=8, block_size=64, num_blocks=64,
                        max_prefill_tokens=256, max_model_len=384, use_graphs=True, weight_dtype="fp8",
                        kv_cache_dtype=kv_dtype, fp8_weights_only=only)
        assert eng.fp8_weights_only == only and eng.model.fp8_weights_only == only
        rids = [eng.add_request(p, greedy) for p in prompts]
        while eng.has_unfinished():
            eng.step()
        outs[only] = [eng.pop_output(r).token_ids for r in rids]
        stats[only] = dict(eng.stats)
        assert eng.stats["graph_replays"] > 0
    assert all(len(t) == 24 for t in outs[True]) and outs[True] == outs[False]
    nk = sum(N * K + N for N, K in (getattr(eng.model.layers[0], n).shape for n in PROJ)) * TOY.layers
    assert stats[True]["weight_bf16_copy"] is False and stats[False]["weight_bf16_copy"] is True
    assert stats[True]["weight_bytes"] == nk and stats[False]["weight_bytes"] > 2 * nk
    assert stats[True]["weight_bits"] == 8


def test_refusals():
    w = _weights(1)
    with pytest.raises(ValueError, match="weight_dtype='fp8'"):
        LlamaModel(CFG, dict(w), DEV, interleaved_mlp=True, fp8_weights_only=True)
    with pytest.raises(ValueError, match="tensor parallelism"):
        LlamaModel(CFG, dict(w), DEV, interleaved_mlp=True, weight_dtype="fp8", fp8_weights_only=True, tp_size=2, tp_rank=0)
    with pytest.raises(ValueError, match="fragment"):
        LlamaModel(CFG, dict(w), DEV, interleaved_mlp=True, weight_dtype="fp8", fp8_weights_only=True,
                   fragment_layout=False)
    odd = DecoderConfig("toy-odd", vocab_size=1024, hidden=384, layers=1, heads=3, kv_heads=1, intermediate=512,
                        max_position=2048, bos_id=1000, eos_ids=(1001,), rope_scaling=None, rope_theta=10000.0)
    wo = _weights(1, odd)
    assert LlamaModel(odd, dict(wo), DEV, interleaved_mlp=True, weight_dtype="fp8").frag  # the two-copy model takes it
    with pytest.raises(ValueError, match="N % 256"):
        LlamaModel(odd, dict(wo), DEV, interleaved_mlp=True, weight_dtype="fp8", fp8_weights_only=True)
    with pytest.raises(ValueError, match="weight_dtype='fp8'"):
        LLMEngine(CFG, device=DEV, weights=dict(w), num_blocks=8, fp8_weights_only=True)
    with pytest.raises(ValueError, match="tensor parallelism"):
        LLMEngine(CFG, device=DEV, weights=dict(w), num_blocks=8, weight_dtype="fp8", fp8_weights_only=True, tp_size=2)

    class NoStream(LlamaModel):
        fp8_stream = False

    with pytest.raises(ValueError, match="fp8_stream"):
        NoStream(CFG, dict(w), DEV, interleaved_mlp=True, weight_dtype="fp8", fp8_weights_only=True)
