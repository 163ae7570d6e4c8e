"""``out_rows`` / ``rows`` on CPU tensors: the reference path computes all rows and selects."""
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams
from django_assistant_bot_amd.models import decoder_config, random_decoder_weights
from django_assistant_bot_amd.models.llama import AttnMeta, KVCache, LlamaModel


def _model():
    cfg = decoder_config("tiny-llama")
    w = {k: v.float() for k, v in random_decoder_weights(cfg, dtype=torch.float32, seed=3).items()}
    return cfg, LlamaModel(cfg, w, "cpu")


def _prefill(cfg, lens):
    bs = 16
    nblk = [-(-n // bs) for n in lens]
    bt = torch.zeros((len(lens), max(nblk)), dtype=torch.int32)
    o = 0
    for b, nb in enumerate(nblk):
        bt[b, :nb] = torch.arange(o, o + nb, dtype=torch.int32)
        o += nb
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens])
    slots = torch.cat([bt[b, torch.arange(n) // bs].long() * bs + torch.arange(n) % bs for b, n in enumerate(lens)])
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
    ids = torch.randint(0, cfg.vocab_size, (sum(lens),), generator=torch.Generator().manual_seed(0)).to(torch.int32)
    meta = AttnMeta(decode=False, positions=pos, slots=slots, block_tables=bt,
                    ctx_lens=torch.tensor(lens, dtype=torch.int32), cu_q=cu, max_q=max(lens))
    return ids, meta, lambda: KVCache(cfg.layers, sum(nblk), cfg.kv_heads, bs, cfg.head_dim, "cpu", dtype=torch.float32)


def test_forward_out_rows_returns_the_reference_rows():
    cfg, m = _model()
    ids, meta, new_kv = _prefill(cfg, [20, 9, 33])
    kv_full, h_full = new_kv(), None
    h_full = m.forward(ids, meta, kv_full)
    for rows, dtype in (([19, 28, 61], torch.int32), ([40], torch.int64), ([], torch.int32)):
        r = torch.tensor(rows, dtype=dtype)
        kv = new_kv()
        h = m.forward(ids, meta, kv, out_rows=r)
        assert h.shape == (len(rows), cfg.hidden)
        assert torch.equal(h, h_full[r.long()])
        assert torch.equal(kv.k, kv_full.k) and torch.equal(kv.v, kv_full.v)


def test_gemm_bt_rows_on_cpu_tensors():
    g = torch.Generator().manual_seed(1)
    A, W, R = torch.randn(40, 64, generator=g), torch.randn(32, 64, generator=g), torch.randn(40, 32, generator=g)
    r = torch.tensor([39, 0, 7, 7], dtype=torch.int32)
    assert torch.equal(ops.gemm_bt(A, W, residual=R, rows=r), ops.gemm_bt(A, W, residual=R)[r.long()])
    assert torch.equal(ops.gemm_bt(A[:3], W, as_m=40), ops.gemm_bt(A[:3], W))


def test_engine_tokens_equal_with_the_switch_on_and_off():
    cfg = decoder_config("tiny-llama")
    w = {k: v.float() for k, v in random_decoder_weights(cfg, dtype=torch.float32, seed=3).items()}
    greedy = SamplingParams(max_new_tokens=8, do_sample=False, temperature=0.0, ignore_eos=True)
    prompts = [list(range(5, 5 + n)) for n in (20, 37, 300)]  # 300 > the prefill budget: a chunk without a last row
    out = {}
    for on in (True, False):
        LlamaModel.prune_last_tail = on
        try:
            eng = LLMEngine(cfg, device="cpu", weights=dict(w), max_batch=8, block_size=16, num_blocks=64,
                            max_prefill_tokens=256, use_graphs=False)
            out[on] = [o.token_ids for o in eng.generate(prompts, greedy)]
        finally:
            LlamaModel.prune_last_tail = True
    assert out[True] == out[False] and all(len(t) == 8 for t in out[True])
