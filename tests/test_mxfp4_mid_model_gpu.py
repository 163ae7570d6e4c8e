"""``mxfp4_mid`` in the model and the engine on the GPU: gemm_mid calls of an MXFP4 decoder read the codes
on the kernel's MXFP4 arm instead of a bf16 copy (or, in the one-copy mode, of the dequantiser's scratch
image).  The arm is bit-equal to the bf16 kernel, so four models from the same weights -- {one copy, two
copies} x {flag off, on} -- must agree bit for bit in every step kind, and the spy pins which launches
changed.  The toy decoder and the spy are those of tests/test_weight_mxfp4_only_gpu.py."""
import pytest
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.models.configs import DecoderConfig
from django_assistant_bot_amd.models.llama import AttnMeta, KVCache, LlamaModel, Mxfp4Proj
from django_assistant_bot_amd.models.weights import random_decoder_weights

pytestmark = pytest.mark.gpu

DEV = "cuda"
# qkv [1024, 512], o [512, 512], gate_up [1792, 512], down [512, 896]; every N % 256 == 0 and K % 128 == 0
TOY = DecoderConfig("toy-w4", vocab_size=1024, hidden=512, layers=2, heads=4, kv_heads=2, intermediate=896,
                    max_position=2048, bos_id=1000, eos_ids=(1001,), rope_scaling=None, rope_theta=10000.0)
NATIVE = ("gemm_bt", "gemm256", "gemm_mid", "gemm_mid_mxfp4", "stream_gemm", "stream_gemm_mxfp4", "weight_dequant_mxfp4")
L = TOY.layers


def _toy_weights(seed):
    return {k: v.to(torch.bfloat16) for k, v in random_decoder_weights(TOY, dtype=torch.float32, seed=seed,
                                                                       interleave_mlp=True).items()}


@pytest.fixture(scope="module")
def models():
    """{(one copy?, mxfp4_mid?): model} from the same weights."""
    w = _toy_weights(6)
    out = {(only, mid): LlamaModel(TOY, dict(w), DEV, interleaved_mlp=True, weight_dtype="mxfp4", mxfp4_weights_only=only,
                                   mxfp4_mid=mid) for only in (True, False) for mid in (False, True)}
    for (only, mid), m in out.items():
        assert m.frag and m.mxfp4_mid == mid and m.mxfp4_weights_only == only and m.proj_group["gate_up"] == 8
        p = m.layers[0].gate_up_w
        assert isinstance(p, Mxfp4Proj) and (p.w is None) == only
    return out


class _Spy:
    """Counts the native GEMM entry points and the dequantiser by name."""

    def __init__(self, monkeypatch):
        self.n = {}
        nat = ops.native()
        for name in NATIVE:
            monkeypatch.setattr(nat, name, self._wrap(name, getattr(nat, name)))

    def _wrap(self, name, real):
        def f(*a, **k):
            self.n[name] = self.n.get(name, 0) + 1
            return real(*a, **k)
        return f

    def take(self):
        n, self.n = self.n, {}
        return n


def _prefill_meta(lens, bt, bs):
    i32 = dict(dtype=torch.int32, device=DEV)
    pos = torch.cat([torch.arange(n, **i32) for n in lens])
    slots = torch.cat([bt[i, 0].long() * bs + torch.arange(n, device=DEV) for i, n in enumerate(lens)])
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), **i32)
    return AttnMeta(decode=False, positions=pos, slots=slots, block_tables=bt, ctx_lens=torch.tensor(lens, **i32),
                    cu_q=cu, max_q=max(lens))


def _prefill(model, lens):
    bs = 64
    nbp = -(-max(lens) // bs)
    T = sum(lens)
    ids = torch.randint(0, TOY.vocab_size, (T,), generator=torch.Generator().manual_seed(T), dtype=torch.int32).to(DEV)
    bt = torch.arange(len(lens) * nbp, dtype=torch.int32, device=DEV).view(len(lens), nbp)
    kv = KVCache(TOY.layers, len(lens) * nbp, TOY.kv_heads, bs, TOY.head_dim, DEV)
    h = model.forward(ids, _prefill_meta(lens, bt, bs), kv)
    return h, kv.k, kv.v


def _decode_setup(model, B, seed):
    """Prefill B short prompts but their last token: (last tokens, decode meta, cache)."""
    bs, nbp = 64, 1
    i32 = dict(dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(20, 60, (B,), generator=g).tolist()
    prompts = [torch.randint(0, TOY.vocab_size, (n,), generator=g).tolist() for n in lens]
    kv = KVCache(TOY.layers, B * nbp, TOY.kv_heads, bs, TOY.head_dim, DEV)
    bt = torch.arange(B * nbp, **i32).view(B, nbp)
    ids = torch.tensor([t for p in prompts for t in p[:-1]], **i32)
    model.forward(ids, _prefill_meta([n - 1 for n in lens], bt, bs), kv)
    dpos = torch.tensor([n - 1 for n in lens], **i32)
    ws = ops.DecodeWorkspace(B, TOY.heads, TOY.head_dim, nbp * bs // 512 + 1, DEV)
    meta = AttnMeta(decode=True, positions=dpos, slots=bt[:, 0].long() * bs + dpos.long(), block_tables=bt,
                    ctx_lens=dpos + 1, workspace=ws)
    return torch.tensor([p[-1] for p in prompts], **i32), meta, kv


def _decode(model, B, spy=None):
    last, meta, kv = _decode_setup(model, B, B)
    if spy is not None:
        spy.take()  # (the counts are those of the decode step alone)
    h = model.forward(last, meta, kv)
    return h, model.logits(h), kv.k, kv.v


def _mixed(model):
    """Warm-up prefills of 39 / 129 / 76 tokens, then a 126-token mixed step (123 prefill rows + 3 decode rows)."""
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
    kv = KVCache(TOY.layers, (nd + npf) * nbp, TOY.kv_heads, bs, TOY.head_dim, DEV)
    for b, p in enumerate(dec):
        model.forward(torch.tensor(p[:-1], **i32), _prefill_meta([len(p) - 1], dbt[b:b + 1], bs), kv)
    ws = ops.DecodeWorkspace(8, TOY.heads, TOY.head_dim, nbp * bs // 512 + 1, DEV)
    meta = AttnMeta(decode=False, positions=pos, slots=slots, block_tables=pbt,
                    ctx_lens=torch.tensor([len(p) for p in pre], **i32),
                    cu_q=torch.tensor([0, len(pre[0]), len(pre[0]) + len(pre[1])], **i32), max_q=90, workspace=ws,
                    n_decode=nd, dec_block_tables=dbt, dec_ctx_lens=dpos + 1)
    h = model.forward(ids, meta, kv)
    return h, kv.k, kv.v


def _all_four(models, spy, fn):
    """fn(model) on the four models: asserts bit-equal tensors; -> {(only, mid): launch counts}."""
    outs, counts = {}, {}
    for key, m in models.items():
        spy.take()
        outs[key] = fn(m)
        counts[key] = spy.take()
    base = outs[(False, False)]
    assert bool(base[0].float().abs().sum() > 0)
    for key, got in outs.items():
        assert len(got) == len(base)
        for a, b in zip(got, base):
            assert a.shape == b.shape and torch.equal(a, b), key
    return counts


def _renamed(n):
    """The flag-off counts as the flag-on model must show them: gemm_mid -> gemm_mid_mxfp4, and no dequantiser
    launch for those calls."""
    n = dict(n)
    mid = n.pop("gemm_mid", 0)
    if mid:
        n["gemm_mid_mxfp4"] = mid
        if "weight_dequant_mxfp4" in n:
            n["weight_dequant_mxfp4"] -= mid
            if not n["weight_dequant_mxfp4"]:
                del n["weight_dequant_mxfp4"]
    return n


def test_prefill_300_is_bit_equal_and_reads_the_codes(models, monkeypatch):
    spy = _Spy(monkeypatch)
    c = _all_four(models, spy, lambda m: _prefill(m, [300]))
    assert c[(False, False)] == {"gemm_mid": 4 * L}
    assert c[(True, False)] == {"gemm_mid": 4 * L, "weight_dequant_mxfp4": 4 * L}
    assert c[(False, True)] == c[(True, True)] == {"gemm_mid_mxfp4": 4 * L}  # zero dequantiser launches


def test_decode_200_is_bit_equal_and_reads_the_codes(models, monkeypatch):
    spy = _Spy(monkeypatch)
    c = _all_four(models, spy, lambda m: _decode(m, 200, spy))
    off = {"stream_gemm_mxfp4": 3 * L, "gemm_mid": L, "stream_gemm": 1}
    on = {"stream_gemm_mxfp4": 3 * L, "gemm_mid_mxfp4": L, "stream_gemm": 1}
    assert c[(False, False)] == off and c[(True, False)] == dict(off, weight_dequant_mxfp4=L)
    assert c[(False, True)] == c[(True, True)] == on  # zero dequantiser launches


def test_mixed_step_is_bit_equal(models, monkeypatch):
    spy = _Spy(monkeypatch)
    c = _all_four(models, spy, _mixed)
    assert c[(False, False)].get("gemm_mid", 0) > 0
    for only in (False, True):
        assert c[(only, True)] == _renamed(c[(only, False)]), only


@pytest.mark.parametrize("lens,fam", [([64], "stream_gemm_mxfp4"), ([1400, 1400, 1400], "gemm256")])
def test_other_kernel_families_keep_their_launches(lens, fam, models, monkeypatch):
    spy = _Spy(monkeypatch)
    c = _all_four(models, spy, lambda m: _prefill(m, lens))
    assert c[(False, False)] == {fam: 4 * L}
    for only in (False, True):
        assert c[(only, True)] == c[(only, False)]
        assert "gemm_mid_mxfp4" not in c[(only, True)]


def test_opt_out_keeps_the_bf16_path(models, monkeypatch):
    m = models[(True, True)]
    monkeypatch.setattr(m, "MXFP4_MID_OFF", frozenset({"gate_up", "o"}))
    spy = _Spy(monkeypatch)
    got = _prefill(m, [300])
    n = spy.take()
    assert n == {"gemm_mid_mxfp4": 2 * L, "gemm_mid": 2 * L, "weight_dequant_mxfp4": 2 * L}
    monkeypatch.undo()
    for a, b in zip(got, _prefill(models[(False, False)], [300])):
        assert torch.equal(a, b)


def test_decode_200_captured_into_a_graph_equals_the_eager_step(models):
    m = models[(True, True)]
    last, meta, kv = _decode_setup(m, 200, 200)
    want = m.forward(last, meta, kv)
    want_logits = m.logits(want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream: its workspaces exist before the capture
        m.logits(m.forward(last, meta, kv))
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        h = m.forward(last, meta, kv)
        lg = m.logits(h)
    for _ in range(2):
        h.zero_()
        lg.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(h, want) and torch.equal(lg, want_logits)


# ------------------------------------------------------------------------------------------------- engine

PROMPTS_1 = [list(range(10, 10 + n)) for n in (10, 77, 150)]
PROMPTS_2 = [list(range(40, 40 + n)) for n in (300, 21)]


def _engine(weights, **kw):
    from django_assistant_bot_amd.engine.llm_engine import LLMEngine

    args = dict(device=DEV, weights=dict(weights), max_batch=8, block_size=64, num_blocks=64, max_prefill_tokens=256,
                max_model_len=384, use_graphs=True, weight_dtype="mxfp4")
    if "shared_model" in kw:
        del args["weights"], args["weight_dtype"]
    args.update(kw)
    return LLMEngine(TOY, **args)


def _two_waves(eng):
    from django_assistant_bot_amd.engine.llm_engine import SamplingParams

    greedy = SamplingParams(max_new_tokens=20, do_sample=False, temperature=0.0, ignore_eos=True)
    rids = [eng.add_request(p, greedy) for p in PROMPTS_1]
    while eng.stats["graph_replays"] < 4:
        eng.step()
    rids += [eng.add_request(p, greedy) for p in PROMPTS_2]
    while eng.has_unfinished():
        eng.step()
    return [eng.pop_output(r).token_ids for r in rids]


def test_engine_greedy_tokens_equal_the_flag_off_engine(monkeypatch):
    w = _toy_weights(4)
    spy = _Spy(monkeypatch)
    outs, counts = {}, {}
    for mid in (True, False):
        eng = _engine(w, mxfp4_weights_only=True, mxfp4_mid=mid)
        assert eng.mxfp4_mid == mid == eng.model.mxfp4_mid and eng.stats["weight_mid_mxfp4"] is mid
        assert eng.stats["weight_bf16_copy"] is False
        spy.take()
        outs[mid] = _two_waves(eng)
        counts[mid] = spy.take()
    assert all(len(t) == 20 for t in outs[True]) and outs[True] == outs[False]
    assert counts[False].get("gemm_mid", 0) > 0 and "gemm_mid_mxfp4" not in counts[False]
    assert counts[True] == _renamed(counts[False])


def test_engine_shared_model_adopts_the_flag_and_a_conflict_raises():
    w = _toy_weights(4)
    e1 = _engine(w, mxfp4_mid=True)
    e2 = _engine(w, shared_model=e1.model)
    assert e2.mxfp4_mid and e2.stats["weight_mid_mxfp4"] is True and e2.stats["weight_bf16_copy"] is True
    with pytest.raises(ValueError, match="mxfp4_mid=False conflicts"):
        _engine(w, shared_model=e1.model, mxfp4_mid=False)
    with pytest.raises(ValueError, match="mxfp4_mid needs weight_dtype='mxfp4'"):
        _engine(w, weight_dtype="bf16", mxfp4_mid=True)
