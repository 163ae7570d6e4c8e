"""Llama-3-8B model step times with ``mxfp4_mid`` off and on, in both MXFP4 weight modes (two copies, one
copy): the step table of profiles/gemm_mid_mxfp4.md (the rows of profiles/weight_mxfp4_only.md section 3
that reach ``gemm_mid``).

``model.forward`` + ``model.logits`` on the engine's model and cache.  Prefill: one packed sequence of T
tokens, logits of its last token, median of 5 eager steps after 2 warm-up steps.  Decode: B sequences with
1100-token contexts, one step captured into a HIP graph, median of 7 replays.  First token: a 200-token
prompt through ``LLMEngine`` with ``max_new_tokens=1``, host included, median of 5.  One model per weight
mode; the flag is switched on that model, the arms alternating round by round.  One JSON line per
(weight mode, step, flag) with the median over the rounds and the min / max of every sample.

    python benchmarks/mxfp4_mid_steps.py [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from django_assistant_bot_amd import ops  # noqa: E402
from django_assistant_bot_amd.engine.llm_engine import LLMEngine, SamplingParams  # noqa: E402
from django_assistant_bot_amd.models.llama import AttnMeta  # noqa: E402

DEV = "cuda"
BS = 64


def prefill_samples(eng, T, n=5, warm=2):
    m, cfg = eng.model, eng.cfg
    i32 = dict(dtype=torch.int32, device=DEV)
    nb = -(-T // BS)
    ids = torch.randint(0, cfg.vocab_size, (T,), generator=torch.Generator().manual_seed(T), dtype=torch.int32).to(DEV)
    bt = torch.arange(nb, **i32).view(1, nb)
    meta = AttnMeta(decode=False, positions=torch.arange(T, **i32), slots=torch.arange(T, device=DEV),
                    block_tables=bt, ctx_lens=torch.tensor([T], **i32), cu_q=torch.tensor([0, T], **i32), max_q=T)
    rows = torch.tensor([T - 1], **i32)
    out = []
    for i in range(warm + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.logits(m.forward(ids, meta, eng.kv, out_rows=rows))
        torch.cuda.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def decode_samples(eng, B, ctx=1100, n=7):
    m, cfg = eng.model, eng.cfg
    i32 = dict(dtype=torch.int32, device=DEV)
    nbp = -(-ctx // BS)
    bt = torch.arange(B * nbp, **i32).view(B, nbp)
    pos = torch.full((B,), ctx - 1, **i32)
    ws = ops.DecodeWorkspace(B, cfg.heads, cfg.head_dim, nbp * BS // 512 + 1, DEV)
    meta = AttnMeta(decode=True, positions=pos, slots=bt[:, -1].long() * BS + (ctx - 1) % BS, block_tables=bt,
                    ctx_lens=pos + 1, workspace=ws)
    ids = torch.randint(0, cfg.vocab_size, (B,), generator=torch.Generator().manual_seed(B), dtype=torch.int32).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.logits(m.forward(ids, meta, eng.kv))
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        m.logits(m.forward(ids, meta, eng.kv))
    g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    del g
    return out


def first_token_samples(eng, n=5, warm=2):
    sp = SamplingParams(max_new_tokens=1, do_sample=False, temperature=0.0, ignore_eos=True)
    out = []
    for i in range(warm + n):
        prompt = [(7 * i + 3 * j) % 120000 + 5 for j in range(200)]  # (a fresh prompt: no prefix-cache hit)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rid = eng.add_request(prompt, sp)
        while eng.has_unfinished():
            eng.step()
        torch.cuda.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
        eng.pop_output(rid)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    steps = [("prefill T=384", lambda e: prefill_samples(e, 384)), ("prefill T=1024", lambda e: prefill_samples(e, 1024)),
             ("decode B=192", lambda e: decode_samples(e, 192)), ("decode B=256", lambda e: decode_samples(e, 256)),
             ("first token, 200-token prompt", first_token_samples)]
    for only in (False, True):
        eng = LLMEngine("llama-3-8b", device=DEV, max_batch=256, kv_cache_gb=48, max_prefill_tokens=32768, block_size=BS,
                        weight_dtype="mxfp4", mxfp4_weights_only=only, mxfp4_mid=False)
        for name, fn in steps:
            samples = {False: [], True: []}
            for _ in range(args.rounds):
                for mid in (False, True):
                    eng.model.mxfp4_mid = mid
                    eng._graphs.clear()
                    samples[mid].append(fn(eng))
            for mid in (False, True):
                meds = [statistics.median(s) for s in samples[mid]]
                flat = [x for s in samples[mid] for x in s]
                print(json.dumps({"weights": "one copy" if only else "two copies", "step": name, "mxfp4_mid": mid,
                                  "ms": round(statistics.median(meds), 3), "min": round(min(flat), 3),
                                  "max": round(max(flat), 3), "round_medians": [round(x, 3) for x in meds]}), flush=True)
        eng.model.mxfp4_mid = False
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
