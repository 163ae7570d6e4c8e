"""A decoder whose output names the token it read (shared by tests/test_copy_decoder_{cpu,gpu}.py).

The weights are constructed, not drawn.  Layer l's attention (one query head, its KV head) copies a 10-bit
token code from position ``p - j_l``; the MLP carries the code on, so gate_up, SwiGLU8 and down lie on the
path; the LM head reads the code back.  With offsets (j0, j1) and J = j0 + j1 the argmax of row p of any
forward is ``seq[p - J]`` and greedy generation continues any prompt as ``x[n] = x[n - 1 - J]``: no
reference run is needed and there are no near-ties.  A decode position off by one, a context length short
by one, a token written to the neighbouring slot, a layer reading another layer's cache, a block-table row
of another sequence: each gives a WRONG TOKEN, not a small error.

Residual subspaces (every entry is +-1 where it is set, so the RMSNorm factor at each point is known:
``sqrt(512 / ones)`` with ones = 11, 21, 31, 41 and 51 at the final norm):

    E   = dims 0..9    the token's 10-bit code as +-1        C = dim 10   the constant 1
    A_0 = dims 16..25  layer 0 attention output               M_0 = dims 32..41  layer 0 MLP output
    A_1 = dims 48..57  layer 1 attention output               M_1 = dims 64..73  layer 1 MLP output

Attention of layer l (query head ``head``, KV head ``head // 2``; rotate-half RoPE holds pair i at dims
(i, i + 64)): K reads C into ``qa`` on dims i < NF, Q reads C into ``qa cos(j_l th_i)`` on dim i and
``-qa sin(j_l th_i)`` on dim i + 64, so after RoPE ``score(p, s) = qa^2 sum_i cos((p - j_l - s) th_i) /
sqrt(128)``, which peaks at ``s = p - j_l``.  V copies the source subspace (E for layer 0, M_0 for layer 1)
into its dims 0..9, o_w copies them into A_l.  MLP: gate row f reads C into G, up row f reads A_l[b], down
maps f to M_l[b] with 1 / G; the ten f = 37 b + 5 lie in different 8-row [gate | up] groups.

The builder's conditions (``check_gap``, ``prompt``) are conditions, not measurements: they are evaluated
in fp64 on the stored (bf16-rounded, or quantised) values and every case of both test modules asserts them.
"""
from __future__ import annotations

import math
import zlib

import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.models.configs import DecoderConfig
from django_assistant_bot_amd.models.llama import AttnMeta, KVCache, LlamaModel
from django_assistant_bot_amd.models.weights import _gate_up
from django_assistant_bot_amd.ops import reference as ref

# the toy of tests/test_weight_mxfp4_gpu.py: every projection streams, FP8 KV is allowed (D = 128), every
# N is a multiple of 256 and every K of 128
CFG = DecoderConfig("copy-toy", vocab_size=1024, hidden=512, layers=2, heads=4, kv_heads=2, intermediate=896,
                    max_position=2048, bos_id=1000, eos_ids=(1001,), rope_scaling=None, rope_theta=10000.0)
D = CFG.head_dim
BS = 64  # KV block size of every model-level case
BITS = 10
E, C = tuple(range(0, 10)), 10
A = (tuple(range(16, 26)), tuple(range(48, 58)))
M = (tuple(range(32, 42)), tuple(range(64, 74)))
ONES = ((11, 21), (31, 41))  # +-1 entries of the residual at layer l's (attention norm, MLP norm)
QA, G, NF = 16.0, 16.0, 24
WRONG = 1023  # the token whose code the anti-needles carry; no prompt holds it
ANTI_GAIN = 1.25  # an anti-needle's K is this much longer than a real key: where it is read, it wins


def codes() -> torch.Tensor:
    """[1024, 10] fp64: bit b of token v as +-1."""
    v = torch.arange(CFG.vocab_size)
    return (((v[:, None] >> torch.arange(BITS)[None]) & 1) * 2 - 1).double()


def _inv_freq() -> torch.Tensor:
    return ref.llama3_inv_freq(D, CFG.rope_theta, CFG.rope_scaling).double()


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).double()


def _gain(target: float, r: float) -> float:
    """The weight that turns the normalised +-r (as the norm stores it, a bf16) into ``target``."""
    return target / float(_bf(torch.tensor(r, dtype=torch.float64)))


def build(offsets=(0, 1), head: int = 1, sharp: float = 1.0, qa: float = QA, gate: float = G, nf: int = NF,
          mlp_group: int = 8) -> dict:
    """bf16 weights under the keys of ``random_decoder_weights(CFG, interleave_mlp=True)``.  ``mlp_group``
    other than 8 is the planted interleave mistake of the CPU module."""
    H, F = CFG.hidden, CFG.intermediate
    kvh = head // (CFG.heads // CFG.kv_heads)
    th = _inv_freq()
    code = codes()
    w = {"embed": torch.zeros((CFG.vocab_size, H), dtype=torch.float64), "final_norm": torch.ones(H, dtype=torch.float64),
         "lm_head": torch.zeros((CFG.vocab_size, H), dtype=torch.float64)}
    w["embed"][:, list(E)] = code
    w["embed"][:, C] = 1.0
    w["lm_head"][:, list(M[-1])] = sharp * code
    fs = [37 * b + 5 for b in range(BITS)]
    assert len({f // 8 for f in fs}) == BITS and max(fs) < F
    for l, j in enumerate(offsets):
        ra, rm = math.sqrt(H / ONES[l][0]), math.sqrt(H / ONES[l][1])
        qkv = torch.zeros(((CFG.heads + 2 * CFG.kv_heads) * D, H), dtype=torch.float64)
        i = torch.arange(nf)
        qkv[head * D + i, C] = _gain(qa, ra) * torch.cos(j * th[:nf])
        qkv[head * D + D // 2 + i, C] = -_gain(qa, ra) * torch.sin(j * th[:nf])
        qkv[(CFG.heads + kvh) * D + i, C] = _gain(qa, ra)
        src = E if l == 0 else M[l - 1]
        for b in range(BITS):
            qkv[(CFG.heads + CFG.kv_heads + kvh) * D + b, src[b]] = _gain(1.0, ra)
        o = torch.zeros((H, CFG.heads * D), dtype=torch.float64)
        for b in range(BITS):
            o[A[l][b], head * D + b] = 1.0
        gt, up = torch.zeros((F, H), dtype=torch.float64), torch.zeros((F, H), dtype=torch.float64)
        down = torch.zeros((H, F), dtype=torch.float64)
        for b, f in enumerate(fs):
            gt[f, C] = _gain(gate, rm)
            up[f, A[l][b]] = _gain(1.0, rm)
            down[M[l][b], f] = 1.0 / gate
        w[f"l{l}.attn_norm"] = torch.ones(H, dtype=torch.float64)
        w[f"l{l}.mlp_norm"] = torch.ones(H, dtype=torch.float64)
        w[f"l{l}.qkv_w"], w[f"l{l}.o_w"] = qkv, o
        w[f"l{l}.gate_up_w"], w[f"l{l}.down_w"] = _gate_up(gt, up, mlp_group), down
    return {k: v.to(torch.bfloat16).contiguous() for k, v in w.items()}


PROJ = ("qkv_w", "o_w", "gate_up_w", "down_w")


def arm_weights(w: dict, weight_dtype: str = "bf16") -> dict:
    """The values a ``weight_dtype`` model computes with: the projections through the quantiser and back."""
    if weight_dtype == "bf16":
        return dict(w)
    out = dict(w)
    for k, v in w.items():
        if k.endswith(PROJ):
            if weight_dtype == "fp8":
                out[k] = ops.weight_dequantize_fp8(*ops.weight_quantize_fp8(v))
            else:
                out[k] = ops.weight_dequantize_mxfp4(*ops.weight_quantize_mxfp4(v))
    return out


# ------------------------------------------------------------------------------------- expected tokens


def expected_rows(seq, J: int) -> list:
    """[(row p, expected argmax)] of a full forward over ``seq``: every row p >= J."""
    return [(p, seq[p - J]) for p in range(J, len(seq))]


def expected_continuation(prompt, J: int, n: int) -> list:
    x = list(prompt)
    assert len(x) >= J + 1, "a prompt is at least J + 1 long"
    for _ in range(n):
        x.append(x[len(x) - 1 - J])
    return x[len(prompt):]


def prompt(key, n: int, J: int, new: int = 0, prefix=()) -> list:
    """A decisive prompt of n tokens (the first of them ``prefix``) for case ``key``: over the prompt and
    its ``new`` continuation tokens every token differs from both neighbours, so for every checked row ``seq[p - J]`` differs from
    ``seq[p - J - 1]`` and ``seq[p - J + 1]`` and an off-by-one is a wrong token.  Redrawn from the next
    seed of the key otherwise; no draw in 16 is an error.  (J = 0 continues with a constant: not decisive
    under generation, so ``new`` > 0 needs J >= 1.)"""
    assert n >= J + 1 and (new == 0 or J >= 1)
    seed = zlib.crc32(repr(key).encode())
    for attempt in range(16):
        g = torch.Generator().manual_seed(seed + attempt)
        p = list(prefix) + torch.randint(0, WRONG, (n - len(prefix),), generator=g).tolist()
        x = p + expected_continuation(p, J, new)
        if all(a != b for a, b in zip(x, x[1:])) and WRONG not in x:
            return p
    raise RuntimeError(f"no decisive prompt for case {key!r}")


# ------------------------------------------------------------------------------------- builder conditions


class Patterns:
    """What the attention of a built model sees, in fp64 on the stored values: the Q and (cached) K rows
    of every position.  They depend on the position only (both read the constant dim C)."""

    def __init__(self, w: dict, offsets, head: int, weight_dtype: str = "bf16", kv_dtype: str = "bf16"):
        self.offsets, self.head, self.kv_dtype = tuple(offsets), head, kv_dtype
        self.kvh = head // (CFG.heads // CFG.kv_heads)
        wa = arm_weights(w, weight_dtype)
        self.cs = ref.rope_cos_sin(ref.llama3_inv_freq(D, CFG.rope_theta, CFG.rope_scaling), CFG.max_position).double()
        self.q_pre, self.k_pre = [], []
        for l in range(CFG.layers):
            c = _bf(torch.tensor(math.sqrt(CFG.hidden / ONES[l][0]), dtype=torch.float64))  # the norm's output at C
            col = wa[f"l{l}.qkv_w"].double()[:, C] * c
            self.q_pre.append(_bf(col[head * D:(head + 1) * D]))
            self.k_pre.append(_bf(col[(CFG.heads + self.kvh) * D:(CFG.heads + self.kvh + 1) * D]))

    def _rope(self, x: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
        cs = self.cs[pos.long()]
        cos, sin = cs[..., 0], cs[..., 1]
        x1, x2 = x[None, :D // 2], x[None, D // 2:]
        return _bf(torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1))

    def q_rows(self, l: int, pos: torch.Tensor) -> torch.Tensor:
        return self._rope(self.q_pre[l], pos)

    def k_rows(self, l: int, pos: torch.Tensor, gain: float = 1.0) -> torch.Tensor:
        """The K rows the cache holds for ``pos``: bf16, or the FP8 cache's quantised values."""
        k = self._rope(self.k_pre[l] * gain, pos)
        if self.kv_dtype == "fp8":
            k = ref.kv_dequantize(*ref.kv_quantize(k.to(torch.bfloat16))).double()
        return k


def check_gap(pat: Patterns, n_ctx: int) -> float:
    """Condition 1: for every layer, every query position p >= j and every key position s != p - j below
    ``n_ctx``, ``score[p, p - j] - score[p, s] >= ln(n_ctx 2^10)``: the rivals together then move an
    attention output by less than one bf16 step of 1.0.  -> the smallest gap (nats); AssertionError."""
    need = math.log(n_ctx * 2.0 ** BITS)
    pos = torch.arange(n_ctx)
    worst = math.inf
    for l, j in enumerate(pat.offsets):
        s = pat.q_rows(l, pos) @ pat.k_rows(l, pos).T / math.sqrt(D)
        p = torch.arange(j, n_ctx)
        peak = s[p, p - j].clone()
        s[p, p - j] = -math.inf
        gap = float((peak - s[j:].amax(1)).min())
        assert gap >= need, f"layer {l} offset {j}: score gap {gap:.2f} < {need:.2f} nats at {n_ctx} keys"
        worst = min(worst, gap)
    return worst


# ------------------------------------------------------------------------------------- models and pools


def model(w: dict, device, **kw) -> LlamaModel:
    """The model of ``w`` on ``device``; the CPU oracle computes in fp32 on the bf16-rounded values."""
    if torch.device(device).type == "cpu":
        kw = {k: v for k, v in kw.items() if k in ("weight_dtype",)}
        return LlamaModel(CFG, {k: v.float() for k, v in w.items()}, "cpu", interleaved_mlp=True, **kw)
    return LlamaModel(CFG, dict(w), device, interleaved_mlp=True, **kw)


def layout(n_seq: int, n_blocks: int, pad_cols: int = 2, seed: int = 0):
    """Block tables [n_seq, n_blocks + pad_cols] over permuted physical block ids, every block distinct;
    the padding columns point at decoy blocks no sequence owns.  -> (int32 CPU table, blocks in the pool:
    three more than the table names)."""
    cols = n_blocks + pad_cols
    total = n_seq * cols + 3
    perm = torch.randperm(total, generator=torch.Generator().manual_seed(1000 + seed))
    return perm[:n_seq * cols].view(n_seq, cols).to(torch.int32).contiguous(), total


def pool(num_blocks: int, device, kv_dtype: str = "bf16", scratch_blocks: int = 0) -> KVCache:
    dt = torch.float32 if torch.device(device).type == "cpu" else torch.bfloat16
    return KVCache(CFG.layers, num_blocks, CFG.kv_heads, BS, D, device, dtype=dt, kv_dtype=kv_dtype,
                   scratch_blocks=scratch_blocks)


def poison(kv: KVCache, pat: Patterns, bt: torch.Tensor | None = None, row_pos=None) -> None:
    """Anti-needles: every slot of every layer gets a K row that is the peak pattern of some position
    (``ANTI_GAIN`` times as long as a real key) and a V row holding the code of ``WRONG``, in the cache's
    own format.  ``row_pos[b]``: the query position the blocks of table row b (decoys included) are aimed
    at -- their layer-l pattern is that of ``row_pos[b] - j_l``, the very key that query looks for, so a
    slot read past ``ctx_len``, from a stale block or through a padding column outbids the real needle.
    Every other block holds the pattern of position 0.  The steps under test then overwrite the slots
    they really write."""
    nb = kv.num_blocks
    v = torch.zeros(D, dtype=torch.float64)
    v[:BITS] = codes()[WRONG]
    for l, j in enumerate(pat.offsets):
        pos = torch.zeros(nb, dtype=torch.long)
        if bt is not None:
            for b, p in enumerate(row_pos):
                pos[bt[b].long()] = max(int(p) - j, 0)
        k = pat.k_rows(l, pos, gain=ANTI_GAIN)  # [nb, D]
        dev = kv.k.device
        if kv.fp8:
            kd, ke = (t.to(dev) for t in ref.kv_quantize(k.to(torch.bfloat16)))
            vd, ve = (t.to(dev) for t in ref.kv_quantize(v.to(torch.bfloat16)))
            kv.k[l].copy_(kd[:, None, None, :].expand_as(kv.k[l]))
            kv.k_exp[l].copy_(ke[:, None, None].expand_as(kv.k_exp[l]))
            kv.v[l].copy_(vd.expand_as(kv.v[l]))
            kv.v_exp[l].copy_(ve.expand_as(kv.v_exp[l]))
        else:
            kv.k[l].copy_(k.to(dev, kv.k.dtype)[:, None, None, :].expand_as(kv.k[l]))
            kv.v[l].copy_(v.to(dev, kv.v.dtype).expand_as(kv.v[l]))


# ------------------------------------------------------------------------------------- steps


def _i32(x, dev):
    return torch.as_tensor(x, dtype=torch.int32).to(dev)


def _slots(bt_row: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
    p = torch.arange(lo, hi)
    return bt_row.long()[p // BS] * BS + p % BS


def prefill_meta(bt: torch.Tensor, spans, dev) -> AttnMeta:
    """Packed prefill chunks: sequence b (row b of ``bt``) feeds its tokens [lo, hi) on top of the lo it
    has cached already."""
    pos = torch.cat([torch.arange(lo, hi) for lo, hi in spans])
    slots = torch.cat([_slots(bt[b], lo, hi) for b, (lo, hi) in enumerate(spans)])
    cu = [0]
    for lo, hi in spans:
        cu.append(cu[-1] + hi - lo)
    return AttnMeta(decode=False, positions=_i32(pos, dev), slots=slots.to(dev), block_tables=bt.to(dev),
                    ctx_lens=_i32([hi for _, hi in spans], dev), cu_q=_i32(cu, dev), max_q=max(hi - lo for lo, hi in spans))


def prefill(m: LlamaModel, kv: KVCache, bt: torch.Tensor, seqs, spans=None, out_rows=None, metas=None) -> torch.Tensor:
    """One prefill step -> logits of its rows (of ``out_rows`` alone).  ``metas``: a list that receives
    the step's ``AttnMeta`` (the FP8 cache's dequantisation groups are planned into it)."""
    dev = m.device
    spans = spans or [(0, len(s)) for s in seqs]
    ids = _i32([t for s, (lo, hi) in zip(seqs, spans) for t in s[lo:hi]], dev)
    rows = None if out_rows is None else _i32(out_rows, dev)
    meta = prefill_meta(bt, spans, dev)
    if metas is not None:
        metas.append(meta)
    return m.logits(m.forward(ids, meta, kv, out_rows=rows))


def decode_meta(bt: torch.Tensor, ctx, dev, part_size: int = 512, order=None, pad: int = 0) -> AttnMeta:
    """One decode row per sequence at position ctx - 1, then ``pad`` padding rows as the engine lays
    them out (position 0, slot -1, one key of block 0)."""
    B = len(ctx)
    pos = [n - 1 for n in ctx] + [0] * pad
    slots = torch.cat([_slots(bt[b], n - 1, n) for b, n in enumerate(ctx)] + [torch.full((pad,), -1, dtype=torch.long)])
    tbl = torch.cat([bt, torch.zeros((pad, bt.shape[1]), dtype=torch.int32)]) if pad else bt
    ws = None
    if torch.device(dev).type == "cuda":
        ws = ops.DecodeWorkspace(B + pad, CFG.heads, D, -(-bt.shape[1] * BS // part_size), dev)
    return AttnMeta(decode=True, positions=_i32(pos, dev), slots=slots.to(dev), block_tables=tbl.to(dev),
                    ctx_lens=_i32(list(ctx) + [1] * pad, dev), workspace=ws, part_size=part_size,
                    order=None if order is None else _i32(list(order) + list(range(len(order), B + pad)), dev))


def decode(m: LlamaModel, kv: KVCache, bt: torch.Tensor, seqs, part_size: int = 512, order=None, pad: int = 0,
           meta_hook=None) -> torch.Tensor:
    """The decode step that feeds every sequence's LAST token over a cache holding the tokens before it
    -> logits [B (+ pad), V]."""
    dev = m.device
    meta = decode_meta(bt, [len(s) for s in seqs], dev, part_size, order, pad)
    if meta_hook is not None:
        meta = meta_hook(meta) or meta
    return m.logits(m.forward(_i32([s[-1] for s in seqs] + [0] * pad, dev), meta, kv))


def mixed(m: LlamaModel, kv: KVCache, pbt, pseqs, pspans, dbt, dseqs, pad: int = 0, order=None,
          decode_first: bool = False) -> torch.Tensor:
    """One mixed step: the prefill chunks ``pspans`` of ``pseqs``, then one decode row per sequence of
    ``dseqs`` (its last token), then ``pad`` padding rows -> logits of every row.  ``decode_first`` is the
    planted row-order mistake of the CPU module (ids / positions / slots with the decode rows in front)."""
    dev = m.device
    pm = prefill_meta(pbt, pspans, dev)
    dm = decode_meta(dbt, [len(s) for s in dseqs], dev, pad=pad, order=order)
    pids = _i32([t for s, (lo, hi) in zip(pseqs, pspans) for t in s[lo:hi]], dev)
    dids = _i32([s[-1] for s in dseqs] + [0] * pad, dev)
    parts = ((dids, pids), (dm.positions, pm.positions), (dm.slots, pm.slots))
    if not decode_first:
        parts = tuple((b, a) for a, b in parts)
    ids, pos, slots = (torch.cat(p) for p in parts)
    meta = AttnMeta(decode=False, positions=pos, slots=slots, block_tables=pm.block_tables, ctx_lens=pm.ctx_lens,
                    cu_q=pm.cu_q, max_q=pm.max_q, workspace=dm.workspace, n_decode=len(dseqs) + pad,
                    dec_block_tables=dm.block_tables, dec_ctx_lens=dm.ctx_lens, order=dm.order)
    return m.logits(m.forward(ids, meta, kv))


def prepare_decode(m: LlamaModel, pat: Patterns, seqs, seed: int = 0, scratch_blocks: int = 0, chunk: int = 16384):
    """The pool of a decode case: permuted blocks, padding columns on decoy blocks, anti-needles aimed at
    every row's decode query, then every sequence but its last token prefilled through the model (packed
    steps of up to ``chunk`` tokens).  -> (cache, block table)."""
    bt, nb = layout(len(seqs), DECODE_BLOCKS, 2, seed)
    kv = pool(nb, m.device, pat.kv_dtype, scratch_blocks)
    poison(kv, pat, bt, [len(s) - 1 for s in seqs])
    lo = 0
    while lo < len(seqs):
        hi, n = lo, 0
        while hi < len(seqs) and (hi == lo or n + len(seqs[hi]) - 1 <= chunk):
            n += len(seqs[hi]) - 1
            hi += 1
        m.forward(_i32([t for s in seqs[lo:hi] for t in s[:-1]], m.device),
                  prefill_meta(bt[lo:hi], [(0, len(s) - 1) for s in seqs[lo:hi]], m.device), kv)
        lo = hi
    return kv, bt


_oracle = {}


def oracle_margins(name: str, weight_dtype: str, kv_dtype: str, key, seqs, last: bool = False) -> torch.Tensor:
    """The CPU oracle's top-1 minus top-2 logit margin of every row of a packed forward over ``seqs``
    (NaN at the unchecked rows p < J), by packed row id; ``last``: of each sequence's last row.  The oracle
    must name every expected token itself.  Cached under ``key`` (one key, one set of sequences)."""
    k = (name, weight_dtype, kv_dtype, key, tuple(len(s) for s in seqs))
    if k not in _oracle:
        m = model(weights(name), "cpu", weight_dtype=weight_dtype)
        bt, nb = layout(len(seqs), -(-max(len(s) for s in seqs) // BS), 0, 0)
        rows, want, total = checked(seqs, sum(MODELS[name][0]))
        lg = prefill(m, pool(nb, "cpu", kv_dtype), bt, seqs, out_rows=rows)
        wrong, _ = verdict(lg, want)
        assert not wrong, f"the CPU oracle itself misses {wrong[:5]}"
        out = torch.full((total,), float("nan"))
        out[rows] = margins(lg)
        _oracle[k] = out
    if last:
        return _oracle[k][torch.tensor([len(s) for s in seqs]).cumsum(0) - 1]
    return _oracle[k]


# ------------------------------------------------------------------------------------- verdicts


def verdict(logits: torch.Tensor, want) -> tuple:
    """(rows whose argmax is not the wanted token, the smallest top-1 minus top-2 margin of the rows)."""
    lg = logits.float().cpu()
    assert lg.shape[0] == len(want), (lg.shape, len(want))
    top = lg.topk(2, dim=-1)
    wrong = [(i, int(t), int(g)) for i, (t, g) in enumerate(zip(want, top.indices[:, 0].tolist())) if t != g]
    return wrong, float((top.values[:, 0] - top.values[:, 1]).min())


def margins(logits: torch.Tensor) -> torch.Tensor:
    top = logits.float().cpu().topk(2, dim=-1).values
    return top[:, 0] - top[:, 1]


# ------------------------------------------------------------------------------------- case tables

# name -> (offsets, query head).  "prev": layer 0 reads the token itself, layer 1 the previous one; "self":
# the LAST layer reads the token itself (the only model on which a context short by one is visible);
# "far": the needle lies 130 keys back (other blocks, an earlier 512-key partition).  Heads 1 and 2 sit on
# different KV heads and are the two on which ``h % 2`` differs from ``h // 2``.
MODELS = {"prev": ((0, 1), 2), "self": ((5, 0), 1), "mid": ((3, 5), 1), "far": ((1, 130), 2)}
MAX_CTX = 1500  # no case holds more keys; ``check_gap`` enumerates this many positions
LONG_CTX = (511, 512, 513, 600)  # around one 512-key partition
DECODE_BLOCKS = -(-max(LONG_CTX) // BS)
# option arms of the GPU module: name -> (LlamaModel keywords, weight_dtype of the values, kv_dtype)
ARMS = {
    "base": ({}, "bf16", "bf16"),
    "small_norm_fused": ({"small_norm_fused": True}, "bf16", "bf16"),
    "kv_fp8": ({}, "bf16", "fp8"),
    "w_fp8": ({"weight_dtype": "fp8"}, "fp8", "bf16"),
    "w_fp8_only": ({"weight_dtype": "fp8", "fp8_weights_only": True}, "fp8", "bf16"),
    "w_mxfp4": ({"weight_dtype": "mxfp4"}, "mxfp4", "bf16"),
    "w_mxfp4_only": ({"weight_dtype": "mxfp4", "mxfp4_weights_only": True}, "mxfp4", "bf16"),
    "slab_f32": ({}, "bf16", "bf16"),  # (``slab_bf16`` off: set on the model by the test)
}

_built = {}


def weights(name: str, sharp: float = 1.0) -> dict:
    if (name, sharp) not in _built:
        offsets, head = MODELS[name]
        _built[(name, sharp)] = build(offsets, head, sharp)
    return _built[(name, sharp)]


def patterns(name: str, weight_dtype: str = "bf16", kv_dtype: str = "bf16") -> Patterns:
    """The model's patterns with condition 1 asserted on the values of the arm."""
    key = ("pat", name, weight_dtype, kv_dtype)
    if key not in _built:
        offsets, head = MODELS[name]
        pat = Patterns(weights(name), offsets, head, weight_dtype, kv_dtype)
        pat.gap = check_gap(pat, MAX_CTX)
        _built[key] = pat
    return _built[key]


def decode_ctx(name: str, B: int) -> list:
    """Context lengths (the new token included) of a decode batch: across the rows the needle key of a
    layer is the token itself (offset 0), the previous token (offset 1), position 0 (ctx = j + 1), the
    last slot of a block and the first slot of the next (ctx = j + 64 k, j + 64 k + 1 for k = 1, 2, 3 where
    that is at least J + 1; j = 0 puts the token itself there), and every 16th row holds one of
    ``LONG_CTX``: its needle or its own key lies beyond the first 512-key partition."""
    (j0, j1), _ = MODELS[name]
    J = j0 + j1
    edges = [j + k + d for j in (0, j0, j1, J) for k in (64, 128, 192) for d in (0, 1)]
    short = sorted({n for n in [J + 1, J + 2, j0 + 1, j1 + 1, 3, 40] + edges if J + 1 <= n < 200})
    return [LONG_CTX[(b // 16) % 4] if b % 16 == 15 else short[b % len(short)] for b in range(B)]


def decode_seqs(name: str, B: int, tag: str = "dec") -> list:
    """Row b's sequence does not depend on B: the rows of a smaller batch are a prefix of a larger one's,
    so one CPU oracle run serves every batch size."""
    J = sum(MODELS[name][0])
    return [prompt((tag, name, b), n, J) for b, n in enumerate(decode_ctx(name, B))]


def checked(seqs, J: int, spans=None) -> tuple:
    """(row ids of the step's rows with p >= J, their expected tokens, rows in the step): condition 3 --
    rows p < J are the only ones left out and every sequence keeps at least one."""
    spans = spans or [(0, len(s)) for s in seqs]
    rows, want, o = [], [], 0
    for s, (lo, hi) in zip(seqs, spans):
        mine = [(o + p - lo, s[p - J]) for p in range(max(lo, J), hi)]
        assert mine, "a sequence without a checked row"
        rows += [r for r, _ in mine]
        want += [t for _, t in mine]
        o += hi - lo
    return rows, want, o


# ------------------------------------------------------------------------------------- engine scenarios


def engine(w: dict, device, **kw):
    from django_assistant_bot_amd.engine.llm_engine import LLMEngine

    cpu = torch.device(device).type == "cpu"
    args = dict(device=device, weights={k: (v.float() if cpu else v) for k, v in w.items()}, max_batch=8, block_size=BS,
                num_blocks=64, max_prefill_tokens=256, use_graphs=not cpu)
    args.update(kw)
    return LLMEngine(CFG, **args)


def greedy(n: int):
    from django_assistant_bot_amd.engine.llm_engine import SamplingParams

    return SamplingParams(max_new_tokens=n, do_sample=False, temperature=0.0, ignore_eos=True)


def drive(eng, arrivals, params, on_step=None, max_steps: int = 2000) -> list:
    """``arrivals``: [(engine step at which the prompt is added, prompt)] -> request ids, in that order;
    steps until nothing is unfinished.  ``on_step(eng, step, rids)`` runs before each step."""
    todo = sorted(enumerate(arrivals), key=lambda a: a[1][0])
    rids = {}
    step = 0
    while todo or eng.has_unfinished():
        while todo and todo[0][1][0] <= step:
            i, (_, p) = todo.pop(0)
            rids[i] = eng.add_request(p, params[i] if isinstance(params, list) else params)
        if on_step is not None:
            on_step(eng, step, rids)
        eng.step()
        step += 1
        assert step < max_steps, "the engine does not finish"
    return [rids[i] for i in range(len(arrivals))]


def assert_continuations(eng, rids, prompts, J: int, n: int, skip=()) -> None:
    for i, (rid, p) in enumerate(zip(rids, prompts)):
        if i in skip:
            continue
        got = eng.pop_output(rid).token_ids
        want = expected_continuation(p, J, n)
        assert got == want, (i, [(k, a, b) for k, (a, b) in enumerate(zip(got, want)) if a != b][:5], len(got))
