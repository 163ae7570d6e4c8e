"""The glue of ``models/llama.py`` and ``engine/llm_engine.py`` on the GPU under the copy decoder of
tests/copy_decoder.py: which position, slot, block table, context length, layer cache, row order and
dispatch order each kernel receives.  The decoder's output names the token it read, so every step kind of
``LlamaModel.forward`` and every scheduling path of ``LLMEngine`` is held to tokens known in closed form
(``x[n] = x[n - 1 - J]``): the token is the assertion.  In addition the logit margin (top-1 minus top-2) of
every checked row must be at least half the CPU oracle's margin of the same row (6.05 - 6.50 there): a
healthy bf16 path costs a few percent, one rival key let in at weight 1 / n far more.

Every pool is filled with anti-needles first (``copy_decoder.poison``), the physical block ids are
permuted and the block tables carry padding columns that point at decoy blocks.  The builder's conditions
for these case keys are asserted on the CPU (tests/test_copy_decoder_cpu.py) and again here, on the values
of each arm (``copy_decoder.patterns``).

Rows checked / rows in the steps and the smallest margin measured on an MI355X, per family (CPU oracle:
6.36 bf16, 6.45 FP8 weights, 6.16 MXFP4 weights, 6.36 FP8 cache; the GPU logits are bf16, whose step at 31.8
is 0.125; the unchecked rows are the rows p < J of a prefill and the padding rows):

    decode step                   1597 / 1600  rows   smallest margin 6.38
    decode step, 2 partitions      222 / 222   rows   smallest margin 6.38
    prefill, streamed              240 / 257   rows   smallest margin 6.38
    prefill, MFMA                 1123 / 1680  rows   smallest margin 6.38
    prefill, gemm_mid              169 / 300   rows   smallest margin 6.38
    prefill, gemm256              3807 / 4200  rows   smallest margin 6.38
    prefill, cached prefix         300 / 306   rows   smallest margin 6.38
    prefill, chunked               451 / 590   rows   smallest margin 6.38
    prefill, out_rows               10 / 10    rows   smallest margin 6.38
    mixed step                     384 / 576   rows   smallest margin 6.38
    arm small_norm_fused           607 / 1027  rows   smallest margin 6.38
    arm kv_fp8                     607 / 1027  rows   smallest margin 6.38
    arm w_fp8                      607 / 1027  rows   smallest margin 6.38
    arm w_fp8_only                 607 / 1027  rows   smallest margin 6.38
    arm w_mxfp4                    607 / 1027  rows   smallest margin 6.25
    arm w_mxfp4_only               607 / 1027  rows   smallest margin 6.25
    arm slab_f32                   607 / 1027  rows   smallest margin 6.38

No case failed on the GPU: every row of every step kind and every engine request gave its closed-form
token.  The engine cases assert tokens and the ``stats`` counters that prove each path ran.
"""
import pytest
import torch

import copy_decoder as cd
from django_assistant_bot_amd import ops
from django_assistant_bot_amd.models.llama import LlamaModel

pytestmark = pytest.mark.gpu

DEV = "cuda"
L = cd.CFG.layers
SEEN = {}  # family -> [rows checked, smallest margin]


def _model(name, arm="base"):
    key = ("model", name, arm, DEV)
    if key not in cd._built:
        kw, wd, kvd = cd.ARMS[arm]
        cd.patterns(name, wd, kvd)  # condition 1 on the values of the arm
        m = cd.model(cd.weights(name), DEV, **kw)
        if arm == "slab_f32":
            m.slab_bf16 = False
        if arm == "small_norm_fused":
            assert m.fold_norms and m.small_norm_fused
        cd._built[key] = m
    return cd._built[key]


def _judge(family, logits, want, oracle, total):
    """The token is the assertion; then every row's margin against half the oracle's.  ``total``: the rows
    of the step (the unchecked ones are the rows p < J of a prefill, and padding)."""
    wrong, _ = cd.verdict(logits, want)
    mg = cd.margins(logits)
    seen = SEEN.setdefault(family, [0, 0, float("inf")])
    seen[0] += len(want)
    seen[1] += total
    seen[2] = min(seen[2], float(mg.min()))
    print(f"[{family}] checked {len(want)} / {total} rows, smallest margin {float(mg.min()):.2f} "
          f"(oracle {float(oracle.min()):.2f})")
    assert not wrong, f"{family}: {len(wrong)} of {len(want)} rows name a wrong token: (row, want, got) {wrong[:8]}"
    low = (mg < 0.5 * oracle).nonzero().flatten().tolist()
    assert not low, f"{family}: margin under half the oracle's at rows {low[:8]}: {mg[low[:8]].tolist()}"


class _Spy:
    """The stream_gemm configurations and the native MFMA GEMM entry points of a step."""

    def __init__(self, monkeypatch):
        self.cfgs, self.n = [], {}
        real = ops.stream_gemm

        def stream(x, w, *a, **k):
            self.cfgs.append(k.get("cfg", 0))
            return real(x, w, *a, **k)

        monkeypatch.setattr(ops, "stream_gemm", stream)
        nat = ops.native()
        for name in ("gemm_bt", "gemm256", "gemm_mid"):
            monkeypatch.setattr(nat, name, self._count(name, getattr(nat, name)))

    def _count(self, name, real):
        def f(*a, **k):
            self.n[name] = self.n.get(name, 0) + 1
            return real(*a, **k)
        return f

    def take(self):
        out = (sorted(set(self.cfgs)), len(self.cfgs), self.n)
        self.cfgs, self.n = [], {}
        return out


def _order(seqs):
    """The engine's dispatch order: longest context first."""
    return torch.tensor([-len(s) for s in seqs]).argsort(stable=True).tolist()


# -------------------------------------------------------------------------------------------- decode step

# batch size -> (stream_gemm configurations, stream_gemm calls, gemm_mid calls) of one decode step with its
# LM head: 16-row tiles, 32-row tiles, BN 128 at M <= 64, the whole-chip gate_up tiling beside BN 128 at
# M <= 128, and from 129 rows on the M <= 256 tiles with gate_up on the mid-M GEMM
DISPATCH = {1: ([30], 4 * L + 1, 0), 16: ([30], 4 * L + 1, 0), 17: ([31], 4 * L + 1, 0), 64: ([13], 4 * L + 1, 0),
            100: ([10, 20], 4 * L + 1, 0), 130: ([27], 3 * L + 1, L), 200: ([27], 3 * L + 1, L)}


def _decode_case(name, B, arm, monkeypatch, family, order="engine", seqs=None, key="dec", **kw):
    J = sum(cd.MODELS[name][0])
    _, wd, kvd = cd.ARMS[arm]
    m = _model(name, arm)
    seqs = seqs or cd.decode_seqs(name, B)
    kv, bt = cd.prepare_decode(m, cd.patterns(name, wd, kvd), seqs, seed=B, scratch_blocks=cd.DECODE_BLOCKS + 2)
    spy = _Spy(monkeypatch)
    lg = cd.decode(m, kv, bt, seqs, order=_order(seqs) if order == "engine" else order, **kw)
    got = spy.take()
    # (row b's sequence does not depend on B: one oracle run serves every batch size of an arm)
    full = cd.decode_seqs(name, 200 if arm == "base" else 100) if key == "dec" else seqs
    oracle = cd.oracle_margins(name, wd, kvd, key, full, last=True)[:len(seqs)]
    _judge(family, lg[:len(seqs)], [s[len(s) - 1 - J] for s in seqs], oracle, lg.shape[0])
    return got


@pytest.mark.parametrize("B", sorted(DISPATCH))
@pytest.mark.parametrize("name", ["prev", "self", "far"])
def test_decode_step(name, B, monkeypatch):
    """Every row of the batch names its token.  Across the rows the needle is the token itself, the
    previous token, position 0, the last slot of a block, the first slot of the next and (every 16th row:
    contexts 511 / 512 / 513 / 600) a key of an earlier 512-key partition; B <= 32 runs the two-slot
    attention kernel, larger batches the one-slot one."""
    cfgs, calls, n = _decode_case(name, B, "base", monkeypatch, "decode step")
    assert (cfgs, calls, n.get("gemm_mid", 0)) == DISPATCH[B] and set(n) <= {"gemm_mid"}


@pytest.mark.parametrize("order", [None, "reversed", "engine"])
@pytest.mark.parametrize("B", [4, 33])
def test_decode_across_a_partition_boundary(B, order, monkeypatch):
    """Contexts 511 / 512 / 513 / 600 alone, ``part_size`` 512 (two partitions), on the two-slot (B = 4) and
    the one-slot (B = 33: more than 64 (sequence, KV head) pairs) attention kernel, with and without a dispatch order; "far" reads 130 keys back,
    "self" the new token's own key, which is the first key of the second partition at context 513."""
    for name in ("far", "self"):
        J = sum(cd.MODELS[name][0])
        # (B = 33: every fourth row is long, the rest have the shortest context a row can have)
        ctx = [cd.LONG_CTX[(b if B == 4 else b // 4) % 4] if B == 4 or b % 4 == 0 else J + 1 + b for b in range(B)]
        seqs = [cd.prompt(("part", name, b), n, J) for b, n in enumerate(ctx)]
        assert {len(s) for s in seqs} >= set(cd.LONG_CTX)
        o = list(range(B))[::-1] if order == "reversed" else order
        _decode_case(name, B, "base", monkeypatch, "decode step, 2 partitions", order=o, seqs=seqs, key=("part", B))
        monkeypatch.undo()


def test_decode_with_padding_rows(monkeypatch):
    """The engine's padded rows (position 0, slot -1, context 1, block 0) behind the real ones."""
    _decode_case("self", 13, "base", monkeypatch, "decode step", pad=3)


@pytest.mark.parametrize("mistake,name,field,delta", [("position + 1", "mid", "positions", 1),
                                                      ("ctx_lens - 1", "self", "ctx_lens", -1)])
def test_a_planted_mistake_shows_on_the_gpu_path_too(mistake, name, field, delta):
    """Two of the CPU module's planted mistakes that stay inside every buffer, on the GPU decode step: all
    rows but those with the shortest contexts (at most three of 17) name a wrong token."""
    J = sum(cd.MODELS[name][0])
    m = _model(name)
    seqs = cd.decode_seqs(name, 17)
    kv, bt = cd.prepare_decode(m, cd.patterns(name), seqs, seed=17)
    lg = cd.decode(m, kv, bt, seqs, order=_order(seqs), meta_hook=lambda meta: setattr(meta, field, getattr(meta, field) + delta))
    wrong, _ = cd.verdict(lg, [s[len(s) - 1 - J] for s in seqs])
    print(f"{mistake} on {name!r}: {len(wrong)} of 17 rows give a wrong token")
    assert len(wrong) >= 14, mistake


# ------------------------------------------------------------------------------------------------ prefill


def _oracle_rows(name, arm, key, seqs, spans):
    """The oracle's margins of the checked rows of the chunks ``spans`` (a whole forward over ``seqs``)."""
    J = sum(cd.MODELS[name][0])
    _, wd, kvd = cd.ARMS[arm]
    rows, off = [], 0
    for s, (lo, hi) in zip(seqs, spans):
        rows += [off + p for p in range(max(lo, J), hi)]
        off += len(s)
    return cd.oracle_margins(name, wd, kvd, key, seqs)[rows]


def _prefill_case(name, lens, arm, family, key, spans=None, cached=None, out_rows=None, scratch_blocks=0, metas=None):
    """One prefill step over fresh decisive sequences of ``lens`` tokens (``spans``: the chunk of each that
    is fed, after its first ``lo`` tokens went through a step of their own)."""
    J = sum(cd.MODELS[name][0])
    _, wd, kvd = cd.ARMS[arm]
    m = _model(name, arm)
    seqs = [cd.prompt((key, name, i), n, J) for i, n in enumerate(lens)]
    spans = spans or [(0, n) for n in lens]
    bt, nb = cd.layout(len(seqs), -(-max(lens) // cd.BS), 2, len(lens))
    kv = cd.pool(nb, DEV, kvd, scratch_blocks or -(-max(lens) // cd.BS) * len(lens))
    cd.poison(kv, cd.patterns(name, wd, kvd), bt, [n - 1 for n in lens])
    if any(lo for lo, _ in spans):
        first = [(b, lo) for b, (lo, _) in enumerate(spans) if lo]
        cd.prefill(m, kv, bt[[b for b, _ in first]], [seqs[b] for b, _ in first], [(0, lo) for _, lo in first])
    rows, want, T = cd.checked(seqs, J, spans)
    oracle = _oracle_rows(name, arm, (key, tuple(lens)), seqs, spans)
    if out_rows is not None:
        keep = [i for i, r in enumerate(rows) if r in set(out_rows)]
        assert sorted(rows[i] for i in keep) == sorted(out_rows), "an unchecked row among out_rows"
        lut = {rows[i]: i for i in keep}
        sel = [lut[r] for r in out_rows]
        lg = cd.prefill(m, kv, bt, seqs, spans, out_rows=out_rows, metas=metas)
        _judge(family, lg, [want[i] for i in sel], oracle[sel], len(out_rows))
        return m, T
    lg = cd.prefill(m, kv, bt, seqs, spans, metas=metas)
    assert lg.shape[0] == T
    _judge(family, lg[rows], want, oracle, T)
    return m, T


@pytest.mark.parametrize("name,T", [("prev", 64), ("mid", 64), ("mid", 128), ("far", 200)])
def test_prefill_streamed(name, T, monkeypatch):
    """T = 64, 128: the streamed short prefill; ("far", 200): a ONE-token chunk behind 199 cached tokens."""
    spy = _Spy(monkeypatch)
    if T == 200:
        _prefill_case(name, [T], "base", "prefill, streamed", "pfs", spans=[(199, 200)])
        return
    _prefill_case(name, [T], "base", "prefill, streamed", "pfs")
    cfgs, calls, n = spy.take()
    assert calls == 4 * L + 1 and not n  # (the LM head of T rows streams too)


@pytest.mark.parametrize("name,T", [("mid", 129), ("far", 300), ("prev", 300)])
def test_prefill_on_the_mfma_gemms(name, T, monkeypatch):
    spy = _Spy(monkeypatch)
    _prefill_case(name, [T], "base", "prefill, MFMA", "pfm")
    cfgs, calls, n = spy.take()
    assert sum(n.values()) >= 4 * L and calls <= 1  # (only the LM head may stream)


def _family_lens():
    """{kernel family: sequence lengths of a prefill step whose four projections all take it}, searched in
    the dispatch predicates themselves."""
    K = ops.kernels
    shapes = [(1024, 512), (512, 512), (1792, 512), (512, 896)]

    def family(T):
        if T <= LlamaModel.PREFILL_STREAM_MAX_M:
            return "stream"
        f = {("gemm_mid" if K.use_gemm_mid(T, N, Kd, Kd) else "gemm256" if K.use_gemm256(T, N, Kd, Kd, Kd) else "gemm_bt")
             for N, Kd in shapes}
        return f.pop() if len(f) == 1 else None

    out = {}
    for lens in ([64], [300], [K.GEMM256_MIN_M], [1400, 1399, 1401], [1100] * 8):
        out.setdefault(family(sum(lens)), lens)
    return out


@pytest.mark.parametrize("fam", ["gemm_mid", "gemm256"])
def test_prefill_per_gemm_family(fam, monkeypatch):
    lens = _family_lens().get(fam)
    assert lens is not None, f"no prefill size of the toy decoder dispatches {fam}"
    spy = _Spy(monkeypatch)
    _prefill_case("far", lens, "base", f"prefill, {fam}", "fam")
    _, _, n = spy.take()
    assert n.get(fam, 0) >= 4 * L and set(n) == {fam}


def test_prefill_packed_sequences_of_unequal_length():
    _prefill_case("mid", [37, 150, 90], "base", "prefill, MFMA", "packed")
    _prefill_case("far", [140, 333, 201], "base", "prefill, MFMA", "packed")


def test_prefill_behind_128_cached_tokens():
    """``ctx_lens`` > the chunk: the first 128 tokens (two blocks) are cached; on "far" the needle of every
    row up to 258 lies in them."""
    _prefill_case("far", [300, 190], "base", "prefill, cached prefix", "hit", spans=[(128, 300), (128, 190)])
    _prefill_case("mid", [200], "base", "prefill, cached prefix", "hit", spans=[(128, 200)])


def test_prompt_fed_in_two_chunks():
    """Both chunks are checked: the first as a step of its own, the second behind it."""
    _prefill_case("far", [300], "base", "prefill, chunked", "chunk", spans=[(0, 170)])
    _prefill_case("far", [300], "base", "prefill, chunked", "chunk", spans=[(170, 300)])
    _prefill_case("mid", [300, 90], "base", "prefill, chunked", "chunk", spans=[(100, 300), (0, 90)])


def test_prefill_out_rows_pruned_and_whole(monkeypatch):
    """``out_rows`` on the pruned last-layer tail (a gemm256 step) and on a step that runs whole."""
    lens = _family_lens()["gemm256"]
    T = sum(lens)
    rows = [lens[0] - 1, lens[0] + lens[1] - 1, T - 1, 500, lens[0] + 131]
    spy = _Spy(monkeypatch)
    m, _ = _prefill_case("far", lens, "base", "prefill, out_rows", "fam", out_rows=rows)
    _, _, n = spy.take()
    x = torch.empty(1, device=DEV)
    meta = cd.AttnMeta(decode=False, positions=x, slots=x, block_tables=x, ctx_lens=x)
    assert m._tail_prunable(T, meta, x, False) and set(n) == {"gemm256"} and not m._tail_prunable(300, meta, x, False)
    _prefill_case("far", [300], "base", "prefill, out_rows", "pfm", out_rows=[299, 131, 200])
    _prefill_case("mid", [64], "base", "prefill, out_rows", "pfs", out_rows=[63, 8])


# --------------------------------------------------------------------------------------------- mixed step


def _mixed_case(name, arm, nd, plens, pspans=None, family="mixed step"):
    J = sum(cd.MODELS[name][0])
    _, wd, kvd = cd.ARMS[arm]
    m = _model(name, arm)
    dseqs = cd.decode_seqs(name, nd, "mixdec")
    pseqs = [cd.prompt(("mixpf", name, i), n, J) for i, n in enumerate(plens)]
    pspans = pspans or [(0, n) for n in plens]
    bt, nb = cd.layout(nd + len(pseqs), cd.DECODE_BLOCKS, 2, 9)
    kv = cd.pool(nb, DEV, kvd, nb)
    cd.poison(kv, cd.patterns(name, wd, kvd), bt, [len(s) - 1 for s in dseqs + pseqs])
    dbt, pbt = bt[:nd], bt[nd:]
    cd.prefill(m, kv, dbt, dseqs, [(0, len(s) - 1) for s in dseqs])
    first = [(b, lo) for b, (lo, _) in enumerate(pspans) if lo]
    if first:
        cd.prefill(m, kv, pbt[[b for b, _ in first]], [pseqs[b] for b, _ in first], [(0, lo) for _, lo in first])
    Tp = sum(hi - lo for lo, hi in pspans)
    pad = (-(Tp + nd)) % 64  # the engine pads a mixed step's decode rows to whole 64-row tiles
    lg = cd.mixed(m, kv, pbt, pseqs, pspans, dbt, dseqs, pad=pad, order=_order(dseqs))
    assert lg.shape[0] == Tp + nd + pad
    rows, want, _ = cd.checked(pseqs, J, pspans)
    oracle = torch.cat([_oracle_rows(name, arm, ("mixpf", tuple(plens)), pseqs, pspans),
                        cd.oracle_margins(name, wd, kvd, "mixdec", dseqs, last=True)])
    _judge(family, lg[rows + list(range(Tp, Tp + nd))], want + [s[len(s) - 1 - J] for s in dseqs], oracle, lg.shape[0])
    return pad


def test_mixed_step():
    """Prefill rows, decode rows and padded rows (slot -1) in one forward; one prompt is the second chunk
    of a sequence."""
    assert _mixed_case("mid", "base", 5, [90, 30]) == 3
    assert _mixed_case("far", "base", 21, [170, 300], [(0, 170), (140, 300)]) == 33
    assert _mixed_case("self", "base", 40, [20]) == 4


# --------------------------------------------------------------------------------------------- option arms


@pytest.mark.parametrize("arm", [a for a in cd.ARMS if a != "base"])
def test_option_arms(arm, monkeypatch):
    """One decode step of B <= 16, one of B = 100 and one prefill step under every option; the expected
    tokens are the same closed form."""
    fam = f"arm {arm}"
    cfgs, calls, n = _decode_case("self", 16, arm, monkeypatch, fam)
    if arm == "small_norm_fused":
        assert 32 in cfgs  # (``_layer_small``: o / down on the whole-K 16-row tiles)
    monkeypatch.undo()
    _decode_case("far", 100, arm, monkeypatch, fam)
    monkeypatch.undo()
    _decode_case("prev", 9, arm, monkeypatch, fam)
    monkeypatch.undo()
    metas = []
    scratch = 6 if arm == "kv_fp8" else 0  # three sequences of 6 / 3 / 4 blocks: at least two groups
    _prefill_case("far", [333, 140, 201], arm, fam, "packed-arm", scratch_blocks=scratch, metas=metas)
    if arm == "kv_fp8":
        assert len(metas[0].kv_groups) >= 2
    _prefill_case("mid", [100], arm, fam, "pfs-arm")
    _mixed_case("mid", arm, 5, [90, 30], family=fam)


# -------------------------------------------------------------------------------------------------- engine

NEW = 24


def _engine(name, sharp=1.0, **kw):
    args = dict(max_batch=8, num_blocks=96, max_prefill_tokens=256, max_model_len=704)
    args.update(kw)
    return cd.engine(cd.weights(name, sharp), DEV, **args)


def _prompts(key, name, lens, new=NEW, prefix=()):
    J = sum(cd.MODELS[name][0])
    return [cd.prompt((key, name, i), n, J, new, prefix=prefix) for i, n in enumerate(lens)]


@pytest.mark.parametrize("graphs,pipeline", [(True, True), (True, False), (False, True), (False, False)])
def test_engine_graphs_and_pipelined_decode(graphs, pipeline):
    name = "mid"
    J = sum(cd.MODELS[name][0])
    prompts = _prompts("eng", name, (10, 77, 150, 64, 129))
    eng = _engine(name, use_graphs=graphs, pipeline_decode=pipeline)
    piped = []
    real = eng._step_pipelined
    eng._step_pipelined = lambda: piped.append(1) or real()
    rids = cd.drive(eng, [(0, p) for p in prompts], cd.greedy(NEW))
    cd.assert_continuations(eng, rids, prompts, J, NEW)
    st = eng.stats
    assert (st["graph_replays"] > 0) == graphs and (len(piped) > 0) == pipeline and st["decode_tokens"] >= 5 * (NEW - 1)


def test_engine_staggered_arrivals_run_mixed_steps():
    name = "far"
    J = sum(cd.MODELS[name][0])
    prompts = _prompts("stagger", name, (140, 200, 333, 150, 180))
    eng = _engine(name, mixed_prefill_tokens=64)
    rids = cd.drive(eng, [(3 * i, p) for i, p in enumerate(prompts)], cd.greedy(NEW))
    cd.assert_continuations(eng, rids, prompts, J, NEW)
    assert eng.stats["mixed_steps"] >= 4


def test_engine_chunked_prompt_and_a_context_that_crosses_512():
    """A prompt longer than ``max_prefill_tokens`` (three chunks) whose context then grows across a block
    boundary and across the 512-key partition during generation; a second one crosses 64 and 128."""
    name = "far"
    J = sum(cd.MODELS[name][0])
    new = 40
    prompts = _prompts("long", name, (600, 500, 140), new)
    eng = _engine(name)
    rids = cd.drive(eng, [(0, prompts[0]), (1, prompts[1]), (1, prompts[2])], cd.greedy(new))
    cd.assert_continuations(eng, rids, prompts, J, new)
    assert eng.stats["prefill_steps"] >= 4 and eng.stats["prefill_tokens"] == 1240


@pytest.mark.parametrize("within_one_step", [True, False])
def test_engine_shared_prefix(within_one_step):
    name = "far"
    J = sum(cd.MODELS[name][0])
    shared = cd.prompt("shared128", 128, 0)  # (neighbours differ; the sharers' draws make the whole decisive)
    prompts = _prompts("sharers", name, (150, 171, 200, 140), prefix=shared)
    eng = _engine(name, max_prefill_tokens=1024)
    rids = cd.drive(eng, [(0 if within_one_step else 2 * i, p) for i, p in enumerate(prompts)], cd.greedy(NEW))
    cd.assert_continuations(eng, rids, prompts, J, NEW)
    assert eng.blocks.prefix_hits() >= 3 * 128
    assert eng.stats["prefill_tokens"] == sum(len(p) for p in prompts) - 3 * 128


def test_engine_preemption_and_recompute():
    name = "mid"
    J = sum(cd.MODELS[name][0])
    new = 40
    prompts = _prompts("preempt", name, (100, 120, 90, 110), new)
    eng = _engine(name, num_blocks=8, max_model_len=256)  # 4 sequences need up to 3 blocks each
    rids = cd.drive(eng, [(0, p) for p in prompts], cd.greedy(new))
    cd.assert_continuations(eng, rids, prompts, J, new)
    assert eng.stats["preemptions"] >= 1 and eng.blocks.num_free_blocks() == eng.blocks.num_blocks()


def test_engine_abort_and_reuse_of_the_freed_blocks():
    name = "mid"
    J = sum(cd.MODELS[name][0])
    new = 30
    prompts = _prompts("abort", name, (90, 95, 80, 92), new)  # two blocks each, also with their new tokens
    eng = _engine(name, num_blocks=6, max_model_len=256, prefix_cache=False)  # three sequences fill the pool
    state = {}

    def on_step(eng, step, rids):
        if step == 8:
            assert eng.abort(rids[1]) and eng.blocks.num_free_blocks() >= 2
            state["free"] = eng.blocks.num_free_blocks()

    rids = cd.drive(eng, [(0, prompts[0]), (0, prompts[1]), (0, prompts[2]), (9, prompts[3])], cd.greedy(new), on_step)
    out1 = eng.finished[rids[1]]
    assert out1.finish_reason == "abort" and 0 < len(out1.out) < new
    assert out1.out == cd.expected_continuation(prompts[1], J, len(out1.out))
    cd.assert_continuations(eng, rids, prompts, J, new, skip=(1,))
    assert eng.stats["preemptions"] == 0 and state["free"] < 4  # the late request needed the aborted one's blocks
    assert eng.blocks.num_free_blocks() == eng.blocks.num_blocks()


@pytest.mark.parametrize("kw", [dict(kv_cache_dtype="fp8"), dict(weight_dtype="mxfp4", mxfp4_weights_only=True)],
                         ids=["kv_fp8", "mxfp4_only"])
def test_engine_lossy_options(kw):
    name = "far"
    J = sum(cd.MODELS[name][0])
    cd.patterns(name, "mxfp4" if "weight_dtype" in kw else "bf16", "fp8" if "kv_cache_dtype" in kw else "bf16")
    prompts = _prompts("lossy", name, (140, 300, 505))
    eng = _engine(name, mixed_prefill_tokens=64, **kw)
    rids = cd.drive(eng, [(0, prompts[0]), (0, prompts[1]), (4, prompts[2])], cd.greedy(NEW))
    cd.assert_continuations(eng, rids, prompts, J, NEW)
    assert eng.stats["mixed_steps"] > 0
    assert eng.stats["graph_replays"] > 0
    assert eng.stats["kv_cache_bits"] == (8 if "kv_cache_dtype" in kw else 16)
    assert eng.stats["weight_bf16_copy"] is ("weight_dtype" not in kw)


def test_engine_sampling_path_gives_the_greedy_tokens():
    """``do_sample`` with temperature 1, top-k 50, top-p 0.95 on a model built with ``sharp=16``: the margin
    is about 100 nats, so the in-graph sampling path must return the closed-form tokens too."""
    from django_assistant_bot_amd.engine.llm_engine import SamplingParams

    name = "mid"
    J = sum(cd.MODELS[name][0])
    prompts = _prompts("sampled", name, (30, 90, 140))
    eng = _engine(name, sharp=16.0)
    sp = SamplingParams(max_new_tokens=NEW, do_sample=True, temperature=1.0, top_k=50, top_p=0.95, ignore_eos=True, seed=7)
    rids = cd.drive(eng, [(0, prompts[0]), (0, prompts[1]), (2, prompts[2])], sp)
    cd.assert_continuations(eng, rids, prompts, J, NEW)
    assert eng.stats["graph_replays"] > 0


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A fault leaves the device unusable for the rest of the process: end the run, start nothing more."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit(f"GPU fault, no further test is started: {exc}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _family_table():
    """Prints the per-family table of the run (the figures of the module docstring) after the last test."""
    yield
    for fam, (rows, total, mg) in sorted(SEEN.items()):
        print(f"    {fam:<28s} {rows:>5d} / {total:<5d} rows   smallest margin {mg:.2f}")
