"""The needle harness of tests/attn_cases.py proves itself on the fp32 oracle (``ops.*`` on CPU tensors
runs ops/reference.py): the oracle passes every case of tests/test_attention_needles_gpu.py at its
real shape, and small deliberately wrong oracles -- the off-by-one mistakes attention kernels make --
fail the checker on exactly the needle rows that sit on the broken edge.

Why this module exists: the same wrong oracles pass the tolerance check the kernel tests use
(``close(atol=2e-2, rtol=2e-2)``) on random 8K-context inputs; ``test_random_8k_is_blind`` keeps that
on record.
"""
import math

import pytest
import torch

import attn_cases as ac
from django_assistant_bot_amd import ops

ALL = sorted(ac.CASES)


def _vis(case, b, n, fn=None):
    """[m, n] visibility of the case's own mask, optionally edited by ``fn``."""
    v = ac.causal_mask(case, b, n) if case.causal else torch.ones(case.qlens[b], n, dtype=torch.bool)
    return v if fn is None else fn(v)


def _skip(lo, hi):
    def fn(v):
        v = v.clone()
        v[:, lo:hi] = False
        return v
    return fn


def mutant(case, kind):
    """A wrong fp32 oracle.  Returns the output in the layout of ``ac.run``."""
    outs = []
    for b in range(case.B):
        n = case.klens[b]
        K, V = ac.logical_kv(case, b)
        vis = None
        if kind == "ctx-1":  # the last key (the token just written) is not read
            K, V, vis = K[:n - 1], V[:n - 1], _vis(case, b, n - 1)
        elif kind == "diag-dropped":  # causal mask with >= in place of >
            vis = ac.causal_mask(case, b, n, strict=True)
        elif kind == "diag+1":  # causal mask key > qpos + 1
            vis = ac.causal_mask(case, b, n, shift=1)
        elif kind == "skip-512":  # one 64-key tile at a partition boundary skipped
            vis = _vis(case, b, n, _skip(512, 576))
        elif kind == "tail":  # n rounded up to the block size
            K, V = ac.logical_kv(case, b, -(-n // case.bs) * case.bs)
            vis = torch.ones(case.qlens[b], K.shape[0], dtype=torch.bool)
        elif kind == "extra-col":  # one more block-table column than the context has
            nb = -(-n // case.bs)
            if nb < case.bt.shape[1]:
                K, V = ac.logical_kv(case, b, (nb + 1) * case.bs)
                vis = _skip(n, nb * case.bs)(torch.ones(case.qlens[b], K.shape[0], dtype=torch.bool))
        elif kind == "head+1":  # kv head h + 1 read for head h
            K, V = K.roll(-1, dims=1), V.roll(-1, dims=1)
        elif kind == "left" and b > 0:  # the packed K range starts one row early
            K, V = ac.logical_kv(case, b, left=1)
            vis = torch.ones(case.qlens[b], n + 1, dtype=torch.bool)
        elif kind == "right" and b < case.B - 1:  # ... or ends one row late
            K, V = ac.logical_kv(case, b, right=1)
            vis = torch.ones(case.qlens[b], n + 1, dtype=torch.bool)
        outs.append(ac.attend(case, b, K, V, dtype=torch.float32, visible=vis).to(torch.bfloat16))
    return torch.cat(outs)


def expected_bad(case, kind):
    """The needle rows (sequence, row position, kv head) that sit on the edge ``kind`` breaks."""
    nb = lambda s: -(-case.klens[s] // case.bs)  # noqa: E731
    hit = {
        "ctx-1": lambda s, p, j: j == case.klens[s] - 1,
        "diag-dropped": lambda s, p, j: j == p,
        "diag+1": lambda s, p, j: p + 1 < case.klens[s],
        "skip-512": lambda s, p, j: 512 <= j < 576,
        "tail": lambda s, p, j: case.klens[s] % case.bs != 0,
        "extra-col": lambda s, p, j: nb(s) < case.bt.shape[1],
        "head+1": lambda s, p, j: True,
        "left": lambda s, p, j: s > 0,
        "right": lambda s, p, j: s < case.B - 1,
    }[kind]
    return {key for key, j in ac.needle_keys(case).items() if hit(key[0], key[1], j)}


@pytest.mark.parametrize("needles", [True, False], ids=["needles", "plain"])
@pytest.mark.parametrize("name", ALL)
def test_oracle_passes(name, needles):
    case = ac.get_case(name, "cpu", needles)
    rep = ac.check(case, ac.run(case, ops))
    assert rep.ok, str(rep)
    if needles:
        assert rep.needle_dev == 0.0  # fp32 weights of 1 - 2e-9 round to the code itself
        assert len(ac.needle_keys(case)) >= case.B * case.Hkv
    else:
        assert rep.f is not None and rep.tau <= ac.TAU_CAP and rep.ratio <= 1.5  # fp32 math: one rounding of O


def test_codes_are_bf16_exact_and_distinct():
    pos = torch.arange(1 << ac.POS_BITS)
    c = ac.code(pos[:, None, None], torch.arange(4)[None, :, None], torch.tensor([0, 3, ac.STALE_SEQ])[None, None, :], 32)
    assert torch.equal(c.to(torch.bfloat16).float(), c)
    flat = c.reshape(-1, 32)
    assert torch.unique(flat, dim=0).shape[0] == flat.shape[0]  # +-1 codes: different slots differ by 2.0
    assert ac.decode_code(ac.code(8191, 5, 9, 128)) == (8191, 5, 9)
    for D in (32, 64, 128):  # the needle directions are orthogonal and the coefficients bf16-exact
        H = ac.hadamard(D)
        assert torch.equal(H @ H.t(), D * torch.eye(D))
        c30 = ac.needle_coef(1 / math.sqrt(D), D)
        assert c30 * D / math.sqrt(D) >= ac.NEEDLE_NATS and float(torch.tensor(17 * c30).to(torch.bfloat16)) == 17 * c30


DECODE = [n for n in ALL if n.startswith("dec")]
PAGED = [n for n in ALL if n.startswith("pre") and n != "pre_g2"]  # (pre_g2: pre_g's edges at four times the cost)
PACKED = [n for n in ALL if n.startswith("pack")]
CAUSAL = [n for n in PAGED + PACKED if n.endswith("-c") or n in ("pre_g", "pre_g-odd", "pre_long")]  # (no case is built at collection)
MUTANTS = ([("ctx-1", n) for n in DECODE + PAGED + PACKED] + [("head+1", n) for n in DECODE + PAGED + PACKED if "-g16" not in n]
           + [("diag-dropped", n) for n in CAUSAL] + [("diag+1", n) for n in CAUSAL]
           + [("skip-512", n) for n in ("dec_a-s0", "dec_a-s8", "dec_b-p512", "dec_b-p2048")]
           + [("tail", n) for n in DECODE + PAGED if n not in CAUSAL]
           + [("extra-col", n) for n in DECODE + PAGED]
           + [(k, n) for k in ("left", "right") for n in PACKED if n not in CAUSAL])


@pytest.mark.parametrize("kind,name", MUTANTS)
def test_wrong_oracle_fails_on_the_broken_edge(kind, name):
    case = ac.get_case(name)
    want = expected_bad(case, kind)
    rep = ac.check(case, mutant(case, kind))
    assert rep.needle_bad == want, f"{kind}: {sorted(rep.needle_bad ^ want)}"
    if want:
        assert not rep.ok


def test_every_mutant_breaks_some_case():
    """No mutant passes by finding no needle on its edge anywhere, and the needle positions the GPU
    cases rely on are all present."""
    for kind in sorted({k for k, _ in MUTANTS}):
        assert any(expected_bad(ac.get_case(n), kind) for k, n in MUTANTS if k == kind), kind
    seen = {j for n in ("dec_a-s0", "dec_a-s8") for (s, p, hk), j in ac.needle_keys(ac.get_case(n)).items() if s == 0}
    assert seen == set(ac.decode_positions(8192, 64, 512))
    long = {j for (s, p, hk), j in ac.needle_keys(ac.get_case("pre_long")).items() if s == 0}
    assert long >= {4095, 4096, 8191, 8192}  # both sides of flash_d128's block-id register seams
    rows = {(s, p) for s, p, hk in ac.needle_keys(ac.get_case("pre_g2"))}
    assert {(0, i) for i in (0, 127, 128, 255, 256, 383, 384, 519)} <= rows


def _random_decode(ctx, Hq=32, Hkv=8, D=128, bs=64):
    g = torch.Generator().manual_seed(0)
    nblk = [-(-c // bs) for c in ctx]
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)  # noqa: E731
    bt = torch.zeros(len(ctx), max(nblk), dtype=torch.int32)
    perm, o = torch.randperm(sum(nblk), generator=g), 0
    for b, nb in enumerate(nblk):
        bt[b, :nb] = perm[o:o + nb].to(torch.int32)
        o += nb
    return ac.Case("decode", rnd(len(ctx), Hq, D), rnd(sum(nblk), Hkv, bs, D), rnd(sum(nblk), Hkv, bs, D), [1] * len(ctx),
                   list(ctx), False, 1 / math.sqrt(D), bt, bs)


def test_random_8k_is_blind():
    """On randn inputs at the 8K contexts of test_paged_decode_8k_context, an oracle that never reads
    the last key of a sequence (the token just written) passes ``close(atol=2e-2, rtol=2e-2)`` against
    the right oracle: the output RMS there (about 0.02 at 8192 keys) is the size of the tolerance, and
    one key in thousands moves most rows by less than a bf16 rounding -- what the needles are for.
    The signal-relative check sees the mutants that move 56-64 keys (a skipped tile, the random tail of
    the last block read as keys)."""
    case = _random_decode([8192, 5000, 4097, 2048])
    good = ac.run(case, ops)
    rep = ac.check(case, good)
    assert rep.ok and rep.f < 3.5e-3, str(rep)
    assert good.float().pow(2).mean().sqrt() < 4e-2
    bad = mutant(case, "ctx-1")
    assert not torch.equal(bad, good)
    assert torch.allclose(bad.float(), good.float(), atol=2e-2, rtol=2e-2) and ac.check(case, bad).close_ok
    for kind in ("skip-512", "tail"):
        assert ac.check(case, mutant(case, kind)).rel_bad, kind
