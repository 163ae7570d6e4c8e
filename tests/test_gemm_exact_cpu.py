"""The GEMM harness of tests/gemm_cases.py proves itself on the CPU: the fp32 oracle (ops/reference.py's
arithmetic writing through the same guarded views) passes every case of tests/test_gemm_exact_gpu.py, so
equality -- and one bf16 ulp for GELU / SwiGLU -- is reachable; the tables reach every class of
gemm_mid's work decomposition and every dispatch arm; and the oracle with one planted mistake, the
mistakes a GEMM kernel makes, is rejected by the cases each test names.

Why this module exists: on the operands the GEMM tests had (``randn`` activations, ``0.05 randn`` weights,
``close(atol=3e-2, rtol=2e-2)``) a truncating bf16 store and a residual added before the rounding both
pass; ``test_old_recipe_is_blind`` keeps that on record.
"""
import pytest
import torch

import gemm_cases as gc
from django_assistant_bot_amd import ops
from django_assistant_bot_amd.ops import reference as ref

BF = torch.bfloat16
ORACLE = gc.oracle()
CPU = "cpu"


def _ok(reps, limit=0.51):
    """Equality where the contract fixes every bit; GELU / SwiGLU: an fp32 epilogue on an exact
    accumulator is the bf16 rounding (0.5 ulp) and a little more."""
    for rep in (reps.values() if isinstance(reps, dict) else [reps]):
        assert rep.ok and rep.n_bad == 0, str(rep)
        if any(f" {e}" in rep.name for e in gc.ACT):
            print(f"GEMM-ORACLE ratio={rep.ratio:.4f} {rep}")
            assert rep.ratio <= limit or " gelu" in rep.name, str(rep)
        else:
            assert rep.ratio == 0.0, str(rep)


def _rejected(reps):
    return [k for k, r in reps.items() if not r.ok] if isinstance(reps, dict) else ([] if reps.ok else [reps.name])


# ------------------------------------------------------------------------------------------------
# the oracle passes every case of the GPU module


@pytest.mark.parametrize("layout", gc.LAYOUTS)
@pytest.mark.parametrize("M,N,K", gc.BT_SHAPES)
def test_oracle_gemm_bt(M, N, K, layout):
    _ok(gc.run_jobs(ORACLE, CPU, "bt", M, N, K, layout, gc.BT_EPIS))
    _ok(gc.run_scores(ORACLE, CPU, M, N, K, layout))


@pytest.mark.parametrize("layout", gc.LAYOUTS)
@pytest.mark.parametrize("M,N,K", gc.BT_SWIGLU_SHAPES)
def test_oracle_gemm_bt_swiglu(M, N, K, layout):
    _ok(gc.run_jobs(ORACLE, CPU, "bt", M, N, K, layout, gc.BT_SWIGLU_EPIS))


@pytest.mark.parametrize("layout", gc.LAYOUTS)
def test_oracle_gemm_bt_256_tile(layout):
    assert gc.bt_big(*gc.BT_BIG[:2]) and gc.BT_BIG[1] % 256 and gc.BT_BIG[2] % 128
    _ok(gc.run_jobs(ORACLE, CPU, "bt", *gc.BT_BIG, layout, gc.BT_BIG_EPIS))


@pytest.mark.parametrize("layout", gc.LAYOUTS)
@pytest.mark.parametrize("M,N,K", gc.G256_SHAPES + (gc.G256_BIG,))
def test_oracle_gemm256(M, N, K, layout):
    _ok(gc.run_jobs(ORACLE, CPU, "g256", M, N, K, layout, gc.g256_epis(layout)))


@pytest.mark.parametrize("M,N,K", gc.MID_SHAPES)
def test_oracle_gemm_mid(M, N, K):
    _ok(gc.run_jobs(ORACLE, CPU, "mid", M, N, K, "shuf", gc.MID_EPIS))
    if (M, N, K) == gc.MID_GROUPED:
        _ok(gc.run_jobs(ORACLE, CPU, "mid", M, N, K, "shuf", gc.MID_EPIS, b_group=8))


def _one_cfg_per_tiling():
    """The oracle sees a configuration only through (N, layout, M limit): one configuration of each."""
    seen = {}
    for cfg in gc.STREAM_CFGS:
        seen.setdefault((gc.stream_n(cfg), gc.STREAM_CFG[cfg][2], gc.STREAM_CFG[cfg][1]), cfg)
    return sorted(seen.values())


@pytest.mark.parametrize("K,S", gc.STREAM_KS)
@pytest.mark.parametrize("cfg", _one_cfg_per_tiling())
def test_oracle_stream_gemm(cfg, K, S):
    for M in gc.stream_ms(cfg):
        _ok(gc.run_stream(ORACLE, CPU, cfg, M, K, S))


# ------------------------------------------------------------------------------------------------
# the tables reach what they claim


def test_gemm_mid_table_reaches_every_decomposition_class():
    """gn = 8 floor(32 / tiles_m) groups share tiles_n K / BK = q gn + r iterations: no whole iteration
    per group, no remainder, a remainder, and column tiles held by 1, 2 and 3 or more groups -- for the
    64-deep K-step and for the 32-deep one."""
    assert sorted({-(-M // 128) for M in gc.MID_M}) == [1, 2, 3, 5, 8, 16, 17, 32]
    for bk in (64, 32):
        ds = [gc.mid_decomposition(M, N, K, bk) for M, N, K in gc.MID_SHAPES]
        assert all(d.gn == 8 * (32 // d.tiles_m) and d.tiles_n * d.kt == d.q * d.gn + d.r for d in ds)
        assert any(d.q == 0 for d in ds) and any(d.r == 0 for d in ds) and any(d.r != 0 and d.q for d in ds)
        segs = {s for d in ds for s in d.segments}
        assert 1 in segs and 2 in segs and max(segs) >= 3, (bk, segs)
        for d in ds:  # the segments of a tile tile its K range
            for t in range(d.tiles_n):
                rs = d.ranges(t)
                assert rs[0][0] == 0 and rs[-1][1] == d.kt * bk and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))
    kinds = {tuple(gc.mid_decomposition(M, N, K).segments) for M, N, K in gc.MID_BACK_TO_BACK}
    assert len(kinds) == 3  # three different decompositions share the workspace back to back


def test_stream_table_matches_the_extension():
    nat = ops.native()
    for cfg in range(64):
        bn = nat.stream_gemm_bn(cfg)
        if cfg in gc.STREAM_CFG:
            assert gc.STREAM_CFG[cfg] == (bn, nat.stream_gemm_max_m(cfg), bool(nat.stream_gemm_shuffled(cfg))), cfg
        else:
            assert bn == 0 or cfg in gc.STREAM_ABLATIONS, f"configuration {cfg} is in no table"
    assert set(gc.STREAM_PRODUCTION) <= set(gc.STREAM_CFG) and {24, 26} <= set(gc.STREAM_CFG)
    for cfg in gc.STREAM_CFGS:
        assert gc.stream_n(cfg) % 32 == 0 and max(gc.stream_ms(cfg)) == gc.STREAM_CFG[cfg][1]
    assert {K // (128 * S) for K, S in gc.STREAM_KS} == {1, 3, 5}  # one K-step per slice; rings that do and do not fill


def test_dispatch_table_follows_the_documented_rule():
    assert {arm for *_, arm in gc.DISPATCH} == set(gc.ARMS)
    for layout, M, N, K, arm in gc.DISPATCH:
        lda = gc._stride(K, gc.A_PAD)
        assert gc.documented_arm(layout, M, N, K, lda) == arm, (layout, M, N, K)
        mid = layout == "shuf" and ops.kernels.use_gemm_mid(M, N, K, lda)
        g256 = not mid and ops.kernels.use_gemm256(M, N, K, lda, K if layout == "shuf" else lda)
        assert (mid, g256) == (arm == "mid", arm.startswith("g256")), (layout, M, N, K)


def test_gemm256_table():
    nat = ops.native()
    for M, N, K in gc.G256_SHAPES + (gc.G256_BIG,):
        assert nat.gemm256_ok(M, N, K, gc._stride(K, gc.A_PAD), K)
    M, N, _ = gc.G256_BIG
    assert -(-M // 256) * (N // 256) > 256 and M % 256  # more tiles than CUs, a ragged last row tile
    assert not nat.gemm256_ok(*gc.BT_BIG, gc.BT_BIG[2], gc.BT_BIG[2])


def test_decisive_shares():
    """The shares the operand recipe gives (the builders assert the 1 % floors on every case)."""
    for K, lo in ((64, 0.01), (256, 0.05), (4096, 0.15)):
        c = gc.exact_case(300, 256, K)
        C, b, r = c.C.double(), c.bias.double(), c.res.double()
        trunc = gc._share(gc.round_bf16(C), gc.trunc_bf16(C))
        early = gc._share(gc.round_bf16(gc.round_bf16(C) + r), gc.round_bf16(C + r))
        late = gc._share(gc.round_bf16(C + b), gc.round_bf16(gc.round_bf16(C) + b))
        print(f"GEMM-SHARES K={K} inexact={gc._share(gc.round_bf16(C), C):.3f} trunc={trunc:.3f} "
              f"res-early={early:.3f} bias-late={late:.3f} max|C|={float(C.abs().max()):.0f}")
        assert min(trunc, early, late) >= lo
    C = gc.exact_case(64, 256, 14336).C
    assert float(C.abs().max()) < 2 ** 24


def test_checker_units():
    x = torch.randn(4096, dtype=torch.float64) * 300
    assert torch.equal(gc.trunc_bf16(x), gc._trunc32(x.float()).double())
    assert torch.equal(gc.round_bf16(x), x.float().to(BF).double())
    E = torch.tensor([[1.0, -2.0]], dtype=BF)
    assert gc.check_same("", E.clone(), E).ratio == 0.0 and not gc.check_same("", E + 1, E).ok
    assert not gc.check_same("", torch.tensor([[1.0, float("nan")]], dtype=BF), E).ok
    buf, out = gc.out_view(3, 8, CPU)
    assert gc.untouched(buf, 3, 8) and out.stride(0) == 24
    gc._past(out, cols=1)[0, 8] = 0.0
    assert not gc.untouched(buf, 3, 8)
    w = torch.arange(48 * 64, dtype=torch.float32).reshape(48, 64).to(BF)
    v, view = gc.shuffled_copy(w[:40], CPU)
    assert view.is_contiguous() and view.shape == (48, 64) and bool(torch.isnan(v[:16]).all() and torch.isnan(v[-16:]).all())
    u = ops.unshuffle_weights(view)
    assert torch.equal(u[:40], w[:40]) and bool(torch.isnan(u[40:]).all())


# ------------------------------------------------------------------------------------------------
# planted mistakes


def _bt(defect, M, N, K, layout, epis):
    return gc.run_jobs(gc.oracle(defect), CPU, "bt", M, N, K, layout, epis)


def _g256(defect, M, N, K, layout, epis):
    return gc.run_jobs(gc.oracle(defect), CPU, "g256", M, N, K, layout, epis)


def _mid(defect, M, N, K, epis=gc.MID_EPIS, **kw):
    return gc.run_jobs(gc.oracle(defect), CPU, "mid", M, N, K, "shuf", epis, **kw)


def _stream(defect, cfg, M, K, S):
    return gc.run_stream(gc.oracle(defect), CPU, cfg, M, K, S)


def test_rejects_a_truncating_store():
    """Every bf16 store; the fp32 output and the slabs have none."""
    for layout in gc.LAYOUTS:
        assert _rejected(_bt("trunc", 127, 132, 64, layout, gc.EXACT)) == list(gc.PLAIN)
        assert _rejected(_bt("trunc", 1, 4, 64, layout, gc.EXACT)) == list(gc.PLAIN)
        assert _rejected(_g256("trunc", 255, 256, 128, layout, gc.PLAIN)) == list(gc.PLAIN)
    assert _rejected(_mid("trunc", 129, 256, 64, ("none", "residual"))) == ["none", "residual"]
    # (SwiGLU is held to one ulp, and a truncation is less than one)
    assert _rejected(_stream("trunc", 10, 17, 128, 1)) == ["none", "residual"]
    assert _rejected(_stream("trunc", 10, 17, 256, 2)) == ["reduce_none", "reduce_residual"]


def test_rejects_a_residual_added_before_the_rounding():
    for layout in gc.LAYOUTS:
        assert _rejected(_bt("res-early", 127, 132, 64, layout, gc.EXACT)) == ["residual", "bias_residual"]
        assert _rejected(_g256("res-early", 257, 256, 128, layout, gc.PLAIN)) == ["residual", "bias_residual"]
    assert _rejected(_bt("res-early", 1, 4, 64, "rm", gc.PLAIN)) == ["residual", "bias_residual"]
    assert _rejected(_mid("res-early", 129, 256, 64)) == ["residual"]
    assert _rejected(_stream("res-early", 13, 16, 640, 1)) == ["residual"]
    assert _rejected(_stream("res-early", 13, 16, 1536, 4)) == ["reduce_residual"]


def test_rejects_a_bias_added_after_the_rounding():
    for layout in gc.LAYOUTS:
        assert _rejected(_bt("bias-late", 127, 132, 64, layout, gc.BT_EPIS)) == ["bias", "bias_residual"]
        assert _rejected(_bt("bias-late", 1, 4, 64, layout, gc.BT_EPIS)) == ["bias", "bias_residual"]
        assert _rejected(_g256("bias-late", 513, 512, 384, layout, gc.PLAIN)) == ["bias", "bias_residual"]


def test_rejects_a_bias_indexed_by_the_row():
    for layout in gc.LAYOUTS:
        assert _rejected(_bt("bias-by-m", 127, 132, 64, layout, gc.BT_EPIS)) == ["bias", "bias_residual", "gelu"]
        assert _rejected(_bt("bias-by-m", 127, 160, 64, layout, gc.BT_SWIGLU_EPIS)) == ["swiglu_bias"]
    assert _rejected(_bt("bias-by-m", 1, 4, 64, "rm", gc.BT_EPIS)) == ["bias", "bias_residual", "gelu"]
    assert _rejected(_g256("bias-by-m", 257, 512, 128, "rm", gc.g256_epis("rm"))) == [
        "bias", "bias_residual", "gelu", "swiglu_bias"]


@pytest.mark.parametrize("defect", ["k-last", "k-chunk-twice"])
def test_rejects_a_wrong_k_range(defect):
    """The last K element dropped; one 32-deep chunk read in place of its neighbour: every output of
    every kernel (the oracle's EPI_SCORES path takes no planted K range)."""
    for layout in gc.LAYOUTS:
        for shape in gc.BT_SHAPES:
            assert _rejected(_bt(defect, *shape, layout, gc.BT_EPIS)) == list(gc.BT_EPIS)
        assert _rejected(_bt(defect, 127, 160, 64, layout, gc.BT_SWIGLU_EPIS)) == list(gc.BT_SWIGLU_EPIS)
        assert _rejected(_g256(defect, 255, 256, 128, layout, gc.g256_epis(layout))) == list(gc.g256_epis(layout))
    assert _rejected(_mid(defect, 300, 768, 320)) == list(gc.MID_EPIS)
    assert _rejected(_stream(defect, 20, 127, 128, 1)) == ["none", "residual", "swiglu8"]
    assert _rejected(_stream(defect, 20, 127, 2048, 16)) == ["slabs", "reduce_none", "reduce_residual"]


def test_rejects_a_segment_left_out_of_the_combine():
    for M, N, K in ((300, 768, 1024), (2100, 256, 320), (1, 256, 1024), (1000, 768, 320)):
        assert max(gc.mid_decomposition(M, N, K).segments) > 1
        assert _rejected(_mid("mid-drop-segment", M, N, K)) == list(gc.MID_EPIS)
    assert gc.mid_decomposition(4096, 768, 64).segments == [1, 1, 1]  # no split tile: nothing to leave out
    assert _rejected(_mid("mid-drop-segment", 4096, 768, 64)) == []
    # the 32-deep K-step splits where the 64-deep one does not
    assert gc.mid_decomposition(4096, 768, 64, 32).segments == [2, 2, 2]
    assert _rejected(_mid("mid-drop-segment", 4096, 768, 64, variant=32)) == list(gc.MID_EPIS)


def test_rejects_a_skipped_slab():
    for cfg, M, K, S in ((10, 17, 256, 2), (30, 16, 1536, 4), (27, 255, 2048, 16)):
        assert _rejected(_stream("slab-skip", cfg, M, K, S)) == ["reduce_none", "reduce_residual"]


def test_rejects_swiglu_over_16_row_groups_where_8_were_asked():
    for layout in gc.LAYOUTS:
        assert _rejected(_bt("swiglu-16-for-8", 127, 160, 64, layout, gc.BT_SWIGLU_EPIS)) == ["swiglu8"]
        assert _rejected(_g256("swiglu-16-for-8", 255, 256, 128, layout, gc.g256_epis(layout))) == ["swiglu8"]
    assert _rejected(_mid("swiglu-16-for-8", 129, 256, 64)) == ["swiglu8"]
    assert _rejected(_stream("swiglu-16-for-8", 20, 17, 128, 1)) == ["swiglu8"]


@pytest.mark.parametrize("defect", ["a-row+1", "b-row+1"])
def test_rejects_a_read_past_an_operand(defect):
    """The row behind the last valid row of A; the first padding row of the fragment-layout copy (the
    guard row behind a row-major B) in place of B's last row: NaN in a valid output."""
    for layout in gc.LAYOUTS:
        for shape in gc.BT_SHAPES:
            assert _rejected(_bt(defect, *shape, layout, gc.BT_EPIS)) == list(gc.BT_EPIS)
            assert not gc.run_scores(gc.oracle(defect), CPU, *shape, layout).ok
        assert _rejected(_g256(defect, 257, 256, 128, layout, gc.PLAIN)) == list(gc.PLAIN)
    assert _rejected(_mid(defect, 129, 256, 64)) == list(gc.MID_EPIS)
    assert _rejected(_stream(defect, 0, 17, 128, 1)) == ["none", "residual", "swiglu", "swiglu8"]
    assert _rejected(_stream(defect, 10, 17, 256, 2)) == ["slabs", "reduce_none", "reduce_residual"]


@pytest.mark.parametrize("defect", ["row-past-m", "col-past-n"])
def test_rejects_a_write_outside_the_output(defect):
    for layout in gc.LAYOUTS:
        for shape in gc.BT_SHAPES:
            reps = _bt(defect, *shape, layout, gc.BT_EPIS)
            assert _rejected(reps) == list(gc.BT_EPIS) and all("outside the output view" in r.name for r in reps.values())
            assert "outside the output view" in gc.run_scores(gc.oracle(defect), CPU, *shape, layout).name
        assert _rejected(_g256(defect, 255, 512, 128, layout, gc.g256_epis(layout))) == list(gc.g256_epis(layout))
    assert _rejected(_mid(defect, 2100, 256, 64)) == list(gc.MID_EPIS)
    assert _rejected(_stream(defect, 32, 15, 128, 1)) == ["none", "residual", "swiglu8"]
    assert _rejected(_stream(defect, 32, 15, 256, 2)) == ["reduce_none", "reduce_residual"]


# ------------------------------------------------------------------------------------------------
# the blind spot


@pytest.mark.parametrize("K", [64, 1024, 4096, 14336])
def test_old_recipe_is_blind(K):
    """``randn`` activations, ``0.05 randn`` weights, ``close(atol=3e-2, rtol=2e-2)`` against the fp32
    reference: a truncating bf16 store and a residual added to the fp32 accumulator both pass (and both
    differ from the reference in many elements)."""
    g = torch.Generator().manual_seed(K)
    M, N = 64, 256
    A, B = torch.randn(M, K, generator=g).to(BF), (0.05 * torch.randn(N, K, generator=g)).to(BF)
    res = torch.randn(M, N, generator=g).to(BF)
    old = lambda a, b: torch.allclose(a.float(), b.float(), atol=3e-2, rtol=2e-2)  # noqa: E731
    c = A.float() @ B.float().t()
    good, good_r = ref.gemm_bt(A, B), ref.gemm_bt(A, B, None, res)
    trunc, early = gc._trunc32(c), (c + res.float()).to(BF)
    assert old(trunc, good) and old(early, good_r)
    assert float((trunc != good).float().mean()) > 0.3 and float((early != good_r).float().mean()) > 0.05
