"""The row-kernel harness of tests/rowwise_cases.py proves itself on the fp32 oracle (``ops.*`` on CPU
tensors runs ops/reference.py): the oracle stays inside every bound of every case of
tests/test_rowwise_gpu.py, with ``a_row <= 2^-12 max|E_row|`` on the cancelling ops, so the bounds are
reachable; and torch emulations with one planted defect each -- the mistakes row kernels make -- are
rejected, on the row built for that defect.

Why this module exists: three of those defects pass ``close(atol=2e-2, rtol=2e-2)`` on ``randn`` rows,
the check the kernel tests had; ``test_old_tolerance_is_blind`` keeps that on record.
"""
from types import SimpleNamespace

import pytest
import torch

import rowwise_cases as rc
from django_assistant_bot_amd import ops
from django_assistant_bot_amd.ops import reference as ref

BF = torch.bfloat16
DTYPES = [torch.float32, BF]
ids = lambda v: str(v).replace("torch.", "")  # noqa: E731


def _ok(rep, limit=0.51):
    """fp32 math: one bf16 rounding of the result (0.5 ulp) and a little of the margin."""
    assert rep.ok and rep.n_bad == 0, str(rep)
    assert rep.ratio <= limit, str(rep)
    assert rep.a_rel is None or rep.a_rel <= rc.A_COND


# ------------------------------------------------------------------------------------------------
# the oracle passes every case of the GPU module


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("cols", rc.RMSNORM_COLS)
def test_oracle_rmsnorm(cols, residual):
    _ok(rc.run_rmsnorm(ops, "cpu", cols, residual))


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("cols,S", rc.SLAB_CASES)
def test_oracle_rmsnorm_slabs(cols, S, dtype, residual):
    _ok(rc.run_rmsnorm_slabs(ops, "cpu", cols, S, dtype, residual))


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("cols", rc.LN_COLS)
def test_oracle_layernorm(cols, residual):
    _ok(rc.run_layernorm(ops, "cpu", cols, residual))


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("cols,rows", rc.LN_WAVE)
def test_oracle_layernorm_wave_widths(cols, rows, residual):
    _ok(rc.run_layernorm(ops, "cpu", cols, residual, (rows,)))


@pytest.mark.parametrize("types", ["none", "ones", "mixed"])
@pytest.mark.parametrize("H", rc.EMBED_H)
def test_oracle_bert_embed(H, types):
    _ok(rc.run_bert_embed(ops, "cpu", H, types))


@pytest.mark.parametrize("cols", rc.GATHER_COLS)
def test_oracle_embed_gather(cols):
    assert rc.run_embed_gather(ops, "cpu", cols).ratio == 0.0


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("H", rc.POOL_H)
def test_oracle_mean_pool(H, normalize):
    _ok(rc.run_mean_pool(ops, "cpu", H, normalize), 1.0)  # (the oracle is its own a_row: at most 2^-22 |E| + 4 a_row)


def _sequential_pool(hidden, cu, normalize=False, want_bf16=False):
    """mean_pool in the kernel's order: tokens added one by one in fp32, times 1 / n, x rsqrt(sum sq)."""
    cu = cu.tolist()
    out = torch.zeros(len(cu) - 1, hidden.shape[1])
    for b in range(len(cu) - 1):
        acc = torch.zeros(hidden.shape[1])
        for t in range(cu[b], cu[b + 1]):
            acc = acc + hidden[t].float()
        if cu[b + 1] > cu[b]:
            out[b] = acc * (torch.tensor(1.0) / (cu[b + 1] - cu[b]))
    if normalize:
        tot = (out * out).sum(-1, keepdim=True)
        out = torch.where(tot > 0, out * torch.rsqrt(tot), torch.zeros_like(out))
    return out, out.to(BF)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("H", [8, 2056])
def test_mean_pool_bound_admits_the_sequential_order(H, normalize):
    """The margin is there for another valid summation order: the kernel's (512 tokens one by one,
    where torch sums in a tree) stays inside it."""
    rep = rc.run_mean_pool(SimpleNamespace(mean_pool=_sequential_pool), "cpu", H, normalize)
    assert rep.ok, str(rep)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("rows,cols", rc.GELU_SHAPES + (rc.BIG, rc.BIG_ODD))
def test_oracle_gelu(rows, cols, bias):
    if (rows, cols) in (rc.BIG, rc.BIG_ODD) and not bias:
        return  # (the GPU module runs the grid-stride shape with bias only)
    _ok(rc.run_gelu(ops, "cpu", rows, cols, bias), 0.75)  # torch's 0.5 x (1 + erf) cancels: a quarter ulp at -3.5


@pytest.mark.parametrize("rows,F", [(r, F) for F in rc.SILU_F for r in rc.ROWS] + [rc.BIG])
def test_oracle_silu_mul(rows, F):
    _ok(rc.run_silu_mul(ops, "cpu", rows, F))


def test_oracle_silu_sweep():
    gate, _ = rc.silu_sweep_inputs()
    assert float(gate.float().min()) == -120.0 and float(gate.float().max()) == 120.0 and gate.shape[1] > 34000
    _ok(rc.run_silu_sweep(ops, "cpu"))


@pytest.mark.parametrize("geom", rc.ROPE_GEOM, ids=lambda g: "-".join(map(str, g)))
def test_oracle_rope(geom):
    _ok(rc.run_rope(ops, "cpu", rc.rope_inputs(*geom)), 0.6)  # two fp32 roundings under a cancelling difference
    _ok(rc.run_rope(ops, "cpu", rc.rope_inputs(*geom), write_q=False), 0.6)
    assert rc.run_rope(ops, "cpu", rc.rope_inputs(*geom, slots="all")).ok
    assert rc.run_rope(ops, "cpu", rc.rope_inputs(*geom, exact=True), exact=True).ratio == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("S", rc.ROPE_SLAB_S)
@pytest.mark.parametrize("D", [64, 128])
def test_oracle_rope_slabs(D, S, dtype):
    _ok(rc.run_rope(ops, "cpu", rc.rope_inputs(D, 4, 2, 16, 9, S=S, dtype=dtype)), 0.6)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("M,N", rc.REDUCE_SHAPES)
@pytest.mark.parametrize("S", rc.REDUCE_S)
def test_oracle_slab_reduce(S, M, N, dtype, residual):
    _ok(rc.run_slab_reduce(ops, "cpu", S, M, N, dtype, residual))


def test_parametrisation_reaches_every_arm():
    """Read against DAB_ROW_DISPATCH: every (NT, VPT) arm is taken by rmsnorm, the generic layernorm,
    bert_embed and the slab kernel, which takes its <512, 1> launch where the others take (256, 2); the
    slab counts run the 8-, 4- and 1-slab loops in every mix."""
    arms = {(64, 1), (128, 1), (256, 1), (256, 2), (256, 4), (256, 8)}
    assert {rc.row_arm(c) for c in rc.RMSNORM_COLS} == arms
    assert {rc.row_arm(c) for c in rc.LN_COLS} == arms
    assert {rc.row_arm(c, True) for c in rc.SLAB_COLS} == arms - {(256, 2)} | {(512, 1)}
    assert {rc.row_arm(c) for c in rc.EMBED_H} == arms
    assert {(S // 8 > 0, S % 8 // 4 > 0, S % 4 > 0) for S in rc.SLAB_S} == {
        (False, False, True), (False, True, False), (False, True, True), (True, False, False), (True, False, True),
        (True, True, False), (True, True, True)}
    assert {(S // 4 > 0, S % 4 > 0) for S in rc.ROPE_SLAB_S} == {(False, True), (True, False), (True, True)}
    assert rc.BIG[0] * rc.BIG[1] // 8 > 8192 * 256  # both grid-stride loops take a second pass
    assert rc.BIG_ODD[0] * rc.BIG_ODD[1] // 8 > 8192 * 256 and (8192 * 256) % (rc.BIG_ODD[1] // 8)
    assert max(rc.POOL_H) > 2048  # mean_pool's second vector per thread


# ------------------------------------------------------------------------------------------------
# planted mistakes


def _rmsnorm_with(defect):
    def rmsnorm(x, w, eps, residual=None):
        if x.dim() == 3:
            if defect == "slab-tail" and x.shape[0] % 4:  # the 1-slab tail loop stops one short
                x = x[:-1]
            x = x.float().sum(0).to(BF)
        xf, res = x.float(), None
        if residual is not None:
            xf = (xf + residual.float()).to(BF).float()
            res = xf.to(BF)
        sq = xf.pow(2)
        if defect == "last-vector":  # the sum of squares loses the row's last 16-byte vector
            sq = sq[..., :-8]
        ms = sq.sum(-1, keepdim=True) / x.shape[-1]
        inv = {"no-eps": lambda: torch.rsqrt(ms), "eps-after-sqrt": lambda: 1.0 / (ms.sqrt() + eps)}.get(
            defect, lambda: torch.rsqrt(ms + eps))()
        return (xf * inv * w.float()).to(BF), res
    return SimpleNamespace(rmsnorm=rmsnorm)


def _needle_rows(cols, nt, first, at):
    pos = rc.needle_positions(cols, nt)
    return {first + i for i, p in enumerate(pos) if p in at}


@pytest.mark.parametrize("cols", [264, 2056, 8200])
def test_rejects_a_dropped_last_vector(cols):
    rep = rc.run_rmsnorm(_rmsnorm_with("last-vector"), "cpu", cols, False)
    assert not rep.ok and rep.row in _needle_rows(cols, rc.row_threads(cols), 4, (cols - 8, cols - 1)), str(rep)
    assert rep.ratio > 50
    assert not rc.run_rmsnorm(_rmsnorm_with("last-vector"), "cpu", cols, True).ok


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("cols,S", [(4096, 5), (4104, 13), (64, 13), (4096, 21)])
def test_rejects_a_skipped_slab(cols, S, dtype):
    assert S % 4
    for residual in (False, True):
        rep = rc.run_rmsnorm_slabs(_rmsnorm_with("slab-tail"), "cpu", cols, S, dtype, residual)
        assert not rep.ok, str(rep)
    assert rc.run_rmsnorm_slabs(_rmsnorm_with("slab-tail"), "cpu", 4096, 8, dtype, False).ok  # S % 4 == 0: no defect


@pytest.mark.parametrize("defect", ["no-eps", "eps-after-sqrt"])
@pytest.mark.parametrize("cols", [8, 2048, 16384])
def test_rejects_a_wrong_eps(cols, defect):
    for residual in (False, True):
        rep = rc.run_rmsnorm(_rmsnorm_with(defect), "cpu", cols, residual)
        assert not rep.ok and rep.row in (2, 3), str(rep)  # the rows whose mean square is under eps
    c = rc.slab_case(4096, 13, torch.float32, False)
    rep = rc.run_rmsnorm_slabs(_rmsnorm_with(defect), "cpu", 4096, 13, torch.float32, False)
    assert not rep.ok and rep.row == 2 and float(c.x.sum(0)[2].pow(2).mean()) < rc.RMS_EPS, str(rep)  # the sparse row


def test_old_tolerance_is_blind():
    """The gap this harness closes, written down: on the ``randn`` row the same wrong outputs pass
    ``close(atol=2e-2, rtol=2e-2)`` against the oracle -- a lost vector or eps moves a unit-variance
    row by about 0.1 %.  (A skipped slab does not: it takes 1 / sqrt(S) of every element's spread with
    it, which that tolerance sees.  Its gap was coverage: S = 1 and 3 never enter the unrolled loops.)"""
    old = lambda a, b: torch.allclose(a.float(), b.float(), atol=2e-2, rtol=2e-2)  # noqa: E731
    for cols in (2056, 8200):
        c = rc.rms_case(cols, False)
        x = c.x[:1]
        good, _ = ref.rmsnorm(x, c.w, rc.RMS_EPS)
        for defect in ("last-vector", "no-eps"):
            bad, _ = _rmsnorm_with(defect).rmsnorm(x, c.w, rc.RMS_EPS)
            assert old(bad, good), defect
        assert not torch.equal(_rmsnorm_with("last-vector").rmsnorm(x, c.w, rc.RMS_EPS)[0], good)
    c = rc.slab_case(4104, 13, torch.float32, False)
    good, _ = ops.rmsnorm(c.x[:, :1], c.w, rc.RMS_EPS)
    bad, _ = _rmsnorm_with("slab-tail").rmsnorm(c.x[:, :1], c.w, rc.RMS_EPS)
    assert not old(bad, good)


def _ln_sumsq(x, gamma, beta, eps, residual=None):
    """Variance as E[x^2] - mean^2 in fp32 (one pass)."""
    v = x.float() if residual is None else x.float() + residual.float()
    mean = v.mean(-1, keepdim=True)
    var = (v * v).mean(-1, keepdim=True) - mean * mean
    return ((v - mean) * torch.rsqrt(var + eps) * gamma.float() + beta.float()).to(BF)


@pytest.mark.parametrize("cols", [520, 1024, 8200])
def test_rejects_a_one_pass_variance(cols):
    rep = rc.run_layernorm(SimpleNamespace(layernorm=_ln_sumsq), "cpu", cols, False)
    assert not rep.ok and rep.row == 1, str(rep)  # the 100 + randn row


@pytest.mark.parametrize("H", rc.EMBED_H[:3])
def test_rejects_ignored_type_ids(H):
    impl = SimpleNamespace(bert_embed=lambda i, p, t, *a: ref.bert_embed(i, p, None, *a))
    assert rc.run_bert_embed(impl, "cpu", H, "none").ok
    for types in ("ones", "mixed"):
        assert not rc.run_bert_embed(impl, "cpu", H, types).ok


def _pool_with(defect):
    def mean_pool(hidden, cu, normalize=False, want_bf16=False):
        cu_l = cu.tolist()
        out = torch.zeros(len(cu_l) - 1, hidden.shape[1])
        for b in range(len(cu_l) - 1):
            s, e = cu_l[b], cu_l[b + 1]
            if e > s:
                if defect == "len+1":
                    out[b] = hidden[s:e].float().sum(0) / (e - s + 1)
                else:  # the range runs one token into the neighbour
                    out[b] = hidden[s:min(e + 1, hidden.shape[0])].float().sum(0) / (e - s)
        if normalize:
            out = torch.nn.functional.normalize(out, dim=-1)
        return out, out.to(BF)
    return SimpleNamespace(mean_pool=mean_pool)


@pytest.mark.parametrize("H", [8, 4096])
def test_rejects_wrong_pooling(H):
    assert not rc.run_mean_pool(_pool_with("len+1"), "cpu", H, False).ok
    for normalize in (False, True):
        assert not rc.run_mean_pool(_pool_with("neighbour"), "cpu", H, normalize).ok


def _rope_with(defect):
    def rope_kv_write(qkv, positions, cos_sin, k_cache, v_cache, slots, Hq, Hkv, D, write_q=True):
        if qkv.dim() == 3:
            qkv = qkv.float().sum(0).to(BF)
        if defect == "sin-sign":
            cos_sin = cos_sin * torch.tensor([1.0, -1.0])
            return ref.rope_kv_write(qkv, positions, cos_sin, k_cache, v_cache, slots, Hq, Hkv, D, k_cache.shape[2])
        # pairs (i, i + 1) in place of (i, i + D / 2): the same rotation on an even / odd de-interleaved copy
        T = qkv.shape[0]
        x = qkv.view(T, Hq + 2 * Hkv, D)
        perm = torch.cat([torch.arange(0, D, 2), torch.arange(1, D, 2)])
        xp = x.clone()
        xp[:, :Hq + Hkv] = x[:, :Hq + Hkv][..., perm]
        kc, vc = k_cache.clone(), v_cache.clone()
        q = ref.rope_kv_write(xp.reshape(T, -1), positions, cos_sin, kc, vc, slots, Hq, Hkv, D, k_cache.shape[2])
        inv = torch.argsort(perm)
        k_cache.copy_(kc[..., inv])
        v_cache.copy_(vc)
        return q[..., inv].contiguous()
    return SimpleNamespace(rope_kv_write=rope_kv_write)


@pytest.mark.parametrize("defect", ["sin-sign", "pair-i-i+1"])
@pytest.mark.parametrize("geom", rc.ROPE_GEOM[:3], ids=lambda g: "-".join(map(str, g)))
def test_rejects_wrong_rope(geom, defect):
    assert not rc.run_rope(_rope_with(defect), "cpu", rc.rope_inputs(*geom)).ok
    # ... and in the k cache alone
    assert not rc.run_rope(_rope_with(defect), "cpu", rc.rope_inputs(*geom), write_q=False).ok
    assert not rc.run_rope(_rope_with(defect), "cpu", rc.rope_inputs(*geom, exact=True), exact=True).ok


def _silu_wrong_chunk(x, interleaved=False, group=None):
    """The interleaved layout read with the two 8-column chunks of every up group swapped."""
    if interleaved:
        v = x.reshape(*x.shape[:-1], -1, 2, 2, 8)
        x = torch.stack([v[..., 0, :, :], v[..., 1, :, :].flip(-2)], -3).reshape(x.shape)
    return ops.silu_mul(x, interleaved=interleaved)


@pytest.mark.parametrize("rows,F", [(1, 16), (9, 1424)])
def test_rejects_a_wrong_swiglu_chunk(rows, F):
    rep = rc.run_silu_mul(SimpleNamespace(silu_mul=_silu_wrong_chunk), "cpu", rows, F)
    assert not rep.ok and "interleaved" in rep.name, str(rep)


def _reduce_residual_first(slabs, residual=None, out=None):
    y = slabs.float().sum(0)
    return (y if residual is None else y + residual.float()).to(BF)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_rejects_a_residual_added_before_the_rounding(dtype):
    impl = SimpleNamespace(slab_reduce=_reduce_residual_first)
    rep = rc.run_slab_reduce(impl, "cpu", 16, 37, 4096, dtype, True)
    assert not rep.ok and rep.row % 2 == 1, str(rep)  # a row whose residual cancels the sum
    assert rc.run_slab_reduce(impl, "cpu", 16, 37, 4096, dtype, False).ok


def test_checker_units():
    E = torch.tensor([[1.0, 1.5, -2.0, 0.0, 0.99, 2.0 ** -110]], dtype=torch.float64)
    assert rc.ulp(E).tolist() == [[2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -107, 2.0 ** -8, 2.0 ** -107]]
    x = torch.randn(4096, dtype=torch.float64) * 3
    assert torch.equal(rc.round_bf16(x), x.float().to(BF).double())
    ties = torch.tensor([1.00390625, 1.01171875], dtype=torch.float64)
    assert rc.round_bf16(ties).tolist() == [1.0, 1.015625]  # to even
    assert rc.check_ulp("", E + rc.ulp(E), E).ok and not rc.check_ulp("", E + 1.01 * rc.ulp(E), E).ok
    assert not rc.check_ulp("", torch.full_like(E, float("nan")), E).ok
    rep = rc.check_ulp("", torch.tensor([[0.0, 0.0], [0.0, 1.0]]), torch.zeros(2, 2), rows=torch.tensor([5, 7]))
    assert (rep.row, rep.col, rep.n_bad) == (7, 1, 1)
    with pytest.raises(AssertionError, match="badly conditioned"):  # a case cannot widen its own bound
        rc.check_margin("", E, E, E * (1 + 2.0 ** -11))
    assert rc.check_margin("", E, E, E * (1 + 2.0 ** -13)).ok
