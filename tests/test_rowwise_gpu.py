"""The memory-bound row kernels (norm.hip, elementwise.hip, ``slab_reduce``) against the fp64 references
of tests/rowwise_cases.py, on rows where one element, one slab or eps decides the output, at one bf16
rounding: ``|got - E| <= ulp(E)`` for rmsnorm (plain and slabs), gelu, silu_mul, rope_kv_write and
slab_reduce, ``ulp(E) + 4 a_row`` for layernorm, bert_embed and mean_pool (``2^-22 |E| + 4 a_row`` for
its fp32 output), equality for embed_gather and the residual stream.  tests/test_rowwise_cpu.py shows
on the CPU oracle that these bounds are reachable and that they reject the mistakes they are built for.

The parametrisation follows the launchers: every (NT, VPT) arm of DAB_ROW_DISPATCH once full and once
with a nearly empty last round, the slab kernel's <512, 1> launch and its 8- / 4- / 1-slab loops,
both layernorm_rows_kernel instantiations with a clamped last row, rope_chunk's U = 4 loop and tail,
mean_pool's second vector per thread, and the second pass of both grid-stride loops.

Largest observed |got - E| / bound per kernel on an MI355X (the bound is 1; 0.50 is the bf16 rounding
of an otherwise exact result):

    rmsnorm_kernel                     0.5000   (cols 264, the 2^-10 row)
    rmsnorm_slab_kernel                0.5000   (bf16 slabs, cols 1024, S 13); res_out equal everywhere
    layernorm_kernel                   0.5001   (cols 2056, the 100 + randn row; a_row / max|E| 5.6e-7)
    layernorm_rows_kernel              0.4999   (cols 1024, 8 rows)
    bert_embed_kernel                  0.4999   (H 384)
    embed_gather_kernel                0        (equal)
    mean_pool_kernel (fp32 output)     0.3613   (H 384, normalised, the 512-token sequence); bf16 copy <= 0.5
    gelu_kernel                        0.5247   (5450 x 3080 with bias; 0.5244 at 4100 x 4096)
    silu_mul_kernel                    0.5000   (both layouts; the sweep to +-120 included)
    rope_kv_kernel                     0.6484   (fp32 slabs, S 5, a q element); exact case: equal
    slab_reduce_kernel                 0.5000   (0 without a residual: the rounded sum itself)

With six in-bounds defects planted in norm.hip and elementwise.hip (the last vector out of rmsnorm's sum
of squares, the slab tail loop one short, the last shuffle step out of the wave kernel's variance,
mean_pool's second vector unscaled, the two grid-stride loops cut to one pass, the interleaved up chunk
swapped) exactly the tests that reach each defect failed: every rmsnorm width, the slab cases with
S % 4 != 0 and none with S in 4, 8, 12, 16, every wave-per-row case, mean_pool at H 2056 and 4096 only,
both second-pass tests, and every silu_mul case but the sweep (whose up values are constant).
"""
import pytest
import torch

import rowwise_cases as rc
from django_assistant_bot_amd import ops
from django_assistant_bot_amd.ops._lib import native, ptr, stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
DTYPES = [torch.float32, BF]
ids = lambda v: str(v).replace("torch.", "")  # noqa: E731


def _assert(rep, kernel):
    print(f"ROWWISE kernel={kernel!r} ratio={rep.ratio:.4f} {rep}")
    assert rep.ok, str(rep)
    return rep


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("cols", rc.RMSNORM_COLS)
def test_rmsnorm(cols, residual):
    _assert(rc.run_rmsnorm(ops, DEV, cols, residual), "rmsnorm")


@pytest.mark.parametrize("cols", rc.RMSNORM_BAD_COLS)
def test_rmsnorm_refuses_bad_widths_before_any_launch(cols):
    x, w = torch.ones(3, cols, dtype=BF, device=DEV), torch.ones(cols, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="rmsnorm"):
        ops.rmsnorm(x, w, rc.RMS_EPS)
    out = torch.full_like(x, rc.SENTINEL)
    with pytest.raises(RuntimeError, match="rmsnorm"):
        native().rmsnorm(ptr(out), 0, ptr(x), 0, ptr(w), 3, cols, rc.RMS_EPS, stream(x))
    slabs = torch.ones(2, 3, cols, device=DEV)
    with pytest.raises(RuntimeError, match="rmsnorm_slabs"):
        ops.rmsnorm(slabs, w, rc.RMS_EPS)
    torch.cuda.synchronize()
    assert bool((out == rc.SENTINEL).all())


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("cols,S", rc.SLAB_CASES)
def test_rmsnorm_slabs(cols, S, dtype, residual):
    _assert(rc.run_rmsnorm_slabs(ops, DEV, cols, S, dtype, residual), "rmsnorm_slabs")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("cols,S", [(4096, 13), (8200, 5)])
def test_rmsnorm_slabs_with_a_padded_slab_stride(cols, S, dtype):
    """A slab stride larger than rows * cols: the first ``rows`` of [S, rows + 2, cols] slabs, with 1e4 in
    the padding rows."""
    c = rc.slab_case(cols, S, dtype, True)
    rows = c.x.shape[1]
    buf = torch.full((S, rows + 2, cols), 1e4, dtype=dtype, device=DEV)
    buf[:, :rows] = c.x.to(DEV)
    r, w = c.r.to(DEV), c.w.to(DEV)
    out, res = torch.empty_like(r), torch.empty_like(r)
    native().rmsnorm_slabs(ptr(out), ptr(res), ptr(buf), S, (rows + 2) * cols, ptr(r), ptr(w), rows, cols, rc.RMS_EPS,
                           stream(buf), int(dtype == BF))
    _assert(rc.check_ulp(f"rmsnorm slabs padded stride cols {cols} S {S}", out, c.E), "rmsnorm_slabs")
    assert torch.equal(res.cpu(), c.Er)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("cols", rc.LN_COLS)
def test_layernorm_row_per_workgroup(cols, residual):
    _assert(rc.run_layernorm(ops, DEV, cols, residual), "layernorm_kernel")


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("cols,rows", rc.LN_WAVE)
def test_layernorm_wave_per_row(cols, rows, residual):
    """layernorm_rows_kernel<3 | 4, 2>: a workgroup takes 8 rows, so 1, 2, 3, 9 and 17 rows end in a
    clamped last row or an early break."""
    _assert(rc.run_layernorm(ops, DEV, cols, residual, (rows,)), "layernorm_rows_kernel")


@pytest.mark.parametrize("types", ["none", "ones", "mixed"])
@pytest.mark.parametrize("H", rc.EMBED_H)
def test_bert_embed(H, types):
    _assert(rc.run_bert_embed(ops, DEV, H, types), "bert_embed")


@pytest.mark.parametrize("cols", rc.GATHER_COLS)
def test_embed_gather(cols):
    assert _assert(rc.run_embed_gather(ops, DEV, cols), "embed_gather").ratio == 0.0


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("H", rc.POOL_H)
def test_mean_pool(H, normalize):
    _assert(rc.run_mean_pool(ops, DEV, H, normalize), "mean_pool")


def test_mean_pool_refuses_a_width_over_4096():
    h = torch.ones(4, 4104, dtype=BF, device=DEV)
    with pytest.raises(ValueError, match="4096"):
        ops.mean_pool(h, torch.tensor([0, 4], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("rows,cols", rc.GELU_SHAPES)
def test_gelu(rows, cols, bias):
    _assert(rc.run_gelu(ops, DEV, rows, cols, bias), "gelu")


@pytest.mark.parametrize("rows,cols", [rc.BIG, rc.BIG_ODD])
def test_gelu_grid_stride_second_pass(rows, cols):
    """2,099,200 vectors against a grid capped at 8192 x 256: the last 2048 take the stride loop's second
    pass, where ``i % cvec`` picks the bias (5450 x 3080: 385 vectors per row do not divide the stride).
    Every element is checked."""
    _assert(rc.run_gelu(ops, DEV, rows, cols, True), "gelu")


@pytest.mark.parametrize("rows,F", [(r, F) for F in rc.SILU_F for r in rc.ROWS])
def test_silu_mul(rows, F):
    _assert(rc.run_silu_mul(ops, DEV, rows, F), "silu_mul")


def test_silu_mul_grid_stride_second_pass():
    _assert(rc.run_silu_mul(ops, DEV, *rc.BIG), "silu_mul")


def test_silu_sweep():
    """Every bf16 gate in [-120, 120] against up = 1 and -3: ``1 + e^-x`` overflows under -88.7, where
    silu_f returns -0 for a true value under 2^-100 (the floor of ``ulp`` allows it)."""
    _assert(rc.run_silu_sweep(ops, DEV), "silu_mul")


@pytest.mark.parametrize("geom", rc.ROPE_GEOM, ids=lambda g: "-".join(map(str, g)))
def test_rope_kv_write(geom):
    _assert(rc.run_rope(ops, DEV, rc.rope_inputs(*geom)), "rope_kv_write")
    _assert(rc.run_rope(ops, DEV, rc.rope_inputs(*geom), write_q=False), "rope_kv_write")
    _assert(rc.run_rope(ops, DEV, rc.rope_inputs(*geom, slots="all")), "rope_kv_write")


@pytest.mark.parametrize("geom", rc.ROPE_GEOM, ids=lambda g: "-".join(map(str, g)))
def test_rope_kv_write_exact(geom):
    """cos / sin drawn from (1, 0), (0, 1), (-1, 0), (0, -1) and integer qkv: q and both caches equal the
    reference bit for bit (a wrong pairing, sign or slot cannot hide in a rounding)."""
    rep = _assert(rc.run_rope(ops, DEV, rc.rope_inputs(*geom, exact=True), exact=True), "rope_kv_write")
    assert rep.ratio == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("S", rc.ROPE_SLAB_S)
@pytest.mark.parametrize("D", [64, 128])
def test_rope_kv_write_slabs(D, S, dtype):
    _assert(rc.run_rope(ops, DEV, rc.rope_inputs(D, 4, 2, 16, 9, S=S, dtype=dtype)), "rope_kv_write")


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("M,N", rc.REDUCE_SHAPES)
@pytest.mark.parametrize("S", rc.REDUCE_S)
def test_slab_reduce(S, M, N, dtype, residual):
    _assert(rc.run_slab_reduce(ops, DEV, S, M, N, dtype, residual), "slab_reduce")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_slab_reduce_into_a_column_slice_with_a_strided_residual(dtype):
    S, M, N = 3, 37, 4096
    slabs, r = rc.reduce_inputs(S, M, N, dtype, True)
    buf = torch.full((M, N + 16), rc.SENTINEL, dtype=BF, device=DEV)
    out = buf[:, 8:8 + N]
    rbuf = torch.full((M, 2 * N), 1e4, dtype=BF, device=DEV)
    rbuf[:, N:] = r.to(DEV)
    rv = rbuf[:, N:]
    assert out.stride(0) == N + 16 and rv.stride(0) == 2 * N
    res = ops.slab_reduce(slabs.to(DEV), rv, out=out)
    assert res.data_ptr() == out.data_ptr()
    _assert(rc.check_ulp(f"slab_reduce {dtype} out slice", out, rc.slab_reduce64(slabs, r)), "slab_reduce")
    assert bool((buf[:, :8] == rc.SENTINEL).all()) and bool((buf[:, 8 + N:] == rc.SENTINEL).all())
