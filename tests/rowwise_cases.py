"""Inputs, fp64 references and the checker of the memory-bound row kernels (norm.hip, elementwise.hip,
``slab_reduce`` of stream_gemm.hip).

``randn`` rows and ``close(atol=2e-2, rtol=2e-2)`` cannot see a reduction that drops a vector, a lane
or a slab, nor a missing or misplaced eps: on unit-variance rows each moves the output by about 0.1 %.
The rows built here make those mistakes decisive, and the check is one bf16 rounding wide:

* **Row kinds** (``norm_rows``), stacked into every norm case, each row different: ``randn``;
  ``100 + randn`` (the two-pass mean); ``randn * 2^-10`` (mean square 1e-6, under RMSNorm's eps of
  1e-5: eps decides the output); ``randn * 2^-20`` (variance 9e-13, next to LayerNorm's eps of 1e-12);
  needle rows, ``0.01 * randn`` with one element of 8.0 at a seam of the kernel's work split (a
  reduction that misses it is off a hundredfold).  With a residual the needle sits in x on even and
  in the residual on odd needle rows.
* **Slab values** are k / 16, k integer in [-64, 64]: exact in bf16 and every partial sum exact in
  fp32, so the sum is the same in any order and the fp64 reference agrees bit for bit; only one slab
  of a needle row holds the needle (first, last, 7, 8, 11, 12 in turn).
* **fp64 references**, one per op, with the contract's own roundings and nothing else: RMSNorm rounds
  x + residual to bf16, slab consumers round the slab sum to bf16, ``slab_reduce`` rounds the sum and
  then adds the residual; everything else is fp64 arithmetic on the bf16 inputs.
* **Checker.**  ``ulp(E) = 2^(floor(log2 max(|E|, 2^-100)) - 7)``.  RMSNorm, gelu, silu_mul,
  rope_kv_write and slab_reduce: ``|got - E| <= ulp(E)`` per element (the rounding of a correct fp32
  result plus one flipped rounding).  LayerNorm, bert_embed and mean_pool cancel, so their bound is
  ``ulp(E) + 4 a_row`` (mean_pool's fp32 output: ``2^-22 |E| + 4 a_row``), ``a_row`` the largest error
  in that row of the project's own fp32 reference (unrounded) against fp64 -- and the checker asserts
  ``a_row <= 2^-12 max|E_row|`` so that a badly conditioned case cannot widen its own bound.

Every ``run_*`` function takes the implementation (``ops``, or a namespace with one op replaced by a
wrong one) and a device: CPU tensors run ``ops.reference``, device tensors the HIP kernels.  It returns
the worst ``Report`` of its launches.
"""
from __future__ import annotations

import functools
import math
import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import torch

from django_assistant_bot_amd.ops import reference as ref

BF = torch.bfloat16
RMS_EPS, LN_EPS = 1e-5, 1e-12
NEEDLE = 8.0
MARGIN = 4.0  # the attention tests' margin for a different, equally valid summation order
A_COND = 2.0 ** -12
FLOOR = 2.0 ** -100
ROWS = (1, 3, 9)


# ------------------------------------------------------------------------------------------------
# roundings and the checker


def _pow2(e):
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())


def round_bf16(x):
    """fp64 -> the nearest bf16 value (ties to even), as fp64; normal range only."""
    m, e = torch.frexp(x.double())  # m in [0.5, 1)
    return torch.round(m * 256.0) * _pow2(e - 8)


def ulp(E):
    """Spacing of bf16 at |E| (floored at 2^-100), fp64."""
    _, e = torch.frexp(E.double().abs().clamp_min(FLOOR))
    return _pow2(e - 8)


@dataclass
class Report:
    name: str
    ratio: float  # worst |got - E| / bound; inf where got is not finite
    row: int
    col: int
    n_bad: int
    a_rel: float | None = None  # worst a_row / max|E_row| of a margin check

    @property
    def ok(self):
        return self.ratio <= 1.0

    def __str__(self):
        a = "" if self.a_rel is None else f" a_row/max|E| {self.a_rel:.3g}"
        return (f"{self.name}: worst |got - E| / bound {self.ratio:.4g} at row {self.row} col {self.col}, "
                f"{self.n_bad} over{a}")


def _as2d(t):
    t = t.detach().cpu().double()
    return t.reshape(-1, t.shape[-1]) if t.dim() else t.reshape(1, 1)


def _report(name, got, E, bound, rows=None, a_rel=None):
    got, E, bound = _as2d(got), _as2d(E), _as2d(bound)
    assert got.shape == E.shape, f"{name}: shape {tuple(got.shape)} against {tuple(E.shape)}"
    err = (got - E).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).nan_to_num(float("inf"), posinf=float("inf"))
    i = int(ratio.argmax())
    r, c = divmod(i, ratio.shape[1])
    return Report(name, float(ratio.reshape(-1)[i]), int(rows[r]) if rows is not None else r, c,
                  int((~(ratio <= 1.0)).sum()), a_rel)


def check_ulp(name, got, E, rows=None):
    """|got - E| <= 1 ulp(E) per element."""
    return _report(name, got, E, ulp(E), rows)


def check_exact(name, got, E, rows=None):
    """got == E (values; -0 equals +0)."""
    return _report(name, got, E, torch.zeros_like(_as2d(E)), rows)


def check_margin(name, got, E, ref32, rows=None, fp32_out=False):
    """|got - E| <= ulp(E) + 4 a_row  (fp32 outputs: 2^-22 |E| + 4 a_row)."""
    E2, r2 = _as2d(E), _as2d(ref32)
    a_row = (r2 - E2).abs().amax(-1, keepdim=True)
    emax = E2.abs().amax(-1, keepdim=True)
    assert bool((a_row <= A_COND * emax).all()), f"{name}: badly conditioned row, a_row {float(a_row.max()):.3g}"
    a_rel = float((a_row / emax.clamp_min(FLOOR)).max())
    base = E2.abs() * 2.0 ** -22 if fp32_out else ulp(E2)
    return _report(name, got, E2, base + MARGIN * a_row, rows, a_rel)


def worst(reports, side=()):
    """The report with the largest ratio; ``side`` checks (exact copies, the bf16 copy of an fp32
    output) only take its place when one of them fails, so the figure printed is the kernel's own."""
    reports, side = list(reports), list(side)
    failed = [r for r in side if not r.ok]
    w = max(failed or reports, key=lambda r: r.ratio)
    return Report(w.name, w.ratio, w.row, w.col, sum(r.n_bad for r in reports + side),
                  max((r.a_rel for r in reports if r.a_rel is not None), default=None))


# ------------------------------------------------------------------------------------------------
# fp64 references


def _rms(v, w, eps):
    return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * w.double()


def rmsnorm64(x, w, eps, residual=None):
    """x bf16 [rows, cols], or slabs [S, rows, cols] whose sum is rounded to bf16.  (E, bf16 res_out)."""
    v = round_bf16(x.double().sum(0)) if x.dim() == 3 else x.double()
    res = None
    if residual is not None:
        v = round_bf16(v + residual.double())
        res = v.float().to(BF)
    return _rms(v, w, eps), res


def _ln(v, gamma, beta, eps):
    d = v - v.mean(-1, keepdim=True)
    return d * torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + eps) * gamma.double() + beta.double()


def layernorm64(x, gamma, beta, eps, residual=None):
    return _ln(x.double() if residual is None else x.double() + residual.double(), gamma, beta, eps)


def bert_embed64(ids, pos_ids, type_ids, word, pos, typ, gamma, beta, eps):
    t = torch.zeros_like(ids) if type_ids is None else type_ids
    return _ln(word[ids.long()].double() + pos[pos_ids.long()].double() + typ[t.long()].double(), gamma, beta, eps)


def mean_pool64(hidden, cu, normalize):
    cu = cu.tolist()
    out = torch.zeros(len(cu) - 1, hidden.shape[1], dtype=torch.float64)
    for b in range(len(cu) - 1):
        if cu[b + 1] > cu[b]:
            out[b] = hidden[cu[b]:cu[b + 1]].double().mean(0)
    if normalize:
        n = out.norm(dim=-1, keepdim=True)
        out = torch.where(n > 0, out / n.clamp_min(FLOOR), torch.zeros_like(out))
    return out


def gelu64(x, bias=None):
    v = x.double() if bias is None else x.double() + bias.double()
    return 0.5 * v * torch.special.erfc(-v * math.sqrt(0.5))  # no cancellation on the negative side


def silu_mul64(gate, up):
    g = gate.double()
    return g / (1.0 + torch.exp(-g)) * up.double()


def rope64(qkv, positions, cos_sin, k_cache, v_cache, slots, Hq, Hkv, D):
    """qkv bf16 [T, W] or slabs [S, T, W].  Returns (q [T, Hq, D], k cache, v cache, written
    [blocks, block_size] bool); the caches are fp64 copies of the given ones with the writes applied."""
    x = round_bf16(qkv.double().sum(0)) if qkv.dim() == 3 else qkv.double()
    T = x.shape[0]
    x = x.view(T, Hq + 2 * Hkv, D)
    cs = cos_sin[positions.long()].double()
    cos, sin = cs[..., 0].unsqueeze(1), cs[..., 1].unsqueeze(1)
    half = D // 2
    x1, x2 = x[:, :Hq + Hkv, :half], x[:, :Hq + Hkv, half:]
    rot = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1)
    kc, vc = k_cache.double().clone(), v_cache.double().clone()
    bs = kc.shape[2]
    written = torch.zeros(kc.shape[0], bs, dtype=torch.bool)
    for t, s in enumerate(slots.tolist()):
        if s >= 0:
            kc[s // bs, :, s % bs] = rot[t, Hq:]
            vc[s // bs, :, s % bs] = x[t, Hq + Hkv:]
            written[s // bs, s % bs] = True
    return rot[:, :Hq], kc, vc, written


def slab_reduce64(slabs, residual=None):
    y = round_bf16(slabs.double().sum(0))
    return y if residual is None else y + residual.double()


# ------------------------------------------------------------------------------------------------
# inputs


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def row_threads(cols, slab=False):
    """NT of the DAB_ROW_DISPATCH arm (norm.hip) a width takes; the slab kernel's <512, 1> launch."""
    n = cols // 8
    if slab and 256 < n <= 512:
        return 512
    return 64 if n <= 64 else 128 if n <= 128 else 256


def row_arm(cols, slab=False):
    """(NT, VPT) of the arm."""
    nt = row_threads(cols, slab)
    n = cols // 8
    return nt, 1 if n <= nt else 2 if n <= 512 else 4 if n <= 1024 else 8


def needle_positions(cols, nt):
    """Needle columns: the seams of a row-per-workgroup kernel of ``nt`` threads x 8-element vectors,
    or (``nt`` None) of layernorm_rows_kernel's lane-strided 4-element chunks."""
    cand = (0, 3, 4, 255, 256, cols - 1) if nt is None else (0, 7, 8, 511, 512, 8 * nt - 1, 8 * nt, cols - 8, cols - 1)
    return list(dict.fromkeys(p for p in cand if 0 <= p < cols))


def norm_rows(cols, nt, residual, *key):
    """(x, residual or None) bf16 [4 + needles, cols]: the row kinds of the module docstring."""
    g = _gen("rows", cols, nt, residual, *key)
    pos = needle_positions(cols, nt)
    scale = torch.tensor([1.0, 1.0, 2.0 ** -10, 2.0 ** -20] + [0.01] * len(pos))[:, None]
    x = torch.randn(len(scale), cols, generator=g) * scale
    x[1] += 100.0
    r = 0.25 * torch.randn(len(scale), cols, generator=g) * scale if residual else None
    for i, p in enumerate(pos):
        (r if residual and i % 2 else x)[4 + i, p] = NEEDLE
    return x.to(BF), None if r is None else r.to(BF)


def affine(cols, *key):
    g = _gen("affine", cols, *key)
    return (0.5 + torch.rand(cols, generator=g)).to(BF), torch.randn(cols, generator=g).to(BF)


def _k16(shape, g, kmax=64):
    return torch.randint(-kmax, kmax + 1, shape, generator=g).float() / 16.0


NEEDLE_SLABS = (0, -1, 7, 8, 11, 12)


def slab_rows(S, cols, nt, dtype, residual, *key):
    """(slabs [S, rows, cols] of ``dtype``, residual or None): two rows of k / 16 draws, a sparse row
    (a few +-1/16, mean square about eps / 2: eps decides) and the needle rows (background k in
    {-1, 0, 1}, the needle in one slab)."""
    g = _gen("slabs", S, cols, nt, str(dtype), residual, *key)
    pos = needle_positions(cols, nt)
    R = 3 + len(pos)
    x = _k16((S, R, cols), g)
    x[:, 2] = 0.0
    n = max(1, round(0.5 * RMS_EPS * cols * 256))
    for c in torch.randperm(cols, generator=g)[:n].tolist():
        x[int(torch.randint(0, S, (1,), generator=g)), 2, c] = 1 / 16 if c % 2 else -1 / 16
    x[:, 3:] = _k16((S, len(pos), cols), g, 1)
    which = [s % S for s in NEEDLE_SLABS if -S <= s < S]
    for i, p in enumerate(pos):
        x[:, 3 + i, p] = 0.0
        x[which[i % len(which)], 3 + i, p] = NEEDLE
    r = None
    if residual:
        scale = torch.tensor([1.0, 1.0, 2.0 ** -10] + [2.0 ** -4] * len(pos))[:, None]
        r = (torch.randn(R, cols, generator=g) * scale).to(BF)
    return x.to(dtype), r


def plans(n, rows=ROWS, full=True):
    """Row-index sets of one case: the whole stack, then its first r rows (wrapping round)."""
    return ([torch.arange(n)] if full else []) + [torch.arange(r) % n for r in rows]


def _dev(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


# ------------------------------------------------------------------------------------------------
# the cases (shared by the CPU self-test and the GPU tests)

# every (NT, VPT) arm once full and once with a nearly empty last round
RMSNORM_COLS = (8, 264, 520, 1032, 2048, 2056, 4104, 8200, 16384)
RMSNORM_BAD_COLS = (12, 16392)
SLAB_S = (1, 2, 4, 5, 8, 9, 12, 13, 16, 21)
SLAB_COLS = (64, 1024, 2048, 2056, 4096, 4104, 8200)
SLAB_CASES = sorted({(c, S) for c in (4096, 4104) for S in SLAB_S} | {(c, 13) for c in SLAB_COLS})
LN_COLS = (8, 384, 520, 1032, 2048, 2056, 4104, 8200)  # (1032, 2048: the (256, 1) arm)
LN_WAVE = tuple((c, r) for c in (768, 1024) for r in (1, 2, 3, 8, 9, 17))
EMBED_H = (384, 768, 1024, 2048, 2056, 4104, 8200)  # the encoder widths, then the other four arms
GATHER_COLS = (8, 768, 2056, 4096)
POOL_H = (8, 384, 1024, 2048, 2056, 4096)
GELU_SHAPES = ((1, 8), (33, 3080))
BIG = (4100, 4096)  # 2,099,200 vectors: past the 8192-block grid cap, the stride loop takes a second pass
# gelu's bias index is i % (cols / 8): a width whose vector count does not divide the 2,097,152-vector grid
# stride (BIG's 512 does), so that a bias picked by the first pass's index shows; 2,098,250 vectors
BIG_ODD = (5450, 3080)
SILU_F = (16, 1424)
ROPE_GEOM = (  # D, Hq, Hkv, block size, T
    (128, 4, 2, 64, 50), (64, 4, 2, 16, 50), (128, 32, 8, 16, 1), (64, 32, 8, 64, 1), (128, 8, 8, 16, 50),
    (64, 8, 8, 64, 50), (128, 4, 2, 16, 1), (64, 32, 8, 16, 9))
ROPE_SLAB_S = (1, 3, 4, 5, 8, 9)
REDUCE_SHAPES = ((5, 1032), (37, 4096))
REDUCE_S = (1, 3, 16)


@functools.lru_cache(maxsize=None)
def rms_case(cols, residual):
    x, r = norm_rows(cols, row_threads(cols), residual, "rms")
    w, _ = affine(cols, "rms")
    E, Er = rmsnorm64(x, w, RMS_EPS, r)
    return SimpleNamespace(x=x, r=r, w=w, E=E, Er=Er)


def run_rmsnorm(impl, dev, cols, residual):
    c = rms_case(cols, residual)
    reps, side = [], []
    for idx in plans(c.x.shape[0]):
        x, r, w = _dev(dev, c.x[idx], None if c.r is None else c.r[idx], c.w)
        out, ro = impl.rmsnorm(x, w, RMS_EPS, residual=r)
        reps.append(check_ulp(f"rmsnorm cols {cols} rows {len(idx)}", out, c.E[idx], idx))
        if residual:
            side.append(check_exact(f"rmsnorm res_out cols {cols} rows {len(idx)}", ro, c.Er[idx], idx))
    return worst(reps, side)


@functools.lru_cache(maxsize=None)
def slab_case(cols, S, dtype, residual):
    x, r = slab_rows(S, cols, row_threads(cols, True), dtype, residual)
    w, _ = affine(cols, "slab")
    E, Er = rmsnorm64(x, w, RMS_EPS, r)
    return SimpleNamespace(x=x, r=r, w=w, E=E, Er=Er)


def run_rmsnorm_slabs(impl, dev, cols, S, dtype, residual, row_plans=None):
    c = slab_case(cols, S, dtype, residual)
    reps, side = [], []
    for idx in plans(c.x.shape[1]) if row_plans is None else row_plans:
        x, r, w = _dev(dev, c.x[:, idx].contiguous(), None if c.r is None else c.r[idx], c.w)
        out, ro = impl.rmsnorm(x, w, RMS_EPS, residual=r)
        reps.append(check_ulp(f"rmsnorm slabs {dtype} cols {cols} S {S} rows {len(idx)}", out, c.E[idx], idx))
        if residual:
            side.append(check_exact(f"rmsnorm slabs res_out cols {cols} S {S} rows {len(idx)}", ro, c.Er[idx], idx))
    return worst(reps, side)


@functools.lru_cache(maxsize=None)
def ln_case(cols, residual):
    x, r = norm_rows(cols, None if cols in (768, 1024) else row_threads(cols), residual, "ln")
    g, b = affine(cols, "ln")
    E = layernorm64(x, g, b, LN_EPS, r)
    return SimpleNamespace(x=x, r=r, g=g, b=b, E=E, ref32=ref.layernorm(x.float(), g, b, LN_EPS, r))


def run_layernorm(impl, dev, cols, residual, rows=None):
    """``rows``: the row counts to launch (default: the whole stack, then 1, 3 and 9 rows)."""
    c = ln_case(cols, residual)
    reps = []
    for idx in plans(c.x.shape[0]) if rows is None else plans(c.x.shape[0], rows, False):
        x, r, g, b = _dev(dev, c.x[idx], None if c.r is None else c.r[idx], c.g, c.b)
        out = impl.layernorm(x, g, b, LN_EPS, residual=r)
        reps.append(check_margin(f"layernorm cols {cols} rows {len(idx)}", out, c.E[idx], c.ref32[idx], idx))
    return worst(reps)


EMBED_V, EMBED_P = 500, 64


@functools.lru_cache(maxsize=None)
def embed_case(H):
    """Word rows 1.. hold the needle rows (randn with one 8.0 at a seam), V - 2 is ``100 + randn``;
    the two type rows differ by about 1; 41 rows with ids 0 and V - 1, positions 0 and P - 1."""
    g = _gen("embed", H)
    V, P = EMBED_V, EMBED_P
    word, pos = torch.randn(V, H, generator=g), torch.randn(P, H, generator=g)
    needles = needle_positions(H, row_threads(H))
    for i, p in enumerate(needles):
        word[1 + i, p] = NEEDLE
    word[V - 2] += 100.0
    typ = 0.1 * torch.randn(2, H, generator=g)
    typ[1] += 1.0
    ids = torch.cat([torch.tensor([0, V - 1, V - 2]), torch.arange(1, 1 + len(needles)),
                     torch.randint(0, V, (41,), generator=g)])[:41].to(torch.int32)
    pids = torch.cat([torch.tensor([0, P - 1]), torch.randint(0, P, (39,), generator=g)]).to(torch.int32)
    types = {"none": None, "ones": torch.ones(41, dtype=torch.int32),
             "mixed": torch.randint(0, 2, (41,), generator=g).to(torch.int32)}
    assert 0 < int(types["mixed"].sum()) < 41
    gam, bet = affine(H, "embed")
    word, pos, typ = word.to(BF), pos.to(BF), typ.to(BF)
    E = {k: bert_embed64(ids, pids, t, word, pos, typ, gam, bet, LN_EPS) for k, t in types.items()}
    r32 = {k: ref.bert_embed(ids, pids, t, word.float(), pos.float(), typ.float(), gam, bet, LN_EPS)
           for k, t in types.items()}
    return SimpleNamespace(ids=ids, pids=pids, types=types, word=word, pos=pos, typ=typ, g=gam, b=bet, E=E, ref32=r32)


def run_bert_embed(impl, dev, H, types):
    c = embed_case(H)
    reps = []
    for n in (41, 1):
        t = c.types[types]
        t = None if t is None else t[:n]
        ids, pids, t, word, pos, typ, g, b = _dev(dev, c.ids[:n], c.pids[:n], t, c.word, c.pos, c.typ, c.g, c.b)
        out = impl.bert_embed(ids, pids, t, word, pos, typ, g, b, LN_EPS)
        reps.append(check_margin(f"bert_embed H {H} types {types} rows {n}", out, c.E[types][:n], c.ref32[types][:n]))
    return worst(reps)


def run_embed_gather(impl, dev, cols):
    g = _gen("gather", cols)
    V = 300
    table = torch.randn(V, cols, generator=g).to(BF)
    ids = torch.cat([torch.tensor([0, V - 1, 5, 5, 0, V - 1]), torch.randint(0, V, (31,), generator=g)]).to(torch.int32)
    reps = []
    for n in (37, 1):
        i, t = _dev(dev, ids[:n], table)
        reps.append(check_exact(f"embed_gather cols {cols} rows {n}", impl.embed_gather(i, t), table[ids[:n].long()]))
    return worst(reps)


POOL_LENS = (0, 1, 512, 0, 0, 7, 3, 20, 0)  # empty first, last and twice in a row; sequence 6 is all zero
POOL_SPIKE = (2, 100)  # (sequence, token): 256 among values of 0.01 in the last column


@functools.lru_cache(maxsize=None)
def pool_case(H):
    g = _gen("pool", H)
    cu = torch.tensor([0] + list(torch.tensor(POOL_LENS).cumsum(0)), dtype=torch.int32)
    h = torch.randn(int(cu[-1]), H, generator=g)
    h[int(cu[6]):int(cu[7])] = 0.0
    s0 = int(cu[POOL_SPIKE[0]])
    h[s0:int(cu[POOL_SPIKE[0] + 1]), H - 1] = 0.01
    h[s0 + POOL_SPIKE[1], H - 1] = 256.0
    h = h.to(BF)
    one = torch.tensor([0, 5], dtype=torch.int32)  # a batch of one: the first five tokens of the 512
    keys = [(n, b) for n in (False, True) for b in (False, True)]  # (normalize, batch of one)
    E = {(n, b): mean_pool64(h[s0:s0 + 5] if b else h, one if b else cu, n) for n, b in keys}
    r32 = {(n, b): ref.mean_pool(h[s0:s0 + 5] if b else h, one if b else cu, n) for n, b in keys}
    return SimpleNamespace(h=h, cu=cu, one=one, s0=s0, E=E, ref32=r32)


def run_mean_pool(impl, dev, H, normalize):
    c = pool_case(H)
    reps, side = [], []
    for single in (False, True):
        h, cu = _dev(dev, c.h[c.s0:c.s0 + 5] if single else c.h, c.one if single else c.cu)
        out, ob = impl.mean_pool(h, cu, normalize=normalize, want_bf16=True)
        E, r32 = c.E[(normalize, single)], c.ref32[(normalize, single)]
        tag = f"mean_pool H {H} normalize {normalize} batch {E.shape[0]}"
        assert out.dtype == torch.float32 and ob.dtype == BF
        reps.append(check_margin(tag, out, E, r32, fp32_out=True))  # empty / all-zero sequences: E = 0 = the bound
        side.append(check_ulp(tag + " bf16 copy", ob, out))  # one bf16 ulp of the fp32 output
    return worst(reps, side)


GELU_MIN = -3.5


def _gelu_inputs(rows, cols, bias, g):
    """Pre-activations x + bias under -3.5 are folded to |x| + bias.  Down there the result is below
    1e-3 and every fp32 erf form loses relative accuracy (torch's 0.5 x (1 + erf), the oracle, is over
    1 bf16 ulp off from -4 and 255 ulp at -12; the kernel's A&S 7.1.26 erfc 5 ulp under -6): the contract
    is the absolute 2e-7 that test_gelu_erf_sweep asserts on [-12, 12], not a relative one."""
    x = torch.randn(rows, cols, generator=g).to(BF)
    b = torch.randn(cols, generator=g).to(BF) if bias else None
    v = x.float() if b is None else x.float() + b.float()
    x = torch.where(v < GELU_MIN, x.abs(), x)
    assert float((x.float() if b is None else x.float() + b.float()).min()) >= GELU_MIN
    return x, b


def run_gelu(impl, dev, rows, cols, bias):
    x, b = _gelu_inputs(rows, cols, bias, _gen("gelu", rows, cols, bias))
    xd, bd = _dev(dev, x, b)
    return check_ulp(f"gelu {rows} x {cols} bias {bias}", impl.gelu(xd, bd), gelu64(x, b))


def interleave16(gate, up):
    """[rows, F] gate and up -> [rows, 2F] in 16-column [gate | up] groups."""
    rows, F = gate.shape
    return torch.stack([gate.reshape(rows, F // 16, 16), up.reshape(rows, F // 16, 16)], 2).reshape(rows, 2 * F)


def run_silu_mul(impl, dev, rows, F):
    """Both layouts of one (gate, up) draw against one reference."""
    g = _gen("silu", rows, F)
    gate, up = (2.0 * torch.randn(rows, F, generator=g)).to(BF), torch.randn(rows, F, generator=g).to(BF)
    E = silu_mul64(gate, up)
    stacked, inter = _dev(dev, torch.cat([gate, up], -1), interleave16(gate, up))
    return worst([check_ulp(f"silu_mul stacked {rows} x {F}", impl.silu_mul(stacked), E),
                  check_ulp(f"silu_mul interleaved {rows} x {F}", impl.silu_mul(inter, interleaved=True), E)])


def silu_sweep_inputs():
    """Every bf16 gate in [-120, 120] (denormals included) against up = 1 and up = -3: x [2, 2n]."""
    bits = torch.arange(-(1 << 15), 1 << 15, dtype=torch.int32).to(torch.int16)
    gate = bits.view(BF)
    gate = gate[torch.isfinite(gate.float()) & (gate.float().abs() <= 120.0)]
    gate = torch.cat([gate, gate.new_zeros(-gate.numel() % 16)])
    gate = gate.expand(2, -1)
    up = torch.tensor([[1.0], [-3.0]]).expand(2, gate.shape[1]).to(BF)
    return gate.contiguous(), up.contiguous()


def run_silu_sweep(impl, dev):
    gate, up = silu_sweep_inputs()
    E = silu_mul64(gate, up)
    stacked, inter = _dev(dev, torch.cat([gate, up], -1), interleave16(gate, up))
    return worst([check_ulp("silu_mul sweep stacked", impl.silu_mul(stacked), E),
                  check_ulp("silu_mul sweep interleaved", impl.silu_mul(inter, interleaved=True), E)])


ROPE_MAX_POS = 4096
SENTINEL = 7.0


@functools.lru_cache(maxsize=None)
def rope_table(D):
    return ref.rope_cos_sin(ref.llama3_inv_freq(D, 500000.0, None), ROPE_MAX_POS).float().contiguous()


def unit_table(D, g):
    """A cos_sin table whose entries are (1, 0), (0, 1), (-1, 0) or (0, -1) per (position, dim)."""
    q = torch.randint(0, 4, (ROPE_MAX_POS, D // 2), generator=g)
    unit = torch.tensor([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    return unit[q].contiguous()


def rope_inputs(D, Hq, Hkv, bs, T, slots="some", S=0, dtype=BF, exact=False):
    """qkv (bf16 rows, or S slabs of ``dtype``), positions with 0 and max_pos - 1, slots (``some``: one
    skipped token and the last slot of the last block; ``all``: every token skipped), caches pre-filled
    with a sentinel."""
    g = _gen("rope", D, Hq, Hkv, bs, T, slots, S, str(dtype), exact)
    W = (Hq + 2 * Hkv) * D
    if exact:
        qkv = torch.randint(-8, 9, (T, W), generator=g).float().to(BF)
    elif S:
        qkv = _k16((S, T, W), g).to(dtype)
    else:
        qkv = torch.randn(T, W, generator=g).to(BF)
    pos = torch.randint(0, ROPE_MAX_POS, (T,), generator=g).to(torch.int32)
    pos[0] = ROPE_MAX_POS - 1 if T > 1 or D == 128 else 0
    pos[-1] = 0 if T > 1 else pos[0]
    nb = -(-T // bs) + 2
    sl = torch.randperm(nb * bs - 1, generator=g)[:T].to(torch.int64)
    sl[-1] = nb * bs - 1
    if T > 3:
        sl[3] = -1
    if slots == "all":
        sl[:] = -1
    kc = torch.full((nb, Hkv, bs, D), SENTINEL, dtype=BF)
    cs = unit_table(D, g) if exact else rope_table(D)
    return SimpleNamespace(qkv=qkv, pos=pos, cs=cs, kc=kc, vc=kc.clone(), slots=sl, Hq=Hq, Hkv=Hkv, D=D)


def run_rope(impl, dev, c, write_q=True, exact=False):
    Eq, Ek, Ev, written = rope64(c.qkv, c.pos, c.cs, c.kc, c.vc, c.slots, c.Hq, c.Hkv, c.D)
    qkv, pos, cs, kc, vc, slots = _dev(dev, c.qkv, c.pos, c.cs, c.kc.clone(), c.vc.clone(), c.slots)
    q = impl.rope_kv_write(qkv, pos, cs, kc, vc, slots, c.Hq, c.Hkv, c.D, write_q=write_q)
    tag = (f"rope D {c.D} heads {c.Hq}/{c.Hkv} bs {c.kc.shape[2]} T {c.pos.numel()} qkv {tuple(c.qkv.shape)} "
           f"{c.qkv.dtype}")
    chk = check_exact if exact else check_ulp
    reps, side = [chk(tag + " k cache", kc, Ek)], [check_exact(tag + " v cache", vc, Ev)]
    if write_q:
        reps.append(chk(tag + " q", q, Eq))
    else:
        assert q is None or not qkv.is_cuda  # (the CPU oracle always returns q)
    keep = ~written[:, None, :, None].expand_as(c.kc)
    for cache in (kc, vc):  # every untouched slot still holds the sentinel
        assert bool((cache.cpu()[keep] == SENTINEL).all()), tag + ": a slot no token names was written"
    return worst(reps, side)


def reduce_inputs(S, M, N, dtype, residual):
    """k / 16 slabs; the residual cancels the sum on odd rows (-sum + 0.25 randn), so a rounding taken
    at the wrong point is many ulp of the small result."""
    g = _gen("reduce", S, M, N, str(dtype), residual)
    slabs = _k16((S, M, N), g).to(dtype)
    r = None
    if residual:
        r = torch.randn(M, N, generator=g)
        r[1::2] = 0.25 * r[1::2] - slabs.float().sum(0)[1::2]
        r = r.to(BF)
    return slabs, r


def run_slab_reduce(impl, dev, S, M, N, dtype, residual):
    slabs, r = reduce_inputs(S, M, N, dtype, residual)
    sd, rd = _dev(dev, slabs, r)
    return check_ulp(f"slab_reduce {dtype} S {S} {M} x {N} residual {residual}", impl.slab_reduce(sd, rd),
                     slab_reduce64(slabs, r))
