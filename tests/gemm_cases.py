"""Exact-operand inputs, fp64 references, guarded buffers and runners of the GEMM family (gemm.hip,
gemm256.hip, gemm_mid.hip, stream_gemm.hip, ``slab_reduce``).

``randn`` activations, ``0.05 randn`` weights and ``close(atol=3e-2, rtol=2e-2)`` cannot see a bf16 store
that truncates, a residual added to the fp32 accumulator or a bias added after the rounding
(tests/test_gemm_exact_cpu.py keeps that on record).  The operands built here leave the final rounding as
the only freedom a kernel has, and the contract of ops/reference.py fixes it:

* **Operands.**  A and B are integers in [-7, 7], bias and residual half-integers in [-32, 32], drawn with
  a CPU generator seeded from the case key.  Every product and partial sum is an integer below 2^24 for
  K <= 14336, so any MFMA order, split-K combine or slab sum is exact in fp32 and the fp64 product is the
  accumulator, bit for bit.  For GELU and SwiGLU, B and the bias are scaled by 2^-s (a power of two keeps
  all of that exact), s chosen per K so that the pre-activations spread by 0.9 to 1.8 (``act_shift``).
* **Decisive draws.**  A builder asserts max |C| < 2^24 and that at least 1 % of the outputs differ between
  nearest-even and truncation, between a bias added before and after the first rounding, and between a
  residual added after and before it (measured over the first 2^20 outputs of a large case).  A draw
  that misses a floor is redrawn from the next seed of the same key (only shapes of a few hundred outputs
  ever need it: at K = 64 the shares are about 2 %); a case that finds no draw raises: an error in the
  table, not a skip.
* **Guarded buffers.**  A is rows [2, 2 + M) of a taller and wider buffer (lda = K + 8); B the same in its
  row-major form, or a ``shuffle_weights`` copy of B padded to whole 16-row blocks (16 ``b_group`` rows)
  between two 16-row guards; the bias a slice of a longer vector.  Everything outside the operand proper is
  NaN.  The output and the residual are views of larger buffers with other row strides, the output's
  pre-filled with a sentinel: afterwards everything outside the view is still the sentinel and no valid
  output is NaN.  Only rows are offset and every stride is a multiple of 8, so all vectors stay on 16-byte
  boundaries.
* **References** in fp64: ``round_bf16(C)``, ``round_bf16(C + b)``, ``round_bf16(round_bf16(C + b) + r)``, C
  itself for fp32 outputs and slabs, C with -inf under the masks for EPI_SCORES, ``gelu64(C + b)``,
  ``silu_mul64`` over 16- and 8-row groups.
* **Bounds.**  Equality for everything but GELU and SwiGLU; those are one fp32 epilogue and one rounding of
  an exact accumulator: ``|got - E| <= ulp(E)``, the bound tests/rowwise_cases.py holds ``gelu`` and
  ``silu_mul`` to.  GELU elements whose pre-activation is under ``GELU_MIN`` take the bound of
  test_gelu_erf_sweep, ``2^-8 |E| + 2e-7`` (every fp32 erf form loses relative accuracy down there, see
  rowwise_cases._gelu_inputs); at most 5 % of a case may be such elements.

Every ``run_*`` takes the implementation and a device: ``ops`` with the HIP kernels, or ``oracle()`` (the
fp32 reference writing through the same views, optionally with one planted mistake) on the CPU.
"""
from __future__ import annotations

import functools
import math
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import rowwise_cases as rc
from django_assistant_bot_amd.ops import reference as ref
from django_assistant_bot_amd.ops.kernels import shuffle_weights, unshuffle_weights
from rowwise_cases import GELU_MIN, SENTINEL, Report, check_exact, check_ulp, gelu64, round_bf16, silu_mul64, ulp

BF = torch.bfloat16
NAN = float("nan")
INF = float("inf")
GUARD = 2  # guard rows before and after an operand / output view
A_PAD, OUT_PAD, RES_PAD = 8, 16, 24  # columns between the width and the row stride (different per buffer)
SHARE_FLOOR = 0.01
SHARE_SAMPLE = 1 << 20
GELU_LOW_SHARE = 0.05
TRIES = 1 << 14

PLAIN = ("none", "bias", "residual", "bias_residual")
EXACT = PLAIN + ("f32",)
ACT = ("gelu", "swiglu", "swiglu_bias", "swiglu8")
EPI_CODE = {"gelu": ref.EPI_GELU, "swiglu": ref.EPI_SWIGLU, "swiglu_bias": ref.EPI_SWIGLU, "swiglu8": ref.EPI_SWIGLU8}


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def trunc_bf16(x):
    """fp64 -> the bf16 value a store that drops the low 16 bits of the fp32 gives, as fp64."""
    m, e = torch.frexp(x.double())
    return torch.trunc(m * 256.0) * rc._pow2(e - 8)


def _share(a, b):
    return float((a != b).double().mean())


def _ints(shape, g):
    return torch.randint(-7, 8, shape, generator=g).double()


def _halves(shape, g):
    return torch.randint(-64, 65, shape, generator=g).double() / 2


def _draw(make, ok, *key):
    for t in range(TRIES):
        x = make(_gen(*key, t))
        if ok(x):
            return x
    raise AssertionError(f"case {key}: no decisive draw in {TRIES} seeds -- an error in the table")


def act_shift(K):
    """The smallest s with 2^-s sqrt(K) 18.67 <= 1.78 (18.67^2: the variance of a uniform integer in
    [-7, 7]): pre-activations spread by 0.89 to 1.78, so that under 2.5 % of them lie below GELU_MIN."""
    return max(0, math.ceil(math.log2(math.sqrt(K) * 56.0 / 3.0 / 1.78)))


def _head(M, N):
    return max(1, min(M, -(-SHARE_SAMPLE // N)))


@functools.lru_cache(maxsize=6)
def exact_case(M, N, K):
    """A, B, bias, residuals (without / with the bias) as bf16, C as fp32 (an exact integer)."""
    h = _head(M, N)

    def abb(g):  # (drawn together: with four outputs a given C may admit no decisive bias)
        A, B = _ints((M, K), g), _ints((N, K), g)
        return A, B, A @ B.t(), _halves((N,), g)

    def abb_ok(x):
        C, v = x[2][:h], x[2][:h] + x[3]
        return (float(x[2].abs().max()) < 2 ** 24 and _share(round_bf16(C), trunc_bf16(C)) >= SHARE_FLOOR
                and _share(round_bf16(v), trunc_bf16(v)) >= SHARE_FLOOR
                and _share(round_bf16(v), round_bf16(round_bf16(C) + x[3])) >= SHARE_FLOOR)

    A, B, C, bias = _draw(abb, abb_ok, "abb", M, N, K)
    Ch = C[:h]

    def res_ok(with_bias):
        P = round_bf16(Ch + bias) if with_bias else round_bf16(Ch)
        late = round_bf16(round_bf16(Ch) + bias) if with_bias else None

        def ok(r):
            r, v = r[:h], P + r[:h]
            good = round_bf16(v)
            return (_share(good, trunc_bf16(v)) >= SHARE_FLOOR
                    and _share(good, round_bf16((Ch + bias if with_bias else Ch) + r)) >= SHARE_FLOOR
                    and (late is None or _share(good, round_bf16(late + r)) >= SHARE_FLOOR))
        return ok

    res = _draw(lambda g: _halves((M, N), g), res_ok(False), "res", M, N, K)
    res_b = _draw(lambda g: _halves((M, N), g), res_ok(True), "res_b", M, N, K)
    assert torch.equal(C.float().double(), C)
    return SimpleNamespace(M=M, N=N, K=K, s=0, A=A.to(BF), B=B.to(BF), bias=bias.to(BF), res=res.to(BF),
                           res_b=res_b.to(BF), C=C.float())


@functools.lru_cache(maxsize=6)
def act_case(M, N, K):
    """Operands of the GELU / SwiGLU epilogues: B and the bias times 2^-s."""
    s = act_shift(K)
    g = _gen("act", M, N, K)
    A, B, bias = _ints((M, K), g), _ints((N, K), g) * 2.0 ** -s, _halves((N,), g) * 2.0 ** -s
    C = A @ B.t()
    assert float(C.abs().max()) * 2.0 ** s < 2 ** 24
    assert torch.equal(C.float().double(), C) and torch.equal(B.to(BF).double(), B)
    assert torch.equal(bias.to(BF).double(), bias)
    return SimpleNamespace(M=M, N=N, K=K, s=s, A=A.to(BF), B=B.to(BF), bias=bias.to(BF), C=C.float())


def case_of(M, N, K, epi):
    return act_case(M, N, K) if epi in ACT else exact_case(M, N, K)


def _groups(v, hg):
    v = v.reshape(v.shape[0], v.shape[1] // (2 * hg), 2, hg)
    return silu_mul64(v[:, :, 0], v[:, :, 1]).reshape(v.shape[0], -1)


@functools.lru_cache(maxsize=12)
def expected(M, N, K, epi):
    """(E, low): E in the output's own dtype where the check is equality, fp64 for GELU / SwiGLU;
    ``low``: the GELU elements under GELU_MIN (else None)."""
    c = case_of(M, N, K, epi)
    C = c.C.double()
    if epi == "none":
        return round_bf16(C).to(BF), None
    if epi == "bias":
        return round_bf16(C + c.bias.double()).to(BF), None
    if epi == "residual":
        return round_bf16(round_bf16(C) + c.res.double()).to(BF), None
    if epi == "bias_residual":
        return round_bf16(round_bf16(C + c.bias.double()) + c.res_b.double()).to(BF), None
    if epi == "f32":
        return c.C, None
    if epi == "gelu":
        v = C + c.bias.double()
        low = v < GELU_MIN
        assert float(low.double().mean()) <= GELU_LOW_SHARE, f"gelu case {M} x {N} x {K}: too many deep negatives"
        return gelu64(v), low
    if epi == "swiglu":
        return _groups(C, 16), None
    if epi == "swiglu_bias":
        return _groups(C + c.bias.double(), 16), None
    if epi == "swiglu8":
        return _groups(C, 8), None
    raise KeyError(epi)


# ------------------------------------------------------------------------------------------------
# checkers


def check_same(name, got, E):
    """Equality; ``E`` holds the expected values in the output's dtype (the quick path of check_exact)."""
    got = got.detach().cpu()
    if got.dtype == E.dtype and got.shape == E.shape and torch.equal(got, E):
        return Report(name, 0.0, 0, 0, 0)
    return check_exact(name, got, E)


def check_act(name, got, E, low=None):
    """One bf16 ulp of the fp64 result; ``2^-8 |E| + 2e-7`` on the ``low`` elements."""
    if low is None or not bool(low.any()):
        return check_ulp(name, got, E)
    got = rc._as2d(got)
    hi = check_ulp(name, torch.where(low, E, got), E)  # the elements held to one ulp alone, for the record
    rep = rc._report(name, got, E, torch.where(low, E.abs() * 2.0 ** -8 + 2e-7, ulp(E)))
    rep.name += f" (from GELU_MIN up: {hi.ratio:.4g})"
    return rep


def _failed(name, why):
    return Report(f"{name}: {why}", INF, -1, -1, 1)


# ------------------------------------------------------------------------------------------------
# guarded buffers


def _stride(cols, pad):
    return cols + pad + (-cols) % 8


def guarded(x, dev, pad=A_PAD, fill=NAN, dtype=BF):
    """(buffer, view): ``x`` as rows [GUARD, GUARD + R) and the first columns of a buffer of ``fill``."""
    R, C = x.shape
    buf = torch.full((R + 2 * GUARD, _stride(C, pad)), fill, dtype=dtype)
    buf[GUARD:GUARD + R, :C] = x.to(dtype)
    buf = buf.to(dev)
    return buf, buf[GUARD:GUARD + R, :C]


def shuffled_copy(B, dev, group=1, rows=None):
    """(buffer, view): ``shuffle_weights`` of B padded with NaN rows to ``rows`` (default: the next
    multiple of 16 ``group``), itself between two 16-row NaN guards; the view is contiguous."""
    N, K = B.shape
    R = -(-N // (16 * group)) * 16 * group if rows is None else rows
    pad = torch.full((R, K), NAN, dtype=BF)
    pad[:N] = B
    buf = torch.full((R + 32, K), NAN, dtype=BF)
    buf[16:16 + R] = shuffle_weights(pad, group)
    buf = buf.to(dev)
    return buf, buf[16:16 + R]


def vector(b, dev):
    buf = torch.full((b.numel() + 16,), NAN, dtype=b.dtype)
    buf[8:8 + b.numel()] = b
    buf = buf.to(dev)
    return buf, buf[8:8 + b.numel()]


def out_view(M, n_out, dev, dtype=BF):
    buf = torch.full((M + 2 * GUARD, _stride(n_out, OUT_PAD)), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + M, :n_out]


def untouched(buf, M, n_out):
    b = buf.detach().cpu()
    return bool((b[:GUARD] == SENTINEL).all() and (b[GUARD + M:] == SENTINEL).all()
                and (b[GUARD:GUARD + M, n_out:] == SENTINEL).all())


def _past(t, rows=0, cols=0):
    """The view ``t`` grown by rows / columns of the memory behind it."""
    return torch.as_strided(t, (t.shape[0] + rows, t.shape[1] + cols), t.stride(), t.storage_offset())


# ------------------------------------------------------------------------------------------------
# gemm_mid's work decomposition (the comment at the top of gemm_mid.hip and its launcher)


def mid_decomposition(M, N, K, bk=64, cus=256):
    """tiles_m row tiles form one group; the tiles_n x (K / bk) iterations (tile-major) are split evenly
    over gn = 8 floor(cus / 8 / tiles_m) groups: group j takes q iterations, one more when j < r.
    ``segments[t]``: the groups that share column tile t; ``ranges(t)``: their K ranges."""
    tiles_m, tiles_n, kt = -(-M // 128), N // 256, K // bk
    gn = 8 * ((cus & ~7) // 8 // tiles_m)
    q, r = divmod(tiles_n * kt, gn)

    def start(j):
        return j * q + min(j, r)

    def owner(i):
        return i // (q + 1) if i < r * (q + 1) else r + (i - r * (q + 1)) // q

    def ranges(t):
        lo, hi = owner(t * kt), owner(t * kt + kt - 1)
        return [((max(start(j), t * kt) - t * kt) * bk, (min(start(j + 1), (t + 1) * kt) - t * kt) * bk)
                for j in range(lo, hi + 1)]

    segments = [len(ranges(t)) for t in range(tiles_n)]
    return SimpleNamespace(tiles_m=tiles_m, tiles_n=tiles_n, kt=kt, gn=gn, q=q, r=r, segments=segments, ranges=ranges)


def bt_big(M, N):
    """gemm.hip's launcher: the 256 x 256 / 8-wave tile."""
    return M >= 2048 and N >= 512 and -(-M // 256) * -(-N // 256) >= 160


# ------------------------------------------------------------------------------------------------
# the fp32 oracle, with planted mistakes

DEFECTS = ("trunc", "res-early", "bias-late", "bias-by-m", "k-last", "k-chunk-twice", "mid-drop-segment", "slab-skip",
           "swiglu-16-for-8", "a-row+1", "b-row+1", "row-past-m", "col-past-n")

# stream_gemm configurations: (weight rows per workgroup, largest M, fragment-layout weights), from the
# table in stream_gemm.hip (test_gemm_exact_cpu.py compares it with the built extension's answers)
_RM, _SH = False, True
STREAM_CFG = {
    0: (64, 128, _RM), 1: (128, 128, _RM), 2: (64, 128, _RM), 3: (64, 128, _RM), 4: (128, 128, _RM), 5: (128, 128, _RM),
    6: (64, 64, _RM), 7: (64, 64, _RM), 8: (128, 64, _RM), 9: (64, 128, _SH), 10: (128, 128, _SH), 11: (64, 128, _SH),
    12: (64, 64, _SH), 13: (128, 64, _SH), 14: (128, 128, _SH), 15: (128, 128, _SH), 16: (128, 64, _SH),
    20: (112, 128, _SH), 21: (96, 128, _SH), 22: (112, 128, _SH), 23: (96, 128, _SH), 24: (128, 256, _SH),
    25: (64, 256, _SH), 26: (128, 256, _SH), 27: (64, 256, _SH), 28: (192, 128, _SH), 29: (192, 128, _SH),
    30: (128, 16, _SH), 31: (128, 32, _SH), 32: (16, 16, _SH), 33: (32, 16, _SH), 34: (32, 128, _SH), 35: (48, 128, _SH),
    36: (64, 128, _SH), 37: (64, 128, _SH), 41: (112, 128, _SH), 42: (112, 128, _SH)}
STREAM_ABLATIONS = (17, 18, 19, 38, 39, 40)
STREAM_PRODUCTION = (10, 13, 20, 27, 28, 30, 31)


def _trunc32(c):
    return (c.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def oracle(defect=None):
    """ops/reference.py's arithmetic behind the entry points the runners call, writing through the given
    views; ``defect`` plants one mistake."""
    assert defect is None or defect in DEFECTS

    def store(c):
        return _trunc32(c) if defect == "trunc" else c.to(BF)

    def operands(A, B, shuffled, N, b_group):
        M = A.shape[0]
        Af = A.float()
        if defect == "a-row+1":  # the last valid row reads the row behind it
            Af = Af.clone()
            Af[M - 1] = _past(A, rows=1)[M].float()
        Bu = unshuffle_weights(B, b_group).float() if shuffled else B.float()
        Bf = Bu[:N]
        if defect == "b-row+1":  # the last valid row of B is the copy's first padding row / the guard row
            Bf = Bf.clone()
            Bf[N - 1] = Bu[N] if Bu.shape[0] > N else _past(B, rows=1)[N].float()
        return Af, Bf

    def product(Af, Bf):
        c = Af @ Bf.t()
        K = Af.shape[1]
        if defect == "k-last":
            c = c - Af[:, K - 1:] @ Bf[:, K - 1:].t()
        if defect == "k-chunk-twice":  # chunk 0 in place of chunk 1
            c = c + Af[:, :32] @ Bf[:, :32].t() - Af[:, 32:64] @ Bf[:, 32:64].t()
        return c

    def epilogue(c, bias, residual, epi, out_f32):
        M, N = c.shape
        if bias is not None:
            b = bias.float()
            if defect == "bias-by-m":
                c = c + b[torch.arange(M) % N][:, None]
            elif defect == "bias-late" and epi == ref.EPI_NONE and not out_f32:
                c = store(c).float() + b
            else:
                c = c + b
        if epi == ref.EPI_GELU:
            # fp32, in the erfc form: torch's 0.5 x (1 + erf(x / sqrt 2)) is 2.7e-7 off at x = -4.8, outside
            # the 2e-7 that test_gelu_erf_sweep holds the kernel to down there
            c = 0.5 * c * torch.special.erfc(-c * math.sqrt(0.5))
        elif epi in (ref.EPI_SWIGLU, ref.EPI_SWIGLU8):
            hg = 16 if epi == ref.EPI_SWIGLU or defect == "swiglu-16-for-8" else 8
            v = c.view(M, N // (2 * hg), 2, hg)
            c = (F.silu(v[:, :, 0]) * v[:, :, 1]).reshape(M, N // 2)
        if residual is not None:
            c = (c if out_f32 or defect == "res-early" else store(c).float()) + residual.float()
        return c if out_f32 else store(c)

    def write(out, y):
        out.copy_(y)
        if defect == "row-past-m":
            _past(out, rows=1)[out.shape[0]] = y[-1]
        if defect == "col-past-n":
            _past(out, cols=1)[:, out.shape[1]] = y[:, -1]
        return out

    epilogue_fn = epilogue

    def gemm_bt(A, B, bias=None, residual=None, epilogue=ref.EPI_NONE, out_f32=False, row_group=None, q_group=None,
                allow=None, out=None, shuffled=False, n=None, b_group=1):
        N = B.shape[0] if n is None else int(n)
        Af, Bf = operands(A, B, shuffled, N, b_group)
        if epilogue == ref.EPI_SCORES:
            return write(out, ref.gemm_bt(Af, Bf, None, None, epilogue, out_f32, row_group, q_group, allow))
        return write(out, epilogue_fn(product(Af, Bf), bias, residual, epilogue, out_f32))

    def gemm256_into(A, B, out, bias, residual, epi, shuffled, b_group=1):
        Af, Bf = operands(A, B, shuffled, B.shape[0], b_group)
        return write(out, epilogue_fn(product(Af, Bf), bias, residual, epi, False))

    def gemm_mid(A, B, residual=None, epilogue=ref.EPI_NONE, out=None, variant=0, b_group=1):
        Af, Bf = operands(A, B, True, B.shape[0], b_group)
        c = product(Af, Bf)
        if defect == "mid-drop-segment":  # the first split tile loses its second segment's partial
            d = mid_decomposition(A.shape[0], B.shape[0], A.shape[1], 32 if variant % 1000 == 32 else 64)
            for t, n_seg in enumerate(d.segments):
                if n_seg > 1:
                    k0, k1 = d.ranges(t)[1]
                    rows = slice(256 * t, 256 * t + 256)
                    c[:, rows] -= Af[:, k0:k1] @ Bf[rows, k0:k1].t()
                    break
        return write(out, epilogue_fn(c, None, residual, epilogue, False))

    def stream_gemm(x, w, splits=1, epilogue=ref.EPI_NONE, residual=None, out=None, nt=False, cfg=0, norm_eps=0.0,
                    slab_dtype=torch.float32, w_group=1):
        Af, Bf = operands(x, w, STREAM_CFG[cfg][2], w.shape[0], w_group)
        if splits == 1:
            return write(out, epilogue_fn(product(Af, Bf), None, residual, epilogue, False))
        kc = x.shape[1] // splits
        for s in range(splits):  # (the K defects: in the first slice)
            a, b = Af[:, s * kc:(s + 1) * kc], Bf[:, s * kc:(s + 1) * kc]
            out[s] = product(a, b) if s == 0 else a @ b.t()
        return out

    def slab_reduce(slabs, residual=None, out=None):
        S = slabs.shape[0]
        c = slabs[:S - 1 if defect == "slab-skip" and S > 1 else S].float().sum(0)
        return write(out, epilogue_fn(c, None, residual, ref.EPI_NONE, False))

    return SimpleNamespace(gemm_bt=gemm_bt, stream_gemm=stream_gemm, slab_reduce=slab_reduce, defect=defect,
                           kernels=SimpleNamespace(_gemm256_into=gemm256_into, gemm_mid=gemm_mid))


# ------------------------------------------------------------------------------------------------
# jobs: operands on the device, one launch, the checks


def _epi_args(c, epi, dev, n_out):
    """(bias view, residual view, epilogue code, out_f32) of an epilogue name."""
    bias = vector(c.bias, dev)[1] if epi in ("bias", "bias_residual", "gelu", "swiglu_bias") else None
    res = None
    if epi in ("residual", "bias_residual"):
        res = guarded(c.res if epi == "residual" else c.res_b, dev, RES_PAD)[1]
    return bias, res, EPI_CODE.get(epi, ref.EPI_NONE), epi == "f32"


class Job:
    """One launch: ``launch(impl)`` enqueues it, ``check()`` reads the buffers back."""

    def __init__(self, kind, dev, M, N, K, layout, epi, b_group=1, variant=0, cfg=0, nt=False):
        self.kind, self.M, self.N, self.K, self.layout, self.epi = kind, M, N, K, layout, epi
        self.b_group, self.variant, self.cfg, self.nt = b_group, variant, cfg, nt
        self.name = f"{kind} {M} x {N} x {K} {layout} {epi}" + (f" b_group {b_group}" if b_group > 1 else "") + (
            f" variant {variant}" if variant else "") + (f" cfg {cfg} nt {nt}" if kind == "stream" else "")
        c = case_of(M, N, K, epi)
        self.n_out = N // 2 if epi in ("swiglu", "swiglu_bias", "swiglu8") else N
        self.A = guarded(c.A, dev)[1]
        self.B = shuffled_copy(c.B, dev, b_group)[1] if layout == "shuf" else guarded(c.B, dev)[1]
        self.bias, self.res, self.code, self.f32 = _epi_args(c, epi, dev, self.n_out)
        self.buf, self.out = out_view(M, self.n_out, dev, torch.float32 if self.f32 else BF)
        assert self.A.stride(0) != self.out.stride(0) and (self.res is None or self.res.stride(0) != self.out.stride(0))

    def launch(self, impl):
        sh = self.layout == "shuf"
        if self.kind == "bt":
            impl.gemm_bt(self.A, self.B, self.bias, self.res, epilogue=self.code, out_f32=self.f32, out=self.out,
                         shuffled=sh, n=self.N if sh else None, b_group=self.b_group)
        elif self.kind == "g256":
            impl.kernels._gemm256_into(self.A, self.B, self.out, self.bias, self.res, self.code, sh, self.b_group)
        elif self.kind == "mid":
            impl.kernels.gemm_mid(self.A, self.B, residual=self.res, epilogue=self.code, out=self.out,
                                  variant=self.variant, b_group=self.b_group)
        else:
            impl.stream_gemm(self.A, self.B, epilogue=self.code, residual=self.res, out=self.out, cfg=self.cfg,
                             nt=self.nt)
        return self

    def check(self):
        E, low = expected(self.M, self.N, self.K, self.epi)
        if not untouched(self.buf, self.M, self.n_out):
            return _failed(self.name, "memory outside the output view was written")
        if self.epi in ACT:
            return check_act(self.name, self.out, E, low)
        return check_same(self.name, self.out, E)


def run_job(impl, dev, kind, M, N, K, layout, epi, **kw):
    return Job(kind, dev, M, N, K, layout, epi, **kw).launch(impl).check()


def run_jobs(impl, dev, kind, M, N, K, layout, epis, **kw):
    """{epilogue: Report}."""
    return {epi: run_job(impl, dev, kind, M, N, K, layout, epi, **kw) for epi in epis}


def worst(reports):
    reports = list(reports.values()) if isinstance(reports, dict) else list(reports)
    w = max(reports, key=lambda r: r.ratio)
    return Report(w.name, w.ratio, w.row, w.col, sum(r.n_bad for r in reports))


# ---- EPI_SCORES


def _allowed(M, n, row_group, q_group, allow):
    ok = torch.ones(M, n, dtype=torch.bool)
    if row_group is not None:
        rg = row_group.long()[None, :n]
        ok &= rg >= 0
        if q_group is not None:
            qg = q_group.long()[:, None]
            ok &= (qg < 0) | (rg == qg)
    if allow is not None:
        idx = torch.arange(n)
        ok &= ((allow[:, idx // 32].long() >> (idx % 32)) & 1).bool()
    return ok


def run_scores(impl, dev, M, N, K, layout):
    """fp32 filtered scores: all three masks, then the allow mask alone.  On the fragment layout the copy
    has more rows than ``n`` (NaN rows), and so has a copy with a whole spare 16-row block."""
    c = exact_case(M, N, K)
    g = _gen("scores", M, N, K)
    rgrp = torch.randint(-1, 3, (N,), generator=g).to(torch.int32)
    qgrp = torch.randint(-1, 3, (M,), generator=g).to(torch.int32)
    allow = torch.randint(-2 ** 31, 2 ** 31, (M, -(-N // 32)), generator=g).to(torch.int32)
    A = guarded(c.A, dev)[1]
    reps = []
    for masks in ((rgrp, qgrp, allow), (None, None, allow), (rgrp, None, None)):
        rows = [None, -(-N // 16) * 16 + 16] if layout == "shuf" else [None]
        for R in rows:
            B = shuffled_copy(c.B, dev, rows=R)[1] if layout == "shuf" else guarded(c.B, dev)[1]
            buf, out = out_view(M, N, dev, torch.float32)
            dm = [None if m is None else m.to(dev) for m in masks]
            impl.gemm_bt(A, B, epilogue=ref.EPI_SCORES, out_f32=True, row_group=dm[0], q_group=dm[1], allow=dm[2],
                         out=out, shuffled=layout == "shuf", n=N if layout == "shuf" else None)
            name = f"scores {M} x {N} x {K} {layout} masks {[m is not None for m in masks]} copy rows {R}"
            E = c.C.masked_fill(~_allowed(M, N, *masks), -INF)
            if not untouched(buf, M, N):
                reps.append(_failed(name, "memory outside the output view was written"))
                continue
            got = out.detach().cpu()
            if not torch.equal(torch.isneginf(got), torch.isneginf(E)):
                reps.append(_failed(name, "-inf pattern differs"))
                continue
            fin = ~torch.isneginf(E)
            zero = torch.zeros_like(E)
            reps.append(check_same(name, torch.where(fin, got, zero), torch.where(fin, E, zero)))
    return worst(reps)


# ---- stream_gemm and slab_reduce


def stream_n(cfg):
    bn = STREAM_CFG[cfg][0]
    return 2 * bn if (2 * bn) % 32 == 0 else 4 * bn


def stream_ms(cfg):
    mm = STREAM_CFG[cfg][1]
    return sorted({m for m in (1, 16, 17, mm - 1, mm) if m <= mm})


def stream_epis(cfg):
    """S = 1 outputs of a configuration: bf16 (+ residual), SwiGLU (32-row tiles only), SwiGLU8."""
    return ("none", "residual") + (("swiglu",) if STREAM_CFG[cfg][0] % 32 == 0 else ()) + ("swiglu8",)


def run_stream(impl, dev, cfg, M, K, S, nt=False):
    """{name: Report} of one (cfg, M, K, S): S = 1: every ``stream_epis`` output through strided views;
    S > 1: fp32 slabs (their sum is C), ``slab_reduce`` of them without and with a residual.  ``nt``: the
    instantiation that streams the weights with non-temporal loads."""
    N = stream_n(cfg)
    layout = "shuf" if STREAM_CFG[cfg][2] else "rm"
    if S == 1:
        return run_jobs(impl, dev, "stream", M, N, K, layout, stream_epis(cfg), cfg=cfg, nt=nt)
    c = exact_case(M, N, K)
    A = guarded(c.A, dev)[1]
    B = shuffled_copy(c.B, dev)[1] if layout == "shuf" else guarded(c.B, dev)[1]
    sbuf = torch.full((S + 2, M, N), SENTINEL, dtype=torch.float32, device=dev)
    slabs = sbuf[1:1 + S]
    impl.stream_gemm(A, B, splits=S, out=slabs, cfg=cfg, nt=nt)
    tag = f"stream cfg {cfg} nt {nt} {M} x {N} x {K} S {S}"
    reps = {}
    sb = sbuf.detach().cpu()
    if not bool((sb[0] == SENTINEL).all() and (sb[-1] == SENTINEL).all()):
        reps["slabs"] = _failed(tag, "memory outside the slabs was written")
    else:
        reps["slabs"] = check_same(tag + " slab sum", sb[1:1 + S].double().sum(0).float(), c.C)
    for epi in ("none", "residual"):
        res = guarded(c.res, dev, RES_PAD)[1] if epi == "residual" else None
        buf, out = out_view(M, N, dev)
        impl.slab_reduce(slabs, res, out=out)
        name = f"{tag} slab_reduce {epi}"
        reps["reduce_" + epi] = (check_same(name, out, expected(M, N, K, epi)[0]) if untouched(buf, M, N)
                                 else _failed(name, "memory outside the output view was written"))
    return reps


# ------------------------------------------------------------------------------------------------
# the case tables (shared by the CPU self-test and the GPU tests)

LAYOUTS = ("rm", "shuf")

BT_SHAPES = ((1, 4, 64), (127, 132, 64), (129, 260, 192), (300, 1000, 256))
BT_SWIGLU_SHAPES = ((1, 160, 64), (127, 160, 64), (129, 288, 192), (300, 288, 256))
BT_EPIS = EXACT + ("gelu",)
BT_SWIGLU_EPIS = ("swiglu", "swiglu_bias", "swiglu8")
BT_BIG = (2049, 4640, 64)  # N % 256 = 32 keeps gemm256 off; 9 x 19 = 171 tiles of 256 x 256
BT_BIG_EPIS = BT_EPIS + BT_SWIGLU_EPIS

G256_SHAPES = tuple((M, N, K) for M in (1, 255, 257, 513) for N in (256, 512) for K in (128, 384))
G256_BIG = (4100, 4096, 128)  # 17 x 16 = 272 tiles on 256 CUs, a ragged last row tile


def g256_epis(layout):
    return PLAIN + ("gelu", "swiglu") + (("swiglu_bias",) if layout == "rm" else ()) + ("swiglu8",)


MID_M = (1, 129, 300, 640, 1000, 2048, 2100, 4096)  # 1, 2, 3, 5, 8, 16, 17, 32 row tiles
# (the last three: tiles shared by exactly two groups at the 64-deep K-step and a tile that one group keeps
# to itself at the 32-deep one, which the product lacks)
MID_SHAPES = tuple((M, N, K) for M in MID_M for N in (256, 768) for K in (64, 320, 1024)) + (
    (300, 768, 128), (2100, 768, 192), (4096, 2048, 64))
MID_EPIS = ("none", "residual", "swiglu8")
MID_VARIANTS = (0, 32)
MID_GROUPED = (300, 768, 320)  # also on the shuffle_weights(w, 8) copy
MID_BACK_TO_BACK = ((300, 768, 1024), (2100, 256, 320), (1, 256, 64))

STREAM_CFGS = tuple(sorted(STREAM_CFG))
STREAM_KS = ((128, 1), (640, 1), (256, 2), (1536, 4), (2048, 16))

# (layout, M, N, K, the arm ``ops.gemm_bt`` must take)
DISPATCH = (
    ("shuf", 300, 512, 256, "mid"),  # 4 tiles
    ("shuf", 1100, 13312, 128, "mid"),  # 260 tiles: the second wave fills 4 of 256 CUs, fill 0.51
    ("shuf", 1024, 12288, 128, "g256-shuf"),  # 192 tiles, fill 0.75
    ("shuf", 800, 12288, 128, "g256-shuf"),  # wide: M < 1024 with 192 tiles
    ("rm", 1100, 512, 128, "g256-rm"),
    ("rm", 800, 12288, 128, "g256-rm"),  # wide
    ("rm", 129, 260, 192, "bt128-rm"), ("shuf", 129, 260, 192, "bt128-shuf"),
    ("rm", 300, 512, 256, "bt128-rm"),  # gemm256's shape, but M < 1024 and 4 tiles; row-major keeps gemm_mid off
    ("rm", 2049, 4640, 64, "bt256-rm"), ("shuf", 2049, 4640, 64, "bt256-shuf"))
ARMS = ("mid", "g256-rm", "g256-shuf", "bt128-rm", "bt128-shuf", "bt256-rm", "bt256-shuf")


def documented_arm(layout, M, N, K, lda):
    """The dispatch rule of ``ops.gemm_bt`` for a plain bf16 call without a bias, from the docstrings of
    ``use_gemm_mid`` / ``use_gemm256`` and the ``big`` rule of gemm.hip (256 CUs)."""
    tiles = -(-M // 256) * (N // 256)
    fill = tiles / (-(-tiles // 256) * 256) if tiles else 0.0
    mid_ok = N % 256 == 0 and K % 64 == 0 and M <= 4096 and lda >= K
    if layout == "shuf" and mid_ok and (tiles < 192 or fill < 0.7):
        return "mid"
    if N % 256 == 0 and K % 128 == 0 and (M >= 1024 or (M >= 256 and tiles >= 192)):
        return "g256-" + layout
    return ("bt256-" if bt_big(M, N) else "bt128-") + layout
