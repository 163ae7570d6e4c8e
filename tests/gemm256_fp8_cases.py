"""Cases for the FP8-weight arm of gemm256 (``gemm256_kernel<..., W8>``): operands whose FP8 and dequantised
forms must give bit-equal results, and the guarded candidate launch of the arm's G_CAND epilogue.  The builders of
tests/gemm_cases.py, tests/cand_cases.py and tests/index_fp8_cases.py are imported, not edited.

Weights: random e4m3fn bytes (no NaN codes) with one exponent byte per row, drawn so that neighbouring rows are far
apart: row n gets 127 + (-1)^n (8 + 5 (n % 7)) + (n // 16 % 3), i.e. 87 .. 167 with a jump of 16 .. 76 between
neighbours and between the gate and up halves of every 8-row group.  With |byte value| <= 448 and bf16 activations
of magnitude 2^-4 .. 4, every product and every sum of K <= 4096 terms lies in 2^-60 .. 2^65: far from fp32's
denormals and overflow, so the power-of-two scale commutes with every rounding and the FP8 arm must EQUAL the bf16
kernel on the dequantised weights.  Rows ``EXTREME`` carry the exponent bytes 1 and 254 with four non-zero bytes
each, of magnitude >= 64 (exponent 1: the dequantised value is >= 2^-120, a normal bf16, and its products are
>= 2^-124) or <= 2^-6 (exponent 254: the values are <= 2^121 and a row's sum of four products stays below 2^125).
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import cand_cases as cc
import gemm_cases as gc
import index_fp8_cases as fc
from django_assistant_bot_amd import ops
from django_assistant_bot_amd.ops import reference as ref

G256_SHAPES = gc.G256_SHAPES
G256_BIG = gc.G256_BIG
EPIS = ("none", "residual", "swiglu8")
EXTREME = {5: 1, 22: 254, 133: 254, 250: 1}  # row -> exponent byte (rows of both 128-row halves of the first tile)

CAND_MS = (97, 128, 129, 300, 1025)
CAND_NS = (384, 1000, 65664)
CAND_KS = (256, 768)


def exps_of(N: int) -> torch.Tensor:
    n = np.arange(N)
    e = 127 + np.where(n % 2 == 0, 1, -1) * (8 + 5 * (n % 7)) + (n // 16) % 3
    for r, b in EXTREME.items():
        if r < N:
            e[r] = b
    assert e.min() >= 1 and e.max() <= 254
    return torch.from_numpy(e.astype(np.uint8))


@functools.lru_cache(maxsize=16)
def weights(N: int, K: int, seed: int = 0):
    """(bytes uint8 [N, K], exponent bytes uint8 [N], dequantised bf16 [N, K]); the dequantisation is exact."""
    g = torch.Generator().manual_seed(1000 * N + K + seed)
    data = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32)
    data = torch.where((data & 0x7f) == 0x7f, data & 0x80, data).to(torch.uint8)  # the NaN codes become +-0
    exps = exps_of(N)
    for r, b in EXTREME.items():
        if r >= N:
            continue
        row = torch.zeros(K, dtype=torch.uint8)
        ks = torch.tensor([0, 33, K // 2 + 7, K - 1])
        # e4m3fn: 0x68 = 64, 0xf0 = -128 (exponent byte 1); 0x04 = 2^-7, 0x87 = -7 x 2^-9 (exponent byte 254)
        row[ks] = torch.tensor([0x68, 0xf0, 0x70, 0xe8] if b == 1 else [0x04, 0x87, 0x02, 0x81], dtype=torch.uint8)
        data[r] = row
    dq = ref.weight_dequantize_fp8(data, exps)
    f = data.view(torch.float8_e4m3fn).double() * torch.exp2(exps.double() - 127)[:, None]
    assert dq.dtype == torch.bfloat16 and torch.equal(dq.double(), f) and bool(torch.isfinite(dq).all())
    return data, exps, dq


@functools.lru_cache(maxsize=16)
def activations(M: int, K: int, seed: int = 0) -> torch.Tensor:
    """bf16 [M, K], both signs, magnitudes 2^-4 .. 4."""
    g = torch.Generator().manual_seed(77 * M + K + seed)
    a = torch.randn(M, K, generator=g)
    return (torch.sign(a) * a.abs().clamp(2.0 ** -4, 4.0)).bfloat16()


def copies(N: int, K: int, dev, group: int = 1, seed: int = 0):
    """(FP8 fragment copy, exponents behind an 8-byte guard, bf16 fragment copy of the dequantised weights)."""
    data, exps, dq = weights(N, K, seed)
    ebuf = torch.full((N + 16,), 255, dtype=torch.uint8, device=dev)
    e = ebuf[8:8 + N]
    e.copy_(exps)
    return ops.shuffle_weights_fp8(data, group).to(dev), e, ops.shuffle_weights(dq, group).to(dev)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equality of the stored bits (a NaN equals itself)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16),
                                                                     b.contiguous().view(torch.int16))


def run_epi(dev, M, N, K, epi, group=1, rows=None, seed=0):
    """(FP8 arm's output in a guarded buffer, the bf16 kernel's on the dequantised weights, guard intact)."""
    w8, e, w16 = copies(N, K, dev, group, seed)
    abuf, A = gc.guarded(activations(M, K, seed), dev)
    n = M if rows is None else rows.numel()
    n_out = N // 2 if epi == "swiglu8" else N
    res = None
    if epi == "residual":
        g = torch.Generator().manual_seed(M + N)
        res = gc.guarded(torch.randn(M, N, generator=g).bfloat16(), dev)[1]
    code = ops.EPI_SWIGLU8 if epi == "swiglu8" else ops.EPI_NONE
    buf, out = gc.out_view(n, n_out, dev)
    got = ops.gemm256(A, w8, residual=res, epilogue=code, shuffled=True, b_group=group, rows=rows, out=out, w_exps=e)
    assert got is out
    want = ops.gemm256(A, w16, residual=res, epilogue=code, shuffled=True, b_group=group, rows=rows)
    torch.cuda.synchronize()
    return out, want, gc.untouched(buf, n, n_out)


# ---------------------------------------------------------------------------------------------
# candidates


def cand_launch(dev, M: int, d: cc.Data, thr: np.ndarray, cap: int, grouped: bool) -> cc.Result:
    """The arm's native candidate launcher on guarded buffers, laid out as ``index_fp8_cases.launch`` does for the
    scan: padding rows and a spare 128-row block hold hot rows under the exponent byte ``PAD_EXP`` (a kernel that
    scores a row at n >= N appends it to every list), the exponents sit behind an 8-byte guard."""
    from django_assistant_bot_amd.ops._lib import ptr, stream

    N, K = d.N, d.K
    nat = ops.native()
    abuf = torch.full((M + 2, K + cc.A_PAD), float("nan"), dtype=torch.bfloat16, device=dev)
    A = abuf[1:M + 1, :K]
    A.copy_(d.A[:M])
    rg = torch.from_numpy(d.row_group).to(dev) if grouped else None
    qg = torch.from_numpy(d.q_group[:M].copy()).to(dev) if grouped else None
    t = torch.from_numpy(thr).to(dev)
    res = cc.empty_result(M, cap)
    cnt, val, idx = res.cnt.to(dev), res.val.to(dev), res.idx.to(dev)
    R = -(-N // 128) * 128 + 128
    q, e = ref.kv_quantize(d.B[:N].to(torch.bfloat16))
    assert torch.equal(ref.kv_dequantize(q, e), d.B[:N])
    hot_q, _ = ref.kv_quantize(torch.full((1, K), 2.0, dtype=torch.bfloat16))
    full = hot_q.repeat(R, 1)
    full[:N] = q
    shuf = ops.shuffle_weights_fp8(full.to(dev))
    ebuf = torch.full((8 + R + 8,), fc.PAD_EXP, dtype=torch.uint8, device=dev)
    exps = ebuf[8:8 + R]
    exps[:N] = e.to(dev)
    nat.gemm256_candidates_fp8(ptr(A), A.stride(0), ptr(shuf), ptr(exps), R, M, N, K, ptr(rg), ptr(qg), ptr(t),
                               ptr(cnt), ptr(val[1]), ptr(idx[1]), cap, stream(A), R)
    torch.cuda.synchronize()
    assert bool(torch.isnan(abuf[0]).all() and torch.isnan(abuf[-1]).all() and torch.isnan(abuf[:, K:]).all())
    return cc.Result(cnt.cpu(), val.cpu(), idx.cpu())


def cand_run(dev, M: int, N: int, K: int, grouped: bool):
    """The exact-integer check of ``cand_cases`` on the arm: the main launch (a dense query beside sparse ones, lists
    that hold every hit) and the overflow launch (cap = 64); -> complaints."""
    d = fc.data(N, K, max(96, M))
    out = []
    thr = cc.thresholds(d, M, dense=True)
    cap = N + 8
    out += [f"main: {c}" for c in cc.check(cand_launch(dev, M, d, thr, cap, grouped), d, M, thr, cap, grouped)]
    out += [f"cap 64: {c}" for c in cc.check(cand_launch(dev, M, d, thr, 64, grouped), d, M, thr, 64, grouped)]
    return out


def sorted_lists(val, idx, cnt, cap):
    """Per query, the stored (index, value bits) pairs in index order, as one comparable tensor triple."""
    c = cnt.clamp(max=cap).long()
    live = torch.arange(val.shape[1], device=val.device)[None, :] < c[:, None]
    key = torch.where(live, idx.long(), torch.full_like(idx, 1 << 30, dtype=torch.long))
    order = torch.argsort(key, dim=1)
    return (torch.gather(key, 1, order), torch.where(live, val, torch.zeros_like(val)).gather(1, order).view(torch.int32),
            cnt)
