"""The MXFP4-weight arm of ``gemm_mid`` (``ops.gemm_mid(A, codes, w_scales=...)``, ``gemm_mid_kernel<..., MX>``).

The arm reads the e2m1 codes and E8M0 scale bytes, converts them in registers and feeds the MFMAs the
operands the bf16 kernel reads from the dequantised image, with the same K-steps, split and combine order.
So nothing here is a tolerance: every comparison is ``torch.equal`` -- against the bf16 kernel on
``shuffle_weights(weight_dequantize_mxfp4(...))``, and, independently of that kernel, against a closed form
(one-hot activations pick single dequantised weights)."""
import pytest
import torch

from django_assistant_bot_amd import ops
from django_assistant_bot_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
# the scale bytes of tests/test_weight_mxfp4_only_gpu.py::test_every_code_under_every_scale_byte_at_known_positions:
# both ends of the range whose products stay normal, and 2^-1 .. 2^1
SCALE_BYTES = (2, 3, 126, 127, 128, 251, 252)
CANARY = -7.0
CANARY_BYTE = 0xA5

# (M, N, K) and why (the split is recomputed from the device in test_shape_list_covers_the_split):
SHAPES = [
    (16, 256, 128),    # one tile split into the two halves of ONE code fragment (odd-kk segment start)
    (1, 512, 896), (127, 512, 896), (128, 512, 896), (129, 512, 896),  # row-tile edge; K = 7 fragments, deepest combine
    (300, 1792, 512),  # the toy decoder's gate_up
    (300, 2048, 2048),  # groups own 3-4 K-steps, cross tile boundaries and start at odd kk
    (4000, 1024, 384),  # 32 row tiles, 8 groups, K not a multiple of 256
    (4000, 2048, 128),  # 32 row tiles, 8 groups of two K-steps: every tile whole (no other shape has one on 256 CUs)
]


def _weights(N, K, seed):
    """Row-major codes [N, K/2] over all 16 values and scale bytes [N, K/32] within 2^-3 .. 2^3."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scales = torch.randint(124, 131, (N, K // 32), generator=g, dtype=torch.uint8)
    return codes, scales


def _operands(M, N, K, group, seed):
    """(A, shuffled codes, shuffled scales, bf16 fragment image of the dequantised weights, residual) on the GPU."""
    g = torch.Generator().manual_seed(seed + 1)
    codes, scales = _weights(N, K, seed)
    A = (torch.randn(M, K, generator=g) * 0.5).to(BF).to(DEV)
    R = torch.randn(M, N, generator=g).to(BF).to(DEV)
    img = ops.shuffle_weights(ops.weight_dequantize_mxfp4(codes, scales), group).to(DEV)
    return (A, ops.shuffle_weights_mxfp4(codes, group).to(DEV), ops.shuffle_scales_mxfp4(scales).to(DEV), img, R)


def _split(M, N, K, cus):
    """gemm_mid's decomposition (the launcher of gemm_mid.hip): the K-step ranges [start, end) of the groups."""
    grid = cus & ~7
    tiles_m, tiles_n, kt = -(-M // 128), N // 256, K // 64
    gpx = (grid // 8) // tiles_m
    gn = 8 * gpx
    q, r = divmod(tiles_n * kt, gn)
    segs = []
    for j in range(gn):
        s = j * q + min(j, r)
        e = s + q + (1 if j < r else 0)
        if e > s:
            segs.append((s, e))
    return segs, kt


def _traits(M, N, K, cus):
    segs, kt = _split(M, N, K, cus)
    whole = odd = spans = False
    for s, e in segs:
        spans |= (e - 1) // kt > s // kt
        it = s
        while it < e:  # the group's segments, one per tile it touches
            nt, k0 = divmod(it, kt)
            k1 = min(kt, k0 + e - it)
            whole |= k0 == 0 and k1 == kt
            odd |= k0 > 0 and k0 % 2 == 1
            it += k1 - k0
    return whole, odd, spans


def test_shape_list_covers_the_split():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t = [_traits(M, N, K, cus) for M, N, K in SHAPES]
    assert any(w for w, _, _ in t), "no shape with a whole (unsplit) tile"
    assert any(o for _, o, _ in t), "no split tile whose later segment starts at an odd K-step"
    assert any(s for _, _, s in t), "no group that spans two weight tiles"
    assert _traits(16, 256, 128, cus)[1]  # the two halves of one fragment


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_bit_equal_to_the_bf16_kernel(M, N, K):
    for epi, group, res in ((ops.EPI_NONE, 1, False), (ops.EPI_NONE, 1, True), (ops.EPI_SWIGLU8, 8, False),
                            (ops.EPI_NONE, 8, True)):
        A, c4, sc, img, R = _operands(M, N, K, group, 3 * M + N + K + group)
        kw = dict(residual=R if res else None, epilogue=epi, b_group=group)
        want = ops.gemm_mid(A, img, **kw)
        got = ops.gemm_mid(A, c4, w_scales=sc, **kw)
        assert got.shape == want.shape == (M, N // 2 if epi == ops.EPI_SWIGLU8 else N)
        assert bool(torch.isfinite(want.float()).all()) and bool(want.float().abs().sum() > 0)
        assert torch.equal(got, want), (M, N, K, epi, group, res)
        for conv in (1, 2):  # both placements of the conversion
            assert torch.equal(ops.gemm_mid(A, c4, w_scales=sc, convert=conv, **kw), want), conv


@pytest.mark.parametrize("group", [1, 8])
def test_closed_form_every_code_under_every_scale_byte(group):
    """A is the identity (row m one-hot at k = m), so C[m, n] must be the dequantised W[n, m] exactly.  W is
    zero but for one non-zero code per (code, scale byte) pair, each in an MX block of its own at a written
    down (row, k): pins the half / byte / nibble / scale-byte map of the arm without the bf16 kernel."""
    M = N = K = 256
    lut = torch.tensor(ref.MXFP4_GRID + tuple(-v for v in ref.MXFP4_GRID), dtype=torch.float64)
    codes = torch.zeros((N, K // 2), dtype=torch.uint8)
    scales = torch.full((N, K // 32), 127, dtype=torch.uint8)
    want = torch.zeros((N, K), dtype=torch.float64)
    where, slots, nib, kins = set(), set(), set(), set()
    for p, (c, s) in enumerate((c, s) for c in range(16) for s in SCALE_BYTES):
        row, blk, kin = (7 * p + 3) % N, (5 * p + 1) % (K // 32), (3 * p + p // 8) % 32
        k = 32 * blk + kin
        assert (row, blk) not in where
        where.add((row, blk))
        slots.add(blk % 4)
        nib.add(k & 1)
        kins.add(kin)
        codes[row, k // 2] |= c << (4 * (k & 1))
        scales[row, blk] = s
        want[row, k] = lut[c] * 2.0 ** (s - 127)
    assert slots == {0, 1, 2, 3} and nib == {0, 1} and kins == set(range(32))
    assert {b for _, b in where} == set(range(K // 32)) and len({r // 16 for r, _ in where}) == N // 16
    A = torch.eye(M, K, dtype=BF, device=DEV)
    got = ops.gemm_mid(A, ops.shuffle_weights_mxfp4(codes, group).to(DEV), w_scales=ops.shuffle_scales_mxfp4(scales).to(DEV),
                       b_group=group)
    assert torch.equal(got.cpu().double(), want.t())  # (every product is a bf16)
    assert int((got != 0).sum()) == 14 * len(SCALE_BYTES)  # (codes 0 and 8 are zeros)


def _guard_rows(x, pad, fill=CANARY):
    """(buffer, view): x [R, C] as rows [3, 3 + R) and the first C columns of a canary buffer with row stride C + pad."""
    R, C = x.shape
    buf = torch.full((R + 6, C + pad), fill, dtype=x.dtype, device=DEV)
    buf[3:3 + R, :C] = x
    return buf, buf[3:3 + R, :C]


def _guard_bytes(x, front):
    """(buffer, contiguous view of the uint8 tensor x) between ``front`` and 64 canary bytes."""
    buf = torch.full((front + x.numel() + 64,), CANARY_BYTE, dtype=torch.uint8, device=DEV)
    view = buf[front:front + x.numel()].view(x.shape)
    view.copy_(x)
    return buf, view


@pytest.mark.parametrize("epi,group,res", [(ops.EPI_NONE, 1, True), (ops.EPI_SWIGLU8, 8, False)])
def test_guarded_buffers(epi, group, res):
    M, N, K = 300, 512, 384  # the last row tile holds 44 rows
    A0, c0, s0, img, R0 = _operands(M, N, K, group, 77 + group)
    n_out = N // 2 if epi == ops.EPI_SWIGLU8 else N
    abuf, A = _guard_rows(A0, 8)
    rbuf, R = _guard_rows(R0, 24)
    obuf, out = _guard_rows(torch.full((M, n_out), CANARY, dtype=BF, device=DEV), 16)
    cbuf, c4 = _guard_bytes(c0, 64)
    sbuf, sc = _guard_bytes(s0, 68)  # 4-byte aligned, not 16
    assert c4.data_ptr() % 16 == 0 and sc.data_ptr() % 16 == 4 and A.stride(0) == K + 8
    before = [t.clone() for t in (abuf, rbuf, cbuf, sbuf)]
    want = ops.gemm_mid(A0, img, residual=R0 if res else None, epilogue=epi, b_group=group)
    ret = ops.gemm_mid(A, c4, w_scales=sc, residual=R if res else None, epilogue=epi, b_group=group, out=out)
    torch.cuda.synchronize()
    assert ret.data_ptr() == out.data_ptr() and torch.equal(out, want)
    for t, b in zip((abuf, rbuf, cbuf, sbuf), before):  # inputs and their canaries
        assert torch.equal(t, b)
    ob = obuf.clone()
    ob[3:3 + M, :n_out] = CANARY
    assert bool((ob == CANARY).all())  # nothing outside [M, n_out]: rows >= M of the last tile, guard columns


def test_refusals_leave_out_untouched(monkeypatch):
    nat = ops.native()
    M, N, K = 300, 512, 384
    A, c4, sc, img, R = _operands(M, N, K, 1, 5)
    out = torch.full((M, N), CANARY, dtype=BF, device=DEV)
    launched = []
    for name in ("gemm_mid", "gemm_mid_mxfp4", "gemm256", "gemm_bt"):
        real = getattr(nat, name)
        monkeypatch.setattr(nat, name, lambda *a, _r=real, _n=name, **k: launched.append(_n) or _r(*a, **k))
    off4 = torch.empty(sc.numel() + 4, dtype=torch.uint8, device=DEV)[2:2 + sc.numel()].view(sc.shape).copy_(sc)
    off16 = torch.empty(c4.numel() + 16, dtype=torch.uint8, device=DEV)[8:8 + c4.numel()].view(c4.shape).copy_(c4)
    A64, c64, s64 = A[:, :320].contiguous(), c4[:, :160].contiguous(), sc[:, :10].contiguous()  # K % 128 != 0, K % 64 == 0
    bad = [
        dict(A=A64, B=c64, w_scales=s64),
        dict(w_scales=off4), dict(B=off16),
        dict(B=c4.to(torch.int8)), dict(w_scales=sc.to(torch.int32)), dict(A=A.float()), dict(B=img),
        dict(w_scales=sc[:, :-1].contiguous()), dict(w_scales=sc[:-16].contiguous()), dict(B=c4[:, :-64].contiguous()),
        dict(w_scales=sc.flatten()), dict(w_scales=sc.t().contiguous().t()),
        dict(variant=64), dict(variant=1000), dict(variant=32), dict(convert=3),
        dict(residual=R[:, :-8].contiguous()), dict(residual=R, epilogue=ops.EPI_SWIGLU8),
        dict(out=out.float()), dict(b_group=4), dict(w_scales=sc.cpu()),
    ]
    for kw in bad:
        args = dict(A=A, B=c4, w_scales=sc, out=out)
        args.update(kw)
        a, b = args.pop("A"), args.pop("B")
        with pytest.raises(ValueError):
            ops.gemm_mid(a, b, **args)
    # gemm_bt: a shape outside use_gemm_mid (found with the predicate itself), and its other refusals
    big = next(m for m in (1024, 2048, 4096, 8192) if not ops.kernels.use_gemm_mid(m, N, K, K))
    Ab = torch.zeros((big, K), dtype=BF, device=DEV)
    with pytest.raises(ValueError, match="no other kernel reads"):
        ops.gemm_bt(Ab, c4, w_scales=sc, shuffled=True)
    for kw in (dict(shuffled=False), dict(shuffled=True, as_m=400), dict(shuffled=True, bias=R[0].contiguous()),
               dict(shuffled=True, rows=torch.zeros(4, dtype=torch.int32, device=DEV)), dict(shuffled=True, out_f32=True),
               dict(shuffled=True, epilogue=ops.EPI_GELU), dict(shuffled=True, w_exps=sc[:, 0].contiguous())):
        with pytest.raises(ValueError):
            ops.gemm_bt(A, c4, w_scales=sc, out=out, **kw)
    assert launched == []
    monkeypatch.undo()
    # the native entry itself: hipErrorInvalidValue before any launch
    st = torch.cuda.current_stream().cuda_stream
    slabs, cnt = ops.kernels._mid_workspace(A.device, st)

    def raw(A_=A.data_ptr(), B_=c4.data_ptr(), S_=sc.data_ptr(), C_=out.data_ptr(), K_=K, N_=N, M_=M, epi=0, grp=1, conv=0,
            res=0):
        nat.gemm_mid_mxfp4(A_, K, B_, S_, C_, N, res, N, M_, N_, K_, epi, slabs.data_ptr(), slabs.numel() * 4,
                           cnt.data_ptr(), cnt.numel(), st, grp, conv)

    assert nat.gemm_mid_mxfp4_ok(M, N, K, K) and not nat.gemm_mid_mxfp4_ok(M, N, 320, 320) and nat.gemm_mid_ok(M, N, 320, 320)
    for kw in (dict(K_=320), dict(K_=0), dict(N_=N + 128), dict(M_=0), dict(M_=1 << 20), dict(B_=c4.data_ptr() + 8),
               dict(S_=sc.data_ptr() + 2), dict(B_=0), dict(S_=0), dict(A_=0), dict(C_=0), dict(grp=4), dict(epi=1),
               dict(epi=4, res=R.data_ptr()), dict(conv=3), dict(conv=-1)):
        with pytest.raises(RuntimeError, match="gemm_mid_mxfp4"):
            raw(**kw)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    raw()
    assert torch.equal(out, ops.gemm_mid(A, img))
    assert torch.equal(ops.gemm_bt(A, c4, w_scales=sc, shuffled=True, residual=R), ops.gemm_bt(A, img, shuffled=True, residual=R))


def test_back_to_back_and_graph_replay_give_identical_bytes():
    M, N, K = 300, 2048, 2048
    A, c4, sc, img, R = _operands(M, N, K, 1, 9)
    want = ops.gemm_mid(A, img, residual=R)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o1 = ops.gemm_mid(A, c4, w_scales=sc, residual=R)
        o2 = ops.gemm_mid(A, c4, w_scales=sc, residual=R)  # back to back on one stream and one workspace
        st = side.cuda_stream
        flags = ops.kernels._mid_workspace(A.device, st)[1]
    side.synchronize()
    assert torch.equal(o1, want) and torch.equal(o2, want)
    assert int(flags.abs().sum()) == 0
    out = torch.full((M, N), CANARY, dtype=BF, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ops.gemm_mid(A, c4, w_scales=sc, residual=R, out=out)
    for _ in range(3):
        out.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        assert int(flags.abs().sum()) == 0  # the ready flags are left zero
