"""The attention kernels on inputs where one key decides a row (tests/attn_cases.py): needle rows must
return the position code of exactly their needle key (|out - code| <= 2^-8), with anti-needles on every
key that must stay invisible (past the causal diagonal, the tail of the last KV block, a stale block
behind the block-table padding, the neighbouring packed sequences); all other rows take the
signal-relative check against the fp64 reference (tau = 4 f, f from the bf16 emulation, tau <= 1.5e-2)
and today's ``close(atol=2e-2, rtol=2e-2)``.  tests/test_attention_needles_cpu.py shows on the CPU
oracle that these checks catch the off-by-one mistakes they are built for.

Each case names the kernel it reaches (the dispatch conditions are in ``flash_attention()`` and
``paged_decode_attention()`` of csrc/kernels/attention.hip).

Largest observed relative error / f per kernel family on an MI355X (the bound is 4; f is 2.4e-3 to
3.9e-3 on the plain cases, so every tau is 4 f or the 1.5e-2 cap, which only the D 32 / 64 cases
reach).  Every needle row returned its code exactly (deviation 0.0):

    decode two-slot DMA (D 128)       1.09   (dec_d-bs128-s8 plain, unsplit)
    decode one-slot DMA (D 128)       0.95   (dec_b-p2048 plain, split)
    decode register path (D 64)       1.07   (dec_c-s4 plain, unsplit)
    flash_d128 unpaired               1.25   (pre_f-n plain)
    flash_d128 paired                 1.23   (pre_g2 plain)
    flash_fwd paged (D 64 / 32)       1.22   (pre_h-d64-n plain)
    flash_fwd packed (D 32 / 64)      1.00   (pack-d64 plain)
    flash_fwd packed wide (D 128)     1.27   (pack-d128-n plain)
    flash_fwd packed narrow (D 128)   1.00   (pack-d128-short-n plain)

(1.00: the worst row is one the emulation rounds the same way, e.g. a one-key sequence.)
"""
import dataclasses
import math

import pytest
import torch

import attn_cases as ac
from django_assistant_bot_amd import ops
from django_assistant_bot_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _assert(case, out, family, tag):
    rep = ac.check(case, out)
    print(f"NEEDLES family={family!r} case={tag} err/f={rep.ratio} f={rep.f} tau={rep.tau} "
          f"needle_dev={rep.needle_dev} max_abs={rep.close_err}")
    assert torch.isfinite(out.float()).all()
    assert rep.ok, str(rep)
    assert rep.tau is None or rep.tau <= ac.TAU_CAP
    return rep


def _both(name):
    """The needle form of a case and its plain form (every row takes the relative check)."""
    return [(ac.get_case(name, DEV, True), f"{name}/needles"), (ac.get_case(name, DEV, False), f"{name}/plain")]


def _decode(case, tag, family, split, parts=None, **kw):
    ws = None
    if split:
        parts = math.ceil(max(case.klens) / case.part) if parts is None else parts
        ws = ops.DecodeWorkspace(case.B, case.Hq, case.D, parts, DEV)
    out = ac.run(case, ops, workspace=ws, **kw)
    _assert(case, out, family, f"{tag}/{'split' if split else 'unsplit'}")
    if split:  # the in-launch combine leaves its arrival counters at rest, and a relaunch agrees
        assert int(ws.cnt.abs().sum()) == 0
        assert torch.equal(ac.run(case, ops, workspace=ws, **kw), out)
        assert int(ws.cnt.abs().sum()) == 0
    return out


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", ["dec_a-s0", "dec_a-s8"])
def test_decode_two_slot_dma(name, split):
    """Case a -- paged_decode_kernel<128, true, true, 2>: batch * Hkv = 32 <= 64 and a partition of
    <= 8192 keys.  Split: 16 partitions of 512 combined in the launch; unsplit: one partition of 8192
    (the 64 sub-tiles per wave the two-slot kernel's per-lane block ids allow)."""
    for case, tag in _both(name):
        assert case.B * case.Hkv <= 64 and case.bt.shape[1] * case.bs <= 8192
        _decode(case, tag, "decode two-slot DMA (D 128)", split)


def test_decode_two_slot_dma_scale_order_out():
    """Case a with a non-default softmax scale, a shuffled dispatch order and a caller's ``out``."""
    order = torch.tensor([2, 0, 3, 1], dtype=torch.int32, device=DEV)
    for case, tag in _both("dec_a-scale"):
        assert case.scale != 1 / math.sqrt(case.D)
        for split in (True, False):
            out = torch.full_like(case.q, 7.0)
            res = _decode(case, tag, "decode two-slot DMA (D 128)", split, order=order, out=out)
            assert res is out


@pytest.mark.parametrize("name,split", [("dec_b-p512", True), ("dec_b-p512", False), ("dec_b-p2048", True)])
def test_decode_one_slot_dma(name, split):
    """Case b -- paged_decode_kernel<128, true, true, 1>: batch * Hkv = 72 > 64.  Partitions of 512
    (3 for the 1100-key sequence), of 2048 (one: the direct store) and the unsplit launch."""
    for case, tag in _both(name):
        assert case.B * case.Hkv > 64
        _decode(case, tag, "decode one-slot DMA (D 128)", split)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", [n for n in sorted(ac.CASES) if n.startswith("dec_c")])
def test_decode_register_path_d64(name, split):
    """Case c -- paged_decode_kernel<64, true>: register-staged sub-tiles, no LDS-DMA."""
    for case, tag in _both(name):
        assert case.D == 64
        _decode(case, tag, "decode register path (D 64)", split)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", [n for n in sorted(ac.CASES) if n.startswith(("dec_d", "dec_e"))])
def test_decode_block_sizes_and_gqa_groups(name, split):
    """Cases d, e -- the two-slot D 128 kernel with 32- / 128-slot blocks (a 32-key sub-tile is a
    whole block / a quarter of one) and GQA groups of 16 and 2 (the MFMA N dimension full / 14 of 16
    columns padding); split: 3 partitions of 128 keys."""
    for case, tag in _both(name):
        _decode(case, tag, "decode two-slot DMA (D 128)", split)


PREFILL = {
    # case f: pair_wgs = 2 * 8 * 4 = 64 < 256 -> flash_d128_kernel<CAUSAL, VPIPE>, one query block per workgroup
    "pre_f-c": "flash_d128 unpaired", "pre_f-n": "flash_d128 unpaired",
    # case g: 2 pairs * 32 heads * 8 sequences = 512 >= 256 -> flash_d128_kernel<true, true, 4, false, PAIR>,
    # three query blocks: the pair (0, 2) and the odd block 1; (Hq * batch) % 8 == 0: heaviest-first walk
    "pre_g": "flash_d128 paired",
    # pairs_per_wg = 2 (>= 2048 pair workgroups, the headline prefill's form); paired without the heaviest-first
    # walk ((Hq * batch) % 8 != 0); block ids past the two preloaded registers (key tiles >= 64, >= 128)
    "pre_g2": "flash_d128 paired", "pre_g-odd": "flash_d128 paired", "pre_long": "flash_d128 unpaired",
    # case h: flash_fwd_kernel<64 | 32, CAUSAL, PAGED = true, 4, 1> (D 64: the 5-waves-per-SIMD bound)
    "pre_h-d64-c": "flash_fwd paged (D 64 / 32)", "pre_h-d64-n": "flash_fwd paged (D 64 / 32)",
    "pre_h-d32-c": "flash_fwd paged (D 64 / 32)", "pre_h-d32-n": "flash_fwd paged (D 64 / 32)",
}


@pytest.mark.parametrize("name", sorted(PREFILL))
def test_paged_prefill(name):
    for case, tag in _both(name):
        pair_wgs = ((max(case.qlens) + 127) // 128 + 1) // 2 * case.Hq * case.B
        assert (pair_wgs >= 256) == name.startswith("pre_g") and (pair_wgs >= 2048) == (name == "pre_g2")
        assert ((case.Hq * case.B) % 8 != 0) == (name == "pre_g-odd")
        _assert(case, ac.run(case, ops), PREFILL[name], tag)


@pytest.mark.parametrize("causal", [True, False])
def test_paged_prefill_strided_q_and_rope_on_load(causal):
    """Case i at the shape of case f (flash_d128, unpaired).  q read as a strided view of a fused qkv
    buffer keeps its needles; with ``rope=`` the kernel rotates q on load, which turns a needle's q
    away from its key, so that path is compared bit for bit with the RoPE kernel's rotated q instead
    (and, on the plain case, against the fp64 reference of that rotated q)."""
    name = "pre_f-c" if causal else "pre_f-n"
    case = ac.get_case(name, DEV, True)
    T, Hq, Hkv, D = case.q.shape[0], case.Hq, case.Hkv, case.D
    W = (Hq + 2 * Hkv) * D
    fused = torch.randn(T, W, device=DEV).to(torch.bfloat16)
    fused[:, :Hq * D] = case.q.reshape(T, Hq * D)
    qv = fused[:, :Hq * D].view(T, Hq, D)
    assert qv.stride(0) == W
    out = ac.run(dataclasses.replace(case, q=qv), ops)
    _assert(case, out, "flash_d128 unpaired", f"{name}/strided-q")

    plain = ac.get_case(name, DEV, False)
    fused[:, :Hq * D] = plain.q.reshape(T, Hq * D)
    pos = torch.cat([torch.arange(n - m, n, dtype=torch.int32) for n, m in zip(plain.klens, plain.qlens)]).to(DEV)
    cs = ref.rope_cos_sin(ref.llama3_inv_freq(D, 500000.0, None), 512).to(DEV)
    scratch = torch.zeros(1, Hkv, plain.bs, D, dtype=torch.bfloat16, device=DEV)
    skip = torch.full((T,), -1, dtype=torch.int64, device=DEV)  # q only: no cache slot is written
    q_rot = ops.rope_kv_write(fused, pos, cs, scratch, scratch.clone(), skip, Hq, Hkv, D)
    rotated = dataclasses.replace(plain, q=q_rot, _cache={})
    a = ac.run(rotated, ops)
    b = ac.run(dataclasses.replace(plain, q=qv), ops, rope=(pos, cs))
    assert torch.equal(a, b)
    _assert(rotated, a, "flash_d128 unpaired", f"{name}/rope")


PACKED = {
    # D 32 / 64, non-causal: flash_fwd_kernel<D, false, false, 4, 1> (D 64: MINW 5), the encoder kernel
    "pack-d32": "flash_fwd packed (D 32 / 64)", "pack-d64": "flash_fwd packed (D 32 / 64)",
    # D 128, max_seqlen_q = 129 > 64: flash_fwd_kernel<128, CAUSAL, false, 8, 1>, 128-query blocks
    "pack-d128-c": "flash_fwd packed wide (D 128)", "pack-d128-n": "flash_fwd packed wide (D 128)",
    # D 128, every sequence <= 64 rows: flash_fwd_kernel<128, CAUSAL, false, 4, 1>
    "pack-d128-short-c": "flash_fwd packed narrow (D 128)", "pack-d128-short-n": "flash_fwd packed narrow (D 128)",
    # cu_q != cu_k: q is the last m rows of each sequence (wide kernel: max_seqlen_q = 128)
    "pack-qtail-c": "flash_fwd packed wide (D 128)", "pack-qtail-n": "flash_fwd packed wide (D 128)",
}


@pytest.mark.parametrize("name", sorted(PACKED))
def test_packed(name):
    for case, tag in _both(name):
        assert (max(case.qlens) > 64) == ("short" not in name)
        if "qtail" in name:
            assert case.qlens != case.klens
        _assert(case, ac.run(case, ops), PACKED[name], tag)


def test_packed_out_is_a_column_slice():
    """``out=`` as a column slice of a wider buffer: the needles land in it, the rest stays."""
    case = ac.get_case("pack-d128-n", DEV, True)
    T, Hq, D = case.q.shape
    buf = torch.full((T, Hq * D + 64), 7.0, dtype=torch.bfloat16, device=DEV)
    out = buf[:, 32:32 + Hq * D].unflatten(1, (Hq, D))
    assert out.stride(0) == Hq * D + 64 and out.data_ptr() == buf.data_ptr() + 64
    res = ac.run(case, ops, out=out)
    assert res.data_ptr() == out.data_ptr()
    _assert(case, out, "flash_fwd packed wide (D 128)", "pack-d128-n/out-slice")
    assert bool((buf[:, :32] == 7.0).all()) and bool((buf[:, 32 + Hq * D:] == 7.0).all())
