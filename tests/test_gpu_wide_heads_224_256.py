"""-m gpu: the wide-head forward at head_dim 224 and 256 (`attn_fwd_hd_kernel<T, 224>` / `<T, 256>`, csrc/attention_hd.hip: the
four heads of the TransformerEncoder Memory-Fuser variant at hidden 896 / 1024) against torch float64, on its own.

Small grids with 32 or more key tiles of 32 - any fuser input of 993 tokens or more - cut every (128-query block, head) into
2 .. 7 key planes merged by `attn_combine_kernel` (`mavlm_attention_hd_splits`).  R = 200 query rows (two query blocks, the
second of 72 rows) x 4 heads over the key counts of `SPLIT_CASES` reach every plane count, most with a ragged last key tile and
a last plane shorter than the others (993 keys: two full planes and one key in the last tile; 1600: 50 whole tiles); the plans are literals, asserted against the C library and `O.split_plan_wide`.  The same
operands also go through the never-split grid (`mavlm_attention_hd`); split and plain are each compared with float64, never with
each other.  At 224 the second 128-column sub-image of a head is partly padding (96 of 128 columns).

Reference, gate and inputs are those of tests/test_gpu_streamk_levels.py: `_ref64` (torch float64 on the GPU from the same
16-bit operands), `gpu_util.attention_gate` unchanged (ctx within ATTN_UNIT x floor per (128-query unit, head) and ATTN_WHOLE x
floor over the tensor, lse2 within LSE2_ATOL per row), and the planted rows of `_plant` in every (query block, head): a row
whose maximum arrives in the last plane, a nearly one-hot row in the first, a row for which every other plane's merge weight
underflows.  Every launch is made twice and must repeat bit for bit.  Measured ratios are printed (-s) and tabulated in
tests/README.md."""
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from oracle import memory_path as O
from gpu_util import DT
from test_gpu_streamk_levels import _check_rows, _exact_merge_ratio, _gate, _plant, _randn, _ref64

pytestmark = pytest.mark.gpu
R, H, KT = 200, 4, 32
# keys -> (planes, key tiles per plane) of O.split_plan_wide(200, S, 4) = mavlm_attention_hd_splits
SPLIT_CASES = {993: (2, 16), 1061: (2, 17), 1600: (3, 17), 2117: (4, 17), 2600: (5, 17), 3100: (6, 17), 3950: (7, 18),
               4100: (7, 19)}
S_UNSPLIT = 992                  # 31 key tiles: the last size that is not split


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _plan(S, hd):
    """(planes, tiles per plane) as the C library plans them, checked against the workspace size and the oracle's mirror"""
    lib = capi.lib()
    info = (capi.i32 * 4)()
    capi.check(lib.mavlm_attention_hd_plan_info(R, S, H, hd, info), "plan info")
    ns, tps = O.split_plan_wide(R, S, H)
    assert info[0] == 0 and info[3] == ns
    assert lib.mavlm_attention_hd_ws_floats(R, S, H, hd) == (ns * R * H * hd + ns * H * R if ns > 1 else 0)
    return ns, tps


def _plain(q, k, v, heads, hd, scale):
    """the never-split grid: mavlm_attention_hd (no workspace)"""
    rows = q.shape[0]
    out = torch.empty((rows, heads * hd), device=q.device, dtype=q.dtype)
    lse = torch.empty((heads, rows), device=q.device, dtype=torch.float32)
    capi.check(capi.lib().mavlm_attention_hd(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                             out.data_ptr(), out.stride(0), lse.data_ptr(), rows, k.shape[0], heads, hd, scale,
                                             ops.dtype_code(q.dtype), ops.stream_ptr()), "mavlm_attention_hd")
    return out, lse


def _split(q, k, v, heads, hd, scale):
    return ops.attention(q, k, v, heads, want_lse=True, head_dim=hd, scale=scale)


def _twice(fn, *a):
    ctx, lse = fn(*a)
    again, lse_again = fn(*a)
    assert torch.equal(again, ctx) and torch.equal(lse_again, lse)
    return ctx, lse


_PARAMS = [pytest.param(hd, S, "bf16", id=f"hd{hd}-S{S}-{ns}planes-bf16") for hd in (224, 256) for S, (ns, _) in SPLIT_CASES.items()] + \
          [pytest.param(hd, S, "fp16", id=f"hd{hd}-S{S}-{ns}planes-fp16") for hd in (224, 256) for S, (ns, _) in SPLIT_CASES.items()
           if ns in (2, 7)]


@pytest.mark.parametrize("hd,S,mode", _PARAMS)
def test_every_split_kv_plane_count_and_the_plain_grid_vs_fp64(hd, S, mode):
    ns, tps = _plan(S, hd)
    assert (ns, tps) == SPLIT_CASES[S]
    nt = -(-S // KT)
    rng = [(p * tps, min(nt, (p + 1) * tps)) for p in range(ns)]
    assert rng[-1][1] == nt and rng[-1][1] > rng[-1][0]                                # every plane holds keys
    cuts = [(0, h, b, rng) for h in range(H) for b in range(-(-R // 128))]
    q, k, v = _randn((R, H * hd), 901, mode), _randn((S, H * hd), 902, mode), _randn((S, H * hd), 903, mode)
    rows = _plant([q], [k], H, cuts, f"wide{hd}", R, S)
    assert len(rows) == 2 * H
    scale = ops.attn_scale(hd)
    ref_ctx, ref_lse2, _ = _ref64(q, k, v, H, hd, scale)
    _check_rows(rows, [ref_lse2], H, hd)
    ctx, lse = _twice(_split, q, k, v, H, hd, scale)
    _gate(f"split-KV hd{hd} R{R} S{S} H{H}: {ns} planes of {tps} tiles", ctx, lse, ref_ctx, ref_lse2, H, mode,
          lambda w: _exact_merge_ratio(q, k, v, w[1], hd, scale, w[0] * 128, min(R, w[0] * 128 + 128), rng, KT, mode))
    ctx, lse = _twice(_plain, q, k, v, H, hd, scale)
    _gate(f"plain grid hd{hd} R{R} S{S} H{H}", ctx, lse, ref_ctx, ref_lse2, H, mode)


@pytest.mark.parametrize("hd", [224, 256])
def test_the_last_unsplit_key_count_vs_fp64(hd):
    """31 key tiles: one plane, no workspace - through the same entry as the split sizes."""
    assert _plan(S_UNSPLIT, hd) == (1, 0) and _plan(S_UNSPLIT + 1, hd) == (2, 16)
    mode = "bf16"
    q, k, v = _randn((R, H * hd), 911, mode), _randn((S_UNSPLIT, H * hd), 912, mode), _randn((S_UNSPLIT, H * hd), 913, mode)
    scale = ops.attn_scale(hd)
    ref_ctx, ref_lse2, _ = _ref64(q, k, v, H, hd, scale)
    ctx, lse = _twice(_split, q, k, v, H, hd, scale)
    _gate(f"unsplit hd{hd} R{R} S{S_UNSPLIT} H{H}", ctx, lse, ref_ctx, ref_lse2, H, mode)


@pytest.mark.parametrize("hd,mode", [(224, "bf16"), (256, "bf16"), (224, "fp16"), (256, "fp16")])
def test_the_fuser_call_shape_vs_fp64(hd, mode):
    """MemoryFuser's self-attention: q, k, v are column slices of ONE packed [N, 3 H hd] in_proj output (row stride 3 H hd),
    N = 1100 tokens, 4 heads: 36 units over 35 key tiles in 2 planes of 18."""
    N, W = 1100, H * hd
    lib = capi.lib()
    assert O.split_plan_wide(N, N, H) == (2, 18)
    assert lib.mavlm_attention_hd_ws_floats(N, N, H, hd) == 2 * N * W + 2 * H * N
    qkv = _randn((N, 3 * W), 921, mode)
    q, k, v = qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:]
    assert q.stride(0) == k.stride(0) == v.stride(0) == 3 * W
    before = qkv.clone()
    scale = ops.attn_scale(hd)
    ref_ctx, ref_lse2, _ = _ref64(q, k, v, H, hd, scale)
    ctx, lse = _twice(_split, q, k, v, H, hd, scale)
    assert torch.equal(qkv, before)
    rng = [(0, 18), (18, 35)]
    _gate(f"fuser shape hd{hd} N{N} H{H}: packed qkv, 2 planes", ctx, lse, ref_ctx, ref_lse2, H, mode,
          lambda w: _exact_merge_ratio(q, k, v, w[1], hd, scale, w[0] * 128, min(N, w[0] * 128 + 128), rng, KT, mode))


def test_refusals():
    """A workspace one float short of the plan's: E_ARG; head sizes without a kernel (160, 192, 320): E_SHAPE.  Nothing is
    written in either case."""
    lib = capi.lib()
    S, mode, sentinel = 1061, "bf16", -1234.0
    for hd in (224, 256):
        q, k, v = _randn((R, H * hd), 931, mode), _randn((S, H * hd), 932, mode), _randn((S, H * hd), 933, mode)
        need = lib.mavlm_attention_hd_ws_floats(R, S, H, hd)
        assert need > 0
        ws = torch.empty((need,), device="cuda", dtype=torch.float32)
        out = torch.full((R, H * hd), sentinel, device="cuda", dtype=DT[mode])

        def call(head_dim, ws_floats, ld):
            return lib.mavlm_attention_hd_ws(q.data_ptr(), ld, k.data_ptr(), ld, v.data_ptr(), ld, out.data_ptr(), ld, 0, R, S, H,
                                             head_dim, ops.attn_scale(head_dim), ws.data_ptr(), ws_floats, ops.dtype_code(q.dtype),
                                             ops.stream_ptr())
        assert call(hd, need - 1, H * hd) == capi.E_ARG
        assert call(hd, 0, H * hd) == capi.E_ARG
        torch.cuda.synchronize()
        assert bool((out == sentinel).all())
    for hd in (160, 192, 320):
        W = H * hd
        q, k, v = _randn((R, W), 941, mode), _randn((S, W), 942, mode), _randn((S, W), 943, mode)
        out = torch.full((R, W), sentinel, device="cuda", dtype=DT[mode])
        ws = torch.empty((8 * (R * W + H * R),), device="cuda", dtype=torch.float32)
        a = (q.data_ptr(), W, k.data_ptr(), W, v.data_ptr(), W, out.data_ptr(), W, 0, R, S, H, hd, ops.attn_scale(hd))
        assert lib.mavlm_attention_hd_ws(*a, ws.data_ptr(), ws.numel(), ops.dtype_code(q.dtype), ops.stream_ptr()) == capi.E_SHAPE
        assert lib.mavlm_attention_hd(*a, ops.dtype_code(q.dtype), ops.stream_ptr()) == capi.E_SHAPE
        torch.cuda.synchronize()
        assert bool((out == sentinel).all())
