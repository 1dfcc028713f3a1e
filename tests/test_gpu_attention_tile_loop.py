"""-m gpu: every path of the tile loop of attn_fwd3_kernel (attention3.hip) against torch float64.

The loop has two forms of a tile iteration.  The steady-state pair (tiles t, t + 1) runs while t + 3 < nt: there "tile t + 1
exists and is not the ragged last one" is a compile-time fact, and both phases of both parities are one basic block.  The last
two or three tiles of a segment (the only one, if nt = 1) run the run-time form, which also masks a ragged last tile.  Which
form a tile takes depends on the number of key tiles of its segment only, so the key counts below walk all of them:

  S = 64 n, n = 1 .. 7        nt = 1, 2, 3: tail only (1, 2 and 3 tiles); nt = 4, 5: one steady pair, then a tail of 2 and of 3;
                              nt = 6, 7: two pairs, the same two tails
  S = 64 n - 28               the same with a ragged last tile of 36 keys: masked as the successor of the first, second and
                              third tile of the tail, in either parity
  34 tiles, cut 4-way         a stream-K level of tests/streamk_cases.py whose pieces have 8 and 9 tiles (even and odd), the
                              last one ragged, with the adversarial rows of tests/test_gpu_streamk_levels.py
  F frames of 196 keys        F = 1, 2, 3, 5: 4, 7, 10 and 16 tiles, the last ragged, frame boundaries inside tiles - the
                              frame-score variants, FR = 1 (entries through the workspace) and FR = 3 (entries in LDS)

Workgroups of 4 waves run the plain grid at R = 300 rows and 2 heads (three query blocks of 128, the last of 44 rows).
Workgroups of 8 waves exist under a stream-K plan only, and a plan needs more units than the 256 workgroups: the same 2 heads at
R = 128 * 256 + 300 rows - 130 query blocks of 256, the last of 44 rows; 256 whole units and one 32-way level of 4 units, whose
pieces at these key counts hold one tile or none.  FR = 3 needs 8 waves.

The reference is torch float64 on the GPU from the same 16-bit operands (`_ref64` of tests/test_gpu_streamk_levels.py); the
gate is `gpu_util.attention_gate`, unchanged; frame scores against the float64 column sums with the TOL of the existing frame
tests.  Every launch is made twice and must repeat bit for bit, and ctx / lse2 of the frame-score variants equal the forward
without scores on the same schedule bit for bit (as tests/test_gpu_ops.py and tests/test_gpu_frames_lds.py assert it)."""
import functools

import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from oracle import memory_path as O
from gpu_util import attention_gate, rel_l2_t
import streamk_cases as T
import test_gpu_streamk_levels as L

pytestmark = pytest.mark.gpu
TOL = L.TOL                      # 1e-3: the gate of the existing frame-score tests
H = 2
ROWS = {"w4": 300, "w8": 128 * 256 + 300}
S_MAX = 5 * 196


@pytest.fixture(autouse=True)
def _hooks(request, monkeypatch):
    lib = capi.lib()
    request.addfinalizer(lambda: (lib.mavlm_set_attention_streamk_min_tiles(64), lib.mavlm_set_attention_streamk_waves(0),
                                  lib.mavlm_set_frame_entries_lds(1)))

    def set_hooks(kernel, lds=1):
        capi.check(lib.mavlm_set_attention_streamk_min_tiles(T.MIN_TILES), "min tiles")
        capi.check(lib.mavlm_set_attention_streamk_waves(T.WAVES[kernel]), "waves")
        capi.check(lib.mavlm_set_frame_entries_lds(lds), "entries")
        monkeypatch.setattr(O, "STREAMK_MIN_TILES", T.MIN_TILES)
        monkeypatch.setattr(O, "STREAMK_WAVES", T.WAVES[kernel])
    with torch.no_grad():
        yield set_hooks


@functools.lru_cache(maxsize=4)
def _qkv(kernel, mode):
    """operands of one (workgroup shape, type): computed once, sliced per key count, never modified.  Row 3 is scaled by 8: its
    maximum jumps from tile to tile, so the deferred rescale fires inside the loop (and scales the frame mass)."""
    R = ROWS[kernel]
    q = L._randn((R, H * 128), 911, mode)
    q[3] *= 8.0
    return q, L._randn((S_MAX, H * 128), 912, mode), L._randn((S_MAX, H * 128), 913, mode)


def _plan(kernel, S):
    """(waves, stream-K workgroups, levels, split-KV planes) of the forward's schedule under the hooks in force"""
    info = (capi.i32 * 4)()
    capi.check(capi.lib().mavlm_attention_plan(ROWS[kernel], S, H, info), "plan")
    if kernel == "w8":
        assert list(info) == [8, 256, 1, 1], list(info)        # 8 waves: one whole round, one (32-way) level
    else:
        assert info[0] == 4 and info[1] == 0, list(info)       # 4 waves: no stream-K plan on six units
    return list(info)


def _gate(name, ctx, lse, ref_ctx, ref_lse2, mode):
    g, lerr, ok = attention_gate(ctx, lse, ref_ctx, ref_lse2, H, mode)
    print(f"\n[{name} {mode}] {g}; worst lse2 error {lerr:.2e}")
    assert ok, (name, str(g), lerr)


_KEYS = [64 * n for n in range(1, 8)] + [64 * n - 28 for n in range(1, 8)]


@pytest.mark.parametrize("S", _KEYS)
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("kernel", ["w4", "w8"])
def test_key_counts_walk_every_path_of_the_loop_vs_fp64(kernel, mode, S, _hooks):
    """FR = 0: 1 .. 7 key tiles, full and with a ragged last tile of 36 keys."""
    _hooks(kernel)
    info = _plan(kernel, S)
    assert info[3] == 1                                         # fewer than 16 tiles: the small grid does not split its keys
    q, k, v = _qkv(kernel, mode)
    k, v = k[:S], v[:S]
    scale = ops.attn_scale(128)
    ctx, lse = ops.attention(q, k, v, H, want_lse=True, scale=scale)
    again, lse_again = ops.attention(q, k, v, H, want_lse=True, scale=scale)
    assert torch.equal(again, ctx) and torch.equal(lse_again, lse)
    ref_ctx, ref_lse2, _ = L._ref64(q, k, v, H, 128, scale)
    _gate(f"{kernel} S{S} ({-(-S // 64)} tiles)", ctx, lse, ref_ctx, ref_lse2, mode)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("kernel", ["w4", "w8"])
def test_pieces_of_odd_and_even_tile_counts_vs_fp64(kernel, mode, _hooks):
    """34 key tiles cut 4-way: pieces of 8, 9, 8 and 9 tiles (the last ragged) - three and four steady pairs in front of a tail
    of 2 and of 3, in segments that follow a whole unit in the same workgroup."""
    case = next(c for c in T.STREAMK_CASES if c[0] == kernel and c[2] == T.S_NARROW and [lv[0] for lv in c[6]] == [2])
    _, R, S, heads, G, full, levels = case
    nt = -(-S // 64)
    assert nt == 34 and sorted({((p + 1) * nt >> 2) - (p * nt >> 2) for p in range(4)}) == [8, 9]
    _hooks(kernel)
    q, k, v, scale, (ref_ctx, ref_lse2, _), _ = L._operands(kernel, R, S, heads, mode)
    ctx, lse = ops.attention(q, k, v, heads, want_lse=True, scale=scale)
    again, lse_again = ops.attention(q, k, v, heads, want_lse=True, scale=scale)
    assert torch.equal(again, ctx) and torch.equal(lse_again, lse)
    g, lerr, ok = attention_gate(ctx, lse, ref_ctx, ref_lse2, heads, mode)
    print(f"\n[{T.case_id(case)} {mode}] {g}; worst lse2 error {lerr:.2e}")
    assert ok, (str(g), lerr)


_FRAME_FORMS = [pytest.param("w4", 1, id="w4-FR1"), pytest.param("w8", 0, id="w8-FR1"), pytest.param("w8", 1, id="w8-FR3")]


@pytest.mark.parametrize("F", [1, 2, 3, 5])
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("kernel,lds", _FRAME_FORMS)
def test_frame_score_variants_walk_the_loop_vs_fp64(kernel, lds, mode, F, _hooks):
    """FR = 1 (4 and 8 waves) and FR = 3 (8 waves, entries in LDS): F frames of 196 keys - 4, 7, 10 and 16 tiles, the last ragged,
    the flush of a frame's entry in the steady state and in the tail."""
    P = 196
    S = F * P
    _hooks(kernel, lds)
    info = _plan(kernel, S)
    q, k, v = _qkv(kernel, mode)
    k, v = k[:S], v[:S]
    R = ROWS[kernel]
    scale = ops.attn_scale(128)
    assert capi.lib().mavlm_attention_frames_ws_floats(R, S, H, P) > 0
    ctx, lse, scores = ops.attention_frames(q, k, v, H, P, want_lse=True, scale=scale)
    again = ops.attention_frames(q, k, v, H, P, want_lse=True, scale=scale)
    assert torch.equal(again[0], ctx) and torch.equal(again[1], lse) and torch.equal(again[2], scores)
    # the forward without scores on the same schedule (the small grid that would split its keys runs the plain grid here)
    plain, lse_p = ops.attention(q, k, v, H, want_lse=True, scale=scale, plain=info[3] > 1)
    assert torch.equal(ctx, plain) and torch.equal(lse, lse_p)
    ref_ctx, ref_lse2, col = L._ref64(q, k, v, H, 128, scale)
    _gate(f"frames {kernel} {'lds' if lds else 'workspace'} F{F}", ctx, lse, ref_ctx, ref_lse2, mode)
    err = rel_l2_t(scores, col.view(F, P).mean(1))
    print(f"frame scores vs float64 column sums: rel-L2 {err:.2e}; sum x P / (H R) = {float(scores.sum()) * P / (H * R):.6f}")
    assert err < TOL and abs(float(scores.sum()) * P - H * R) < 1e-3 * H * R
