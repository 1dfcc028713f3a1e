"""CPU (-m "not gpu") tests of clip row batches (videos of fewer than 32 frames, different frame counts in one step): the planner,
the binding of the new exports, the prefix sums of the variable-length column-sum scratch, the refusals that need no device, and
the workspace offsets, which must not move."""
import ctypes
import os
import re

import pytest
import torch

import memory_augmented_vlm_amd as pkg
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd.model import llava_arch as arch
from conftest import ROOT

NEW = ("mavlm_attention_batch_varlen", "mavlm_attention_colsum_batch_varlen", "mavlm_step_batch_frames",
       "mavlm_fuse_emit_layout_frames_to")


@pytest.fixture(scope="module")
def built_lib():
    return pkg.build_library()


def test_new_exports_are_declared_and_bound(built_lib):
    hdr = open(os.path.join(ROOT, "include", "mavlm.h")).read()
    l = ctypes.CDLL(built_lib)
    for name in NEW:
        assert name in capi.SIGNATURES and hasattr(l, name)
        assert re.search(r"\bint %s\(" % name, hdr)
    assert "mavlm_attention_colsum_batch_varlen_floats" in capi.SIGNATURES and hasattr(l, "mavlm_attention_colsum_batch_varlen_floats")
    assert re.search(r"\bint64_t mavlm_attention_colsum_batch_varlen_floats\(", hdr)
    assert re.search(r"#define MAVLM_ABI_VERSION 3\b", hdr) and capi.lib().mavlm_abi_version() == 3


# ---- the planner -----------------------------------------------------------------------------------------------------------------------
def test_planner_mixed_lengths():
    # 9 and 17 share a batch (2 * 9 >= 17); the 64-frame video and the 40-frame one are not clips
    clips, rest = arch.plan_clip_batches([9, 64, 17, 40])
    assert clips == [(2, [2, 0])] and rest == [1, 3]
    # equal lengths are eligible: input order among equals, the group takes the equal-F step
    assert arch.plan_clip_batches([5, 5, 5]) == ([(4, [0, 1, 2])], [])
    # 0 and 32 frames are not clips
    assert arch.plan_clip_batches([0, 32, 31, 31]) == ([(2, [2, 3])], [0, 1])


def test_planner_half_length_rule():
    # 31, 27, 23, 19, 16 stay with the 31 (2 * 16 >= 31); 12 opens the next group (bound 6), which takes 9; 5 is left alone
    clips, rest = arch.plan_clip_batches([31, 27, 23, 19, 16, 12, 9, 5])
    assert clips == [(8, [0, 1, 2, 3, 4]), (2, [5, 6])] and rest == [7]
    # a lopsided pair never shares a batch
    assert arch.plan_clip_batches([4, 20]) == ([], [0, 1])
    # longest first, whatever the input order; the groups in the order of their first video
    clips, rest = arch.plan_clip_batches([3, 20, 5, 11, 4])
    assert clips == [(4, [2, 4, 0]), (2, [1, 3])] and rest == []


@pytest.mark.parametrize("k, size", [(2, 2), (3, 4), (4, 4), (5, 8), (6, 8), (7, 8), (8, 8)])
def test_planner_engine_sizes(k, size):
    clips, rest = arch.plan_clip_batches(list(range(31, 31 - k, -1)))
    assert clips == [(size, list(range(k)))] and rest == []


def test_planner_groups_of_at_most_eight_keys_and_errors():
    clips, rest = arch.plan_clip_batches([20] * 11)
    assert clips == [(8, list(range(8))), (4, [8, 9, 10])] and rest == []
    clips, rest = arch.plan_clip_batches([20] * 9)
    assert clips == [(8, list(range(8)))] and rest == [8]
    # another dtype / device never shares a batch
    assert arch.plan_clip_batches([9, 10], ["a", "b"]) == ([], [0, 1])
    assert arch.plan_clip_batches([]) == ([], []) and arch.plan_clip_batches([7]) == ([], [0])
    with pytest.raises(ValueError):
        arch.plan_clip_batches([9, 9], sizes=(1,))
    with pytest.raises(ValueError):
        arch.plan_clip_batches([9, 9], keys=[None])


def test_switch_is_off_by_default_and_inference_only(monkeypatch):
    assert arch.LlavaMetaForCausalLM._clip_row_batches is False

    class M(arch.LlavaMetaForCausalLM):
        pass

    m = M()
    m.enable_clip_row_batches()
    assert m._clip_row_batches is True and arch.LlavaMetaForCausalLM._clip_row_batches is False
    m.enable_clip_row_batches(False)
    assert m._clip_row_batches is False
    calls = []

    class Stop(Exception):
        pass

    def spy(name, real):
        def f(*a, **k):
            calls.append(name)
            real(*a, **k)
            raise Stop
        return f

    monkeypatch.setattr(arch, "plan_row_batches", spy("equal", arch.plan_row_batches))
    monkeypatch.setattr(arch, "plan_clip_batches", spy("clips", arch.plan_clip_batches))

    class Model:
        recurrent_memory_transformer = None

    vids = [(torch.zeros(9, 196, 8), None), (torch.zeros(17, 196, 8), None)]
    for kw, want in (({}, "equal"), ({"clips": False}, "equal"), ({"clips": True}, "clips"), ({"clips": True, "train": True}, "equal")):
        del calls[:]
        with pytest.raises(Stop):
            arch.run_video_groups(Model(), vids, None, None, None, **kw)
        assert calls[0] == want


# ---- host arithmetic and refusals ---------------------------------------------------------------------------------------------------------
def _S(*v):
    return (capi.i32 * len(v))(*v)


def _off(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_varlen_colsum_floats_are_prefix_sums(built_lib):
    lib = capi.lib()
    R, H = 1568, 8
    S = [980, 6076, 196, 3920]
    per = [int(lib.mavlm_attention_colsum_floats(R, s, H)) for s in S]
    assert all(p >= H * s for p, s in zip(per, S))
    for nb in range(1, 5):
        assert int(lib.mavlm_attention_colsum_batch_varlen_floats(R, _S(*S[:nb]), H, nb)) == sum(per[:nb])
    assert lib.mavlm_attention_colsum_batch_varlen_floats(R, _S(980, 0), H, 2) == 0
    assert lib.mavlm_attention_colsum_batch_varlen_floats(R, _S(*([196] * 17)), H, 17) == 0
    assert lib.mavlm_attention_colsum_batch_varlen_floats(R, None, H, 2) == 0
    assert lib.mavlm_attention_colsum_batch_varlen_floats(0, _S(980), H, 1) == 0


def test_varlen_operator_refusals_without_a_device(built_lib):
    lib = capi.lib()
    P, ld, R = 4096, 256, 196

    def fwd(S, off, nb, H=None, hd=128, ldk=ld):
        return lib.mavlm_attention_batch_varlen(P, ld, P, ldk, P, ld, P, ld, None, R, _S(*S), _off(*off), 2 * nb if H is None else H, 0.1,
                                                nb, hd, capi.BF16, None)

    S17, off17 = [64] * 17, [64 * ld * b for b in range(17)]
    assert fwd(S17, off17, 17) == capi.E_ARG                                  # more videos than the by-value arrays hold
    assert fwd([64], [0], 0) == capi.E_ARG
    assert fwd([64, 64], [0, 64 * ld], 2, H=3) == capi.E_ARG                  # H % nb
    assert fwd([64, 0], [0, 64 * ld], 2) == capi.E_ARG                        # S[b] < 1
    assert fwd([64, 64], [0, 63 * ld], 2) == capi.E_ARG                       # video 1 starts inside video 0's keys
    assert fwd([40, 64, 980], [0, 40 * ld, 103 * ld], 3) == capi.E_ARG        # video 2 starts on video 1's last row
    assert fwd([64, 64], [0, 64 * ld + 4], 2) == capi.E_ARG                   # alignment
    assert fwd([64, 64], [0, -8], 2) == capi.E_ARG
    assert fwd([64, 64], [0, 64 * ld], 2, ldk=ld + 4) == capi.E_ARG           # stride alignment
    assert fwd([64, 64], [0, 64 * ld], 2, hd=448) == capi.E_SHAPE
    assert fwd([64, 64], [0, 64 * ld], 2, hd=256) == capi.E_SHAPE

    def cs(S, off, nb, floats, hd=128):
        return lib.mavlm_attention_colsum_batch_varlen(P, ld, P, ld, _off(*off), P, P, floats, R, _S(*S), 2, nb, hd, 0.1, capi.BF16, None)

    need = int(lib.mavlm_attention_colsum_batch_varlen_floats(R, _S(64, 980), 2, 2))
    assert cs(S17, off17, 17, 1 << 40) == capi.E_ARG
    assert cs([64, 980], [0, 63 * ld], 2, need) == capi.E_ARG                 # overlapping key ranges
    assert cs([64, 980], [0, 64 * ld], 2, need - 1) == capi.E_ARG             # too small a `part`
    assert cs([64, 0], [0, 64 * ld], 2, need) == capi.E_ARG
    assert cs([64, 980], [0, 64 * ld], 2, need, hd=448) == capi.E_SHAPE


def cfg(batch, frames=4):
    return capi.Config(hidden=256, heads=2, patches=196, mem_tokens=2, depth=2, inter=1024, cache_cap=2, max_chunk_frames=frames,
                       dtype=0, eps=1e-12, batch=batch)


def test_step_frames_refusals_without_a_device(built_lib):
    lib = capi.lib()
    h = capi.vp()
    assert lib.mavlm_create(cfg(4), h) == 0
    segs = (capi.vp * 4)(256, 256, 256, 256)

    def step(F, n, ctx=h, scores=None, ld=0):
        return lib.mavlm_step_batch_frames(ctx, segs, _S(*F), n, scores, ld, 0, None)

    assert step([4, 2, 0], 3) == capi.E_ARG                                   # F[b] = 0
    assert step([4, 5, 1], 3) == capi.E_ARG                                   # above max_chunk_frames
    assert step([4, 2, 1], 0) == capi.E_ARG and step([4, 2, 1, 1, 1], 5) == capi.E_ARG
    assert step([4, 2, 1], 3, scores=4096, ld=3) == capi.E_ARG                # a score row shorter than the longest clip
    assert lib.mavlm_step_batch_frames(h, segs, None, 3, None, 0, 0, None) == capi.E_ARG
    assert step([4, 2, 1], 3) == capi.E_STATE                                 # nothing bound yet
    assert step([2, 2, 2], 3) == capi.E_STATE                                 # (equal F: the existing step, same answer)
    assert lib.mavlm_steps(h) == 0
    lib.mavlm_destroy(h)
    h1 = capi.vp()
    assert lib.mavlm_create(cfg(0), h1) == 0                                  # a single-video context
    assert step([4], 1, ctx=h1) == capi.E_STATE
    lib.mavlm_destroy(h1)


def test_frames_emit_refusals_without_a_device(built_lib):
    lib = capi.lib()
    h = capi.vp()
    assert lib.mavlm_create(cfg(4), h) == 0
    rows = (ctypes.c_int64 * 4)()
    xs = (capi.vp * 4)(256, 256, 256, 256)

    def emit(n, nf, dst, out_rows, ctx=h, fine_ld=4):
        return lib.mavlm_fuse_emit_layout_frames_to(ctx, n, xs, 512, fine_ld, _S(*nf), 1024, 3, 2048, 2, None, 1, capi.LAYOUT_NONE, 4096,
                                                    out_rows, _off(*dst), rows, None)

    # no video has stepped: a block is [3 prompt rows ; 2 prompt rows ; its fine frames]
    a, b = 5 + 4 * 196, 5 + 1 * 196
    assert emit(2, [4, 1], [0, a], a + b) == capi.E_STATE                     # destinations fine by each block's OWN length: state
    assert emit(2, [4, 1], [0, a - 1], a + b) == capi.E_ARG                   # the long block runs into the short one
    assert emit(2, [4, 1], [b, 0], a + b) == capi.E_STATE                     # the short block first: fits
    assert emit(2, [4, 1], [b - 1, 0], a + b) == capi.E_ARG
    assert emit(2, [4, 1], [0, a + 1], a + b) == capi.E_ARG                   # past `out_rows`
    assert emit(2, [5, 1], [0, a + 196], 2 * a + 400) == capi.E_ARG           # more fine frames than an index row holds
    assert emit(2, [4, -1], [0, a], a + b) == capi.E_ARG
    assert list(rows) == [0] * 4
    lib.mavlm_destroy(h)
    h1 = capi.vp()
    assert lib.mavlm_create(cfg(1), h1) == 0
    assert emit(1, [4], [0], a, ctx=h1) == capi.E_STATE                       # a single-video context
    lib.mavlm_destroy(h1)
    h2 = capi.vp()                                                            # hidden 896: no multiple of the 256-column tiles' width
    assert lib.mavlm_create(capi.Config(hidden=896, heads=2, patches=196, mem_tokens=2, depth=2, inter=3584, cache_cap=2,
                                        max_chunk_frames=4, dtype=0, eps=1e-12, batch=2), h2) == 0
    assert emit(2, [4, 1], [0, a], a + b, ctx=h2) == capi.E_SHAPE
    lib.mavlm_destroy(h2)


# ---- the workspace ---------------------------------------------------------------------------------------------------------------------------
# mavlm_workspace_layout of the commit before clip row batches (read from a build of it): the 14 reported values per config
LAYOUT_CONFIGS = {
    "d256_b4": cfg(4),
    "d256_b8_f32": cfg(8, 32),
    "d1024_single": capi.Config(hidden=1024, heads=8, patches=196, mem_tokens=8, depth=2, inter=4096, cache_cap=10, max_chunk_frames=32,
                                dtype=0, eps=1e-12, batch=0),
    "d1024_b8": capi.Config(hidden=1024, heads=8, patches=196, mem_tokens=8, depth=2, inter=4096, cache_cap=10, max_chunk_frames=32,
                            dtype=0, eps=1e-12, batch=8),
    "d896_b4": capi.Config(hidden=896, heads=2, patches=196, mem_tokens=8, depth=2, inter=3584, cache_cap=10, max_chunk_frames=32,
                           dtype=0, eps=1e-12, batch=4),
    "d3584_b2": capi.Config(hidden=3584, heads=8, patches=196, mem_tokens=1, depth=2, inter=14336, cache_cap=10, max_chunk_frames=32,
                            dtype=0, eps=1e-12, batch=2),
}
PARENT_LAYOUT = {
    "d256_b4": [0, 6422528, 7225344, 8028160, 8830976, 15253504, 16859136, 17661952, 18464768, 18477312, 31466752, 3211264, 0, 0],
    "d256_b8_f32": [0, 102760448, 104366080, 105971712, 107577344, 120422400, 123633664, 125239296, 126844928, 126870016, 153112064,
                    6422528, 0, 0],
    "d1024_single": [0, 102760448, 105971712, 109182976, 112394240, 240844800, 247267328, 250478592, 253689856, 253740032, 280571648,
                     25690112, 0, 0],
    "d1024_b8": [0, 411041792, 436731904, 462422016, 488112128, 693633024, 745013248, 770703360, 796393472, 796794880, 865368832, 0, 0,
                 0],
    "d896_b4": [0, 179830784, 191070208, 202309632, 213549056, 438337536, 460816384, 472055808, 483295232, 483345408, 483395584, 0, 0, 0],
    "d3584_b2": [0, 359661568, 362471424, 365281280, 368091136, 480485376, 486105088, 488914944, 491724800, 491737344, 491938048,
                 22478848, 0, 0],
}
# ... and the totals of the contexts that gain no region: a single video, the wide heads
PARENT_TOTAL = {"d1024_single": 328998656, "d896_b4": 531214336, "d3584_b2": 522160384}


@pytest.mark.parametrize("name", sorted(PARENT_LAYOUT))
def test_workspace_offsets_did_not_move(built_lib, name):
    lib = capi.lib()
    c = LAYOUT_CONFIGS[name]
    off = (ctypes.c_size_t * 14)()
    assert lib.mavlm_workspace_layout(c, off, 14) == 0
    assert list(off) == PARENT_LAYOUT[name]
    # the scratch of the variable-length column sums lies behind every reported region
    assert lib.mavlm_workspace_bytes(c) >= max(off[:11]) + off[11]
    if name in PARENT_TOTAL:
        assert lib.mavlm_workspace_bytes(c) == PARENT_TOTAL[name]
