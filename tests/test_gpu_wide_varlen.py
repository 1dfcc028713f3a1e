"""-m gpu: the variable-length forward for heads of 448 columns (`mavlm_attention_hd_batch_varlen`: one plain-grid launch of the
32-query-wave kernel over (video, head, 128-query block)) and its switch in the clip step (`mavlm_set_attention_hd_varlen`, off by
default).

Yardsticks: `mavlm_attention_hd` without a workspace (the plain grid) on each video's own, separately allocated operands - bit
for bit -, float64 through `gpu_util.attention_gate`, the step with the switch off - bit for bit -, the single-video engine under
the row-batch gates of tests/test_gpu_ragged_batch.py, and the pinned launch census (tests/launch_census.json, read here, never
copied)."""
import ctypes
import json

import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
from oracle import memory_path as O
from gpu_util import attention_gate, to_dev, to_np
from test_gpu_launch_census import CHUNK, FIXTURE, _Case, _census
from test_gpu_path import make_projector
from test_gpu_ragged_batch import ROW_BATCH_ROWS, ROW_BATCH_SCORES
from test_gpu_streamk_levels import _randn, _ref64

pytestmark = pytest.mark.gpu
P, HD = 196, 448


@pytest.fixture(autouse=True)
def _inference_path():
    with torch.no_grad():
        yield


class _hooks:
    """the process-wide switches of this file, put back on the way out"""

    def __init__(self, varlen, wide_groups=0):
        self.varlen, self.wide_groups = varlen, wide_groups

    def __enter__(self):
        lib = capi.lib()
        capi.check(lib.mavlm_set_attention_wide_groups(self.wide_groups), "mavlm_set_attention_wide_groups")
        capi.check(lib.mavlm_set_attention_hd_varlen(1 if self.varlen else 0), "mavlm_set_attention_hd_varlen")

    def __exit__(self, *exc):
        lib = capi.lib()
        lib.mavlm_set_attention_hd_varlen(0)
        lib.mavlm_set_attention_wide_groups(0)


# ---- 1. the operator, bit for bit ---------------------------------------------------------------------------------------------------------
def _varlen_forward(q, k, v, S, offs, Hv, R, scale, lse=True):
    nb = len(S)
    out = torch.full((nb * R, Hv * HD), float("nan"), device="cuda", dtype=q.dtype)
    l2 = torch.full((nb * Hv, R), float("nan"), device="cuda", dtype=torch.float32)
    capi.check(capi.lib().mavlm_attention_hd_batch_varlen(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                                          out.data_ptr(), out.stride(0), l2.data_ptr() if lse else None, R,
                                                          (capi.i32 * nb)(*S), (ctypes.c_int64 * nb)(*offs), nb * Hv, scale, nb, HD,
                                                          ops.dtype_code(q.dtype), ops.stream_ptr()), "mavlm_attention_hd_batch_varlen")
    torch.cuda.synchronize()
    return out, l2


def _single_plain(qb, kb, vb, Hv, scale):
    """mavlm_attention_hd without a workspace: the plain grid of one video"""
    R, S = qb.shape[0], kb.shape[0]
    out = torch.full((R, Hv * HD), float("nan"), device="cuda", dtype=qb.dtype)
    l2 = torch.full((Hv, R), float("nan"), device="cuda", dtype=torch.float32)
    capi.check(capi.lib().mavlm_attention_hd(qb.data_ptr(), qb.stride(0), kb.data_ptr(), kb.stride(0), vb.data_ptr(), vb.stride(0),
                                             out.data_ptr(), out.stride(0), l2.data_ptr(), R, S, Hv, HD, scale, ops.dtype_code(qb.dtype),
                                             ops.stream_ptr()), "mavlm_attention_hd")
    torch.cuda.synchronize()
    return out, l2


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("S", [(20, 32, 980), (64, 96)], ids=["lt1-1-30.6tiles", "2-3tiles"])
def test_wide_varlen_forward_equals_the_plain_grid_per_video(S, mode):
    """2 heads of 448 per video, R = 196 (two query blocks, the second ragged).  Key counts: less than one 32-key tile, exactly
    one, 30 tiles + 20 keys; and 2 and 3 tiles (the prologue in which K runs a tile ahead of V).  K / V are packed back to back: a
    load past a video's last key would read its neighbour's rows (row 0 of every video is scaled up, so such a key cannot go
    unnoticed)."""
    Hv, R, W = 2, 196, 2 * HD
    nb, tot = len(S), sum(S)
    q = _randn((nb * R, W), 9900, mode)
    q[3] *= 8.0                                            # (the deferred rescale fires inside the tile loop)
    k, v = _randn((tot, W), 9901, mode), _randn((tot, W), 9902, mode)
    starts = [sum(S[:b]) for b in range(nb)]
    for s0 in starts:
        k[s0] *= 6.0
        v[s0] *= 50.0
    scale = ops.attn_scale(HD)
    offs = [s0 * W for s0 in starts]
    out, l2 = _varlen_forward(q, k, v, list(S), offs, Hv, R, scale)
    again, l2_again = _varlen_forward(q, k, v, list(S), offs, Hv, R, scale)
    assert torch.equal(out, again) and torch.equal(l2, l2_again)
    assert torch.isfinite(out.float()).all() and torch.isfinite(l2).all()
    for b in range(nb):
        qb = q[b * R:(b + 1) * R].clone()                                                          # separately allocated copies
        kb, vb = k[starts[b]:starts[b] + S[b]].clone(), v[starts[b]:starts[b] + S[b]].clone()
        want, want_l2 = _single_plain(qb, kb, vb, Hv, scale)
        assert torch.equal(out[b * R:(b + 1) * R], want), f"video {b} (S = {S[b]}): O differs from mavlm_attention_hd"
        assert torch.equal(l2[b * Hv:(b + 1) * Hv], want_l2), f"video {b} (S = {S[b]}): lse2 differs from mavlm_attention_hd"
        ref_ctx, ref_lse2, _ = _ref64(qb, kb, vb, Hv, HD, scale)
        g, lerr, ok = attention_gate(out[b * R:(b + 1) * R], l2[b * Hv:(b + 1) * Hv], ref_ctx, ref_lse2, Hv, mode)
        print(f"\n[wide varlen {mode} video {b} S={S[b]}] {g}; worst lse2 error {lerr:.2e}")
        assert ok, (b, str(g), lerr)
    # without lse2: the same O
    out2, _ = _varlen_forward(q, k, v, list(S), offs, Hv, R, scale, lse=False)
    assert torch.equal(out2, out)
    # the wrapper: the same launch
    out3, l3 = ops.attention_hd_batch_varlen(q, k, v, Hv, S, want_lse=True, scale=scale)
    torch.cuda.synchronize()
    assert torch.equal(out3, out) and torch.equal(l3, l2)


# ---- 2. the step --------------------------------------------------------------------------------------------------------------------------
def _projector(hidden, heads, mem, seed):
    cfg = O.PathConfig(hidden=hidden, heads=heads, mem_tokens=mem, depth=2)
    return make_projector(cfg, O.make_weights(cfg, seed=seed))


def _segs(frames, D, seed, alt=None):
    xs = [O.bf16_round(O.hash_normal_like((f, P, D), seed + b)) for b, f in enumerate(frames)]
    if alt is not None:
        xs[alt] = O.bf16_round(O.hash_normal_like(xs[alt].shape, seed + 900))
    return [to_dev(x) for x in xs]


def _run_steps(proj, engine, steps, on, wide_groups=0):
    """a fresh engine stepping `steps` (a list of lists of clips): per step the newest memory and the frame scores of every video"""
    bp = BatchedProjector(proj, engine)
    res = []
    with _hooks(on, wide_groups):
        bp.reset()
        for segs in steps:
            views = bp.step_frames(segs)
            torch.cuda.synchronize()
            res.append(([bp.memory_cache(b)[-1].clone() for b in range(len(segs))], [s.clone() for s in views]))
    return res, bp


def _check_against_single_engine(proj, steps, bp, res, heads, mem, what):
    for b in range(len(steps[0])):
        chunks = [segs[b] for segs in steps if b < len(segs)]
        proj.memory_cache = []
        want_scores = []
        for c in chunks:
            cache, scores = proj(c)
            torch.cuda.synchronize()
            want_scores.append(scores[-1].clone())
        mine = bp.memory_cache(b)
        assert len(mine) == len(cache) == len(chunks)
        err = O.rel_l2(to_np(torch.cat(list(mine))), to_np(torch.cat(list(cache))))
        serr = max(O.rel_l2(to_np(res[t][1][b]), to_np(w)) for t, w in enumerate(want_scores))
        print(f"{what}, video {b} ({[c.shape[0] for c in chunks]} frames): memories vs single-video engine {err:.2e}, frame scores {serr:.2e}")
        assert err < ROW_BATCH_ROWS and serr < ROW_BATCH_SCORES
        for t, c in enumerate(chunks):
            assert tuple(res[t][1][b].shape) == (c.shape[0],)
            assert abs(float(res[t][1][b].float().sum()) - heads * mem) < 2e-2 * heads * mem      # sum_f score_f = H * M


def test_step_with_the_switch_on_equals_the_per_video_launches():
    """hidden 896 = 2 heads of 448, M = 2, depth 2 (the census shape); clips of 3, 2 and 1 frames on an engine of 4, then a second
    step of 1 and 3 frames (the prefix shrinks)."""
    proj = _projector(896, 2, 2, 78)
    steps = [_segs((3, 2, 1), 896, 9910), _segs((1, 3), 896, 9920)]
    off, _ = _run_steps(proj, 4, steps, on=False)
    on, bp = _run_steps(proj, 4, steps, on=True)
    for t, segs in enumerate(steps):
        for b in range(len(segs)):
            assert torch.isfinite(on[t][0][b].float()).all()
            assert torch.equal(on[t][0][b], off[t][0][b]), f"step {t} video {b}: memory differs from the per-video launches"
            assert torch.equal(on[t][1][b], off[t][1][b]), f"step {t} video {b}: frame scores differ from the per-video launches"
    assert not torch.equal(on[0][0][0], on[0][0][1])
    _check_against_single_engine(proj, steps, bp, on, 2, 2, "hidden 896")
    # a video's result does not depend on its neighbours' content
    alt, _ = _run_steps(proj, 4, [_segs((3, 2, 1), 896, 9910, alt=1)], on=True)
    assert not torch.equal(alt[0][0][1], on[0][0][1])
    for b in (0, 2):
        assert torch.equal(alt[0][0][b], on[0][0][b]), f"video {b}: memory moved with another clip's frames"
        assert torch.equal(alt[0][1][b], on[0][1][b]), f"video {b}: frame scores moved with another clip's frames"


# ---- 3. / 4. the census ---------------------------------------------------------------------------------------------------------------------
def _census_scenario(on, wide_groups=0):
    """`i_hidden_896 / heads2_step_frames` of tests/test_gpu_launch_census.py: the same model construction, the single video first,
    frames (3, 2) on an engine of 2"""
    c = _Case(hidden=896, heads=2)
    vid, idx = c.video(2 * CHUNK, 190)
    c.single(vid, idx, "frame")
    bp = BatchedProjector(c.rm, 2)
    segs = [c.video(f, 195 + f)[0] for f in (3, 2)]

    def frames_step():
        bp.reset()
        bp.step_frames(segs)

    with _hooks(on, wide_groups):
        got = _census(frames_step)
    return got, [bp.memory_cache(b)[-1].clone() for b in range(2)]


def _fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)["i_hidden_896"]["heads2_step_frames"]


def test_census_with_the_switch_on_and_off():
    want = _fixture()
    assert want["attention_fwd"][0] == 4                         # (depth 2 x 2 videos: what the switch replaces)
    got, mem_on = _census_scenario(True)
    print("switch on:", json.dumps(got, sort_keys=True))
    assert got["attention_fwd"] == [2] + want["attention_fwd"][1:], "one launch per formation layer, the flops and bytes of the four"
    for kind in sorted(set(want) | set(got)):
        if kind != "attention_fwd":
            assert got.get(kind) == want.get(kind), f"{kind}: launches, flops or bytes differ from the recorded census"
    back, mem_off = _census_scenario(False)
    assert back == want, "with the switch off the census is the recorded one"
    assert all(torch.equal(a, b) for a, b in zip(mem_on, mem_off))


def test_fallback_to_the_per_video_launches_under_16_query_waves():
    """switch on, `mavlm_set_attention_wide_groups(1)`: the 16-query-wave kernel has no variable-length form - the per-video loop"""
    want = _fixture()
    got, mem = _census_scenario(True, wide_groups=1)
    print("switch on, 16-query waves:", json.dumps(got, sort_keys=True))
    assert got["attention_fwd"] == want["attention_fwd"] and got["attention_fwd"][0] == 4
    assert got == want
    assert all(torch.isfinite(m.float()).all() for m in mem)
    ref, mem_ref = _census_scenario(False, wide_groups=1)
    assert ref == want and all(torch.equal(a, b) for a, b in zip(mem, mem_ref))


# ---- 5. the full width once -----------------------------------------------------------------------------------------------------------------
def test_clips_wide_heads_with_the_switch_on():
    """D = 3584 (8 heads of 448), M = 1, clips of 3 and 1 frames on an engine of 2 (the shape of test_gpu_clip_batch.py's
    test_clips_wide_heads), under its gates; and the bits of the per-video launches"""
    proj = _projector(3584, 8, 1, 77)
    steps = [[to_dev(O.bf16_round(O.hash_normal_like((f, P, 3584), 9800 + b))) for b, f in enumerate((3, 1))]]
    on, bp = _run_steps(proj, 2, steps, on=True)
    _check_against_single_engine(proj, steps, bp, on, 8, 1, "hidden 3584")
    off, _ = _run_steps(proj, 2, steps, on=False)
    for b in range(2):
        assert torch.equal(on[0][0][b], off[0][0][b]) and torch.equal(on[0][1][b], off[0][1][b])
