"""-m gpu: clip row batches under autograd at heads of 448 columns (hidden 3584 / 8 heads, the OneVision-7B width; the small shapes
here use hidden 896 = 2 heads of 448).  The variable-length 448 backward (`mavlm_attention_bwd_hd_batch_varlen`,
`ops.attention_bwd_hd_batch_varlen`: `attn_bwd_hd_kernel<..., VL>` in all four modes), the step
(`BatchedProjector.step_train_frames` behind `ops.set_attention_hd_varlen_train`, off by default) and the entry point
(`enable_clip_row_batches(True, training=True)` plus the switch).

Yardsticks: `ops.attention_bwd_hd` on separately allocated copies of each video's operands (bit for bit: every output element has
one owner, a workgroup of video b runs the single-video kernel's instruction stream on b's rows), oracle/backward.py at the gate of
the 448 operator test (tests/test_gpu_backward_ops.py, 1e-3), the inference clip step (bit for bit), oracle/torch_path.py float64
autograd summed over the clips, and the single-video training path (statistic and gates of tests/test_gpu_clip_train.py)."""
import functools

import numpy as np
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from memory_augmented_vlm_amd.model import llava_arch as arch
from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector, TransformerProjector
from oracle import memory_path as O
from oracle import backward as OB
from oracle import torch_path as TP
from gpu_util import DT, to_dev, to_np
from test_gpu_backward_ops import TOL as OP_TOL_448
from test_gpu_batch_train import GRAD_TOL
from test_gpu_clip_train import BIG, TAIL, _clips, _cots, _grad_errors, _grads, _i32, _i64, _loss
from test_gpu_ragged_batch import ROW_BATCH_ROWS, ROW_BATCH_SCORES
from test_gpu_ragged_train import CAP, _assert_no_unit_is_cut, _setup
from test_gpu_streamk_levels import _randn

pytestmark = pytest.mark.gpu
P, HD = 196, 448
FRAMES = (4, 2, 1)          # the clips of the step tests: 784, 392 and 196 keys
GAP = 3                     # sentinel rows between two videos' key gradients


@pytest.fixture(autouse=True)
def _switch_is_off_outside_a_test():
    assert ops.attention_hd_varlen_train() is False
    yield
    ops.set_attention_hd_varlen_train(False)


class _switch:
    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        ops.set_attention_hd_varlen_train(self.on)

    def __exit__(self, *exc):
        ops.set_attention_hd_varlen_train(False)


# ---- 1. the variable-length 448 backward operator, bit for bit ------------------------------------------------------------------------------
def _bwd_varlen(q, k, v, o, do, lse, S, Hv, R, scale, want=(True, True, True)):
    """the export itself, into sentinel-filled buffers: GAP sentinel rows between the videos' key gradients (dkv_off has gaps that
    kv_off has not) and a tail behind the last video.  Returns (dq, dk, dv, row starts of the videos in dk / dv)"""
    nb, tot, W = len(S), sum(S), Hv * HD
    dq = torch.full((nb * R + TAIL, W), -BIG, device="cuda", dtype=q.dtype)
    dk = torch.full((tot + GAP * nb + TAIL, W), -BIG, device="cuda", dtype=q.dtype)
    dv = torch.full((tot + GAP * nb + TAIL, W), -BIG, device="cuda", dtype=q.dtype)
    delta = torch.empty((nb * Hv, R), device="cuda", dtype=torch.float32)
    offs = [sum(S[:b]) * k.stride(0) for b in range(nb)]
    dstart = [sum(S[:b]) + GAP * b for b in range(nb)]
    p = lambda t, on: t.data_ptr() if on else None
    capi.check(capi.lib().mavlm_attention_bwd_hd_batch_varlen(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(),
                                                              v.stride(0), o.data_ptr(), o.stride(0), do.data_ptr(), do.stride(0),
                                                              lse.data_ptr(), delta.data_ptr(), p(dq, want[0]), W, p(dk, want[1]), W,
                                                              p(dv, want[2]), W, R, _i32(S), _i64(offs), _i64([d * W for d in dstart]),
                                                              nb * Hv, scale, nb, HD, ops.dtype_code(q.dtype), ops.stream_ptr()),
               "mavlm_attention_bwd_hd_batch_varlen")
    torch.cuda.synchronize()
    return dq, dk, dv, dstart


def _sentinels_intact(name, t, S, dstart, written=True):
    """every row of a key-gradient buffer that belongs to no video still holds the sentinel (all rows where nothing is written)"""
    own = torch.zeros(t.shape[0], dtype=torch.bool, device=t.device)
    if written:
        for s, d in zip(S, dstart):
            own[d:d + s] = True
    assert bool((t[~own] == -BIG).all()), f"{name}: a row between the videos or behind the last one was written"
    assert not written or bool((t[own] != -BIG).any())


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("S", [(20, 40, 980), (64, 128, 192)], ids=["lt1-1.25-30.6tiles", "2-4-6tiles"])
def test_wide_varlen_backward_equals_the_single_video_backward_per_video(S, mode):
    """2 heads of 448 per video, R = 196 (four 64-row dQ workgroups, the last holding 4 rows).  Key counts: 20 (less than one
    32-key tile of dQ; in dK / dV one running workgroup whose second 32-row group lies wholly past the end), 40 (a tile and a
    ragged one), 980 (30.6 tiles; 16 dK workgroups and 8 dV workgroups per head, of which the short videos leave all but the
    first); and 64 / 128 / 192 (whole tiles and whole workgroups: the tile that runs one ahead starts exactly at the next video's
    first key).  K / V are packed back to back: a load past a video's last key reads its neighbour's first (row 0 of every video is
    scaled up); a store past it lands in a sentinel row."""
    S = list(S)
    Hv, R, W = 2, 196, 2 * HD
    nb, tot = len(S), sum(S)
    q = _randn((nb * R, W), 9400, mode) * 0.5            # (the magnitudes of the 448 operator test, tests/test_gpu_backward_ops.py)
    do = _randn((nb * R, W), 9403, mode) * 0.5
    k, v = _randn((tot, W), 9401, mode) * 0.5, _randn((tot, W), 9402, mode)
    starts = [sum(S[:b]) for b in range(nb)]
    for s0 in starts:
        k[s0] *= 6.0
        v[s0] *= 50.0
    scale = ops.attn_scale(HD)
    o, lse = ops.attention_hd_batch_varlen(q, k, v, Hv, S, want_lse=True, scale=scale)

    dq, dk, dv, dstart = _bwd_varlen(q, k, v, o, do, lse, S, Hv, R, scale)
    dq2, dk2, dv2, _ = _bwd_varlen(q, k, v, o, do, lse, S, Hv, R, scale)
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2), "a second launch differs from the first"
    assert bool((dq[nb * R:] == -BIG).all()), "dQ: the tail behind the last video was written"
    _sentinels_intact("dK", dk, S, dstart)
    _sentinels_intact("dV", dv, S, dstart)
    # each single-output call runs that output's own kernel mode (dK alone: MODE 1, dV alone: MODE 2; together: the fused MODE 3)
    only = [_bwd_varlen(q, k, v, o, do, lse, S, Hv, R, scale, want=tuple(j == i for j in range(3))) for i in range(3)]
    for i, name in enumerate(("dQ", "dK", "dV")):
        for j in range(3):
            if j != i:
                assert bool((only[i][j] == -BIG).all()), f"{name}-only call wrote another gradient"
    assert torch.equal(only[0][0], dq)
    _sentinels_intact("dK-only", only[1][1], S, dstart)
    _sentinels_intact("dV-only", only[2][2], S, dstart)
    r = O.rounder(mode)
    for b in range(nb):
        sl, kl, gl = slice(b * R, (b + 1) * R), slice(starts[b], starts[b] + S[b]), slice(dstart[b], dstart[b] + S[b])
        qb, kb, vb, ob, dob, lb = (q[sl].clone(), k[kl].clone(), v[kl].clone(), o[sl].clone(), do[sl].clone(),
                                   lse[b * Hv:(b + 1) * Hv].clone())              # separately allocated copies
        wq, wk, wv = ops.attention_bwd_hd(qb, kb, vb, ob, dob, lb, Hv, HD, scale)
        _, wk1, _ = ops.attention_bwd_hd(qb, kb, vb, ob, dob, lb, Hv, HD, scale, False, True, False)
        _, _, wv1 = ops.attention_bwd_hd(qb, kb, vb, ob, dob, lb, Hv, HD, scale, False, False, True)
        torch.cuda.synchronize()
        assert torch.equal(dq[sl], wq), f"video {b} (S = {S[b]}): dQ differs from mavlm_attention_bwd_hd"
        assert torch.equal(dk[gl], wk), f"video {b} (S = {S[b]}): dK (fused) differs from mavlm_attention_bwd_hd"
        assert torch.equal(dv[gl], wv), f"video {b} (S = {S[b]}): dV (fused) differs from mavlm_attention_bwd_hd"
        assert torch.equal(only[1][1][gl], wk1), f"video {b} (S = {S[b]}): dK-only differs from the dK-only single-video call"
        assert torch.equal(only[2][2][gl], wv1), f"video {b} (S = {S[b]}): dV-only differs from the dV-only single-video call"
        rq, rk, rv = OB.attention_bwd(to_np(qb), to_np(kb), to_np(vb), to_np(ob), to_np(dob), to_np(lb), Hv, mode, scale_in_ds=False)
        errs = (O.rel_l2(to_np(dq[sl]), r(rq)), O.rel_l2(to_np(dk[gl]), r(rk)), O.rel_l2(to_np(dv[gl]), r(rv)))
        errs1 = (O.rel_l2(to_np(only[1][1][gl]), r(rk)), O.rel_l2(to_np(only[2][2][gl]), r(rv)))
        print(f"\n[wide varlen bwd {mode} video {b} S={S[b]}] dq / dk / dv rel-L2 vs oracle {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}; "
              f"dk-only / dv-only {errs1[0]:.2e} {errs1[1]:.2e}")
        assert max(errs + errs1) <= OP_TOL_448, (b, errs, errs1)
    # the wrapper: its own destinations, and caller-owned ones that are column views of one wider buffer (a strided dk / dv)
    gq, gk, gv = ops.attention_bwd_hd_batch_varlen(q, k, v, o, do, lse, Hv, S, scale=scale)
    torch.cuda.synchronize()
    assert torch.equal(gq, dq[:nb * R])
    for b in range(nb):
        assert torch.equal(gk[starts[b]:starts[b] + S[b]], dk[dstart[b]:dstart[b] + S[b]])
        assert torch.equal(gv[starts[b]:starts[b] + S[b]], dv[dstart[b]:dstart[b] + S[b]])
    dst = torch.full((tot + 3, 2 * W + 8), -BIG, device="cuda", dtype=DT[mode])
    gq, _, _ = ops.attention_bwd_hd_batch_varlen(q, k, v, o, do, lse, Hv, S, need_dq=False, scale=scale, dk_out=dst[:tot, :W],
                                                 dv_out=dst[:tot, W:2 * W])
    torch.cuda.synchronize()
    assert gq is None and torch.equal(dst[:tot, :W], gk) and torch.equal(dst[:tot, W:2 * W], gv)
    assert bool((dst[tot:] == -BIG).all()) and bool((dst[:, 2 * W:] == -BIG).all())


# ---- 2. the step: forward -------------------------------------------------------------------------------------------------------------------
def _wide(mode="bf16"):
    return _setup(mode, 896, 2, 2)            # hidden 896 = 2 heads of 448, M = 2, depth 2


def _single_schedule_cuts_no_unit(R, H, keys):
    """does the single-video forward run every (128-query unit, head) whole at these key counts?  The existing
    `_assert_no_unit_is_cut` decides (it asks the plan of the narrow kernels); at this width the single-video forward
    additionally splits the keys of a small grid (`mavlm_attention_hd_ws_floats` > 0), which cuts every unit"""
    try:
        _assert_no_unit_is_cut(R, H, keys)
    except AssertionError:
        return False
    return all(int(capi.lib().mavlm_attention_hd_ws_floats(R, S, H, HD)) == 0 for S in keys)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_step_forward_equals_clip_inference_and_single_video_training(mode):
    """clips of 4, 2 and 1 frames on an engine of 4, the switch on: memories and frame scores of `step_train_frames` equal
    `step_frames`'s bit for bit; against the single-video training forward bit for bit where its schedule cuts no unit, else under
    the row-batch gates"""
    st = _wide(mode)
    exact = _single_schedule_cuts_no_unit(2 * P, 2, tuple(f * P for f in FRAMES))
    _, xs = _clips(st, FRAMES, 9900)
    bp = BatchedProjector(st.rm, 4)
    with torch.no_grad():
        bp.reset()
        views = [v.clone() for v in bp.step_frames(xs)]
        ref = [bp.memory_cache(b)[-1].clone() for b in range(3)]
        padded = bp.frame_scores[-1].clone()
    bp.reset()
    with pytest.raises(capi.MavlmError, match="448"):          # the switch is off: today's refusal, before any launch
        bp.step_train_frames(xs)
    assert bp._mode is None
    with _switch():
        got = bp.step_train_frames(xs)
    torch.cuda.synchronize()
    assert bp._tragged is True and [bp.video_steps(b) for b in range(4)] == [1, 1, 1, 0]
    assert len(bp.frame_scores) == 1 and torch.equal(bp.frame_scores[-1], padded)
    rm = st.rm
    print(f"\n{mode}: the single video's schedule cuts no unit: {exact}")
    for b, f in enumerate(FRAMES):
        cache = bp.memory_cache(b)
        assert len(cache) == 1 and cache[0].requires_grad and tuple(cache[0].shape) == (2, P, st.D)
        assert torch.isfinite(cache[0].detach().float()).all()
        assert torch.equal(cache[0].detach(), ref[b]), f"clip {b}: memory differs from the inference clip step"
        assert tuple(got[b].shape) == (f,) and not got[b].requires_grad and torch.equal(got[b], views[b]), f"clip {b}: frame scores"
        rm.memory_cache = []
        n0 = len(rm.frame_attn_scores)
        single, scores = rm(xs[b])
        assert single[-1].requires_grad
        err = O.rel_l2(to_np(cache[0].detach()), to_np(single[-1].detach()))
        serr = O.rel_l2(to_np(got[b]), to_np(scores[n0]))
        print(f"{mode} clip {b} ({f} frames): memory vs single-video training forward {err:.2e}, frame scores {serr:.2e}")
        if exact:
            assert torch.equal(single[-1].detach(), ref[b]), f"clip {b}: differs from the single-video training forward"
            assert torch.equal(scores[n0], views[b])
        assert err <= ROW_BATCH_ROWS and serr <= ROW_BATCH_SCORES
    assert not torch.equal(ref[0], ref[1])
    rm.memory_cache = []
    bp.reset()


def test_equal_frame_counts_are_the_ragged_training_step():
    """clips of 3, 3 and 3 frames with the switch on: `step_train_frames` takes the launches of `step_train(ragged=True)` -
    memories, frame scores and, after one backward pass of the same scalar, every parameter gradient are equal bit for bit"""
    st = _wide()
    rm = st.rm
    _, xs = _clips(st, (3, 3, 3), 9950)
    cots = _cots(st, 3, 9960)
    bp = BatchedProjector(rm, 4)
    runs = []
    for frames_form in (True, False):
        rm.zero_grad(set_to_none=True)
        bp.reset()
        with _switch(frames_form):
            sc = bp.step_train_frames(xs) if frames_form else bp.step_train(xs, ragged=True)
        mems = [bp.memory_cache(b)[-1].detach().clone() for b in range(3)]
        padded = bp.frame_scores[-1].clone()
        if frames_form:
            assert isinstance(sc, list) and all(torch.equal(sc[b], padded[b]) for b in range(3))
        _loss(bp, cots, range(3)).backward()
        bp.reset()
        runs.append((mems, padded, _grads(rm)))
    rm.zero_grad(set_to_none=True)
    (ma, sa, ga), (mb, sb, gb) = runs
    assert all(torch.equal(x, y) for x, y in zip(ma, mb)) and torch.equal(sa, sb)
    assert not torch.equal(ma[0], ma[1])
    assert sorted(ga) == sorted(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), f"{k}: gradient differs from the ragged step's at equal frame counts"


# ---- 3. gradients -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_grads(mode, hidden, heads, M, frames, seed):
    """float64 autograd of oracle/torch_path.py: every clip is one chunk of all its frames; summed over the clips (once per grid)"""
    st = _setup(mode, hidden, heads, M)
    host, _ = _clips(st, frames, seed)
    cots = _cots_m(st, len(frames), M)
    p = TP.params_from(st.w)
    loss = 0.0
    for b in range(len(frames)):
        cache = TP.run_steps(p, st.cfg, [host[b]], cache_cap=CAP)
        loss = loss + (cache[-1] * torch.from_numpy(cots[b]).double()).sum()
    return float(loss.detach()), TP.grads(p, loss)


def _cots_m(st, n, M):
    return _cots(st, n, 9960) if M == 2 else [O.bf16_round(O.hash_normal_like((M, P, st.D), 9960 + 10 * b, 0.05)) for b in range(n)]


def _clip_batch_vs_single_passes(st, frames, engine, M, seed, name):
    """ONE backward pass over the clip batch (switch on) and len(frames) accumulated single-video passes (the parent's path: the
    yardstick) against float64.  Returns (worst rel-L2 of the clip batch, of the single-video passes)"""
    mode = st.mode
    ref_loss, ref = _oracle_grads(mode, st.D, st.cfg.heads, M, tuple(frames), seed)
    _, xs = _clips(st, frames, seed)
    cots = _cots_m(st, len(frames), M)
    rm = st.rm
    rm.zero_grad(set_to_none=True)
    single_loss = 0.0
    for b in range(len(frames)):
        rm.memory_cache = []
        cache, _ = rm(xs[b])
        l1 = (cache[-1].float() * torch.from_numpy(cots[b]).cuda()).sum()
        l1.backward()
        single_loss += float(l1.detach())
    rm.memory_cache = []
    single = {k: to_np(g) for k, g in _grads(rm).items()}
    rm.zero_grad(set_to_none=True)
    bp = BatchedProjector(rm, engine)
    bp.reset()
    with _switch():
        bp.step_train_frames(xs)
        loss = _loss(bp, cots, range(len(frames)))
        loss.backward()
    bp.reset()
    batch = {k: to_np(g) for k, g in _grads(rm).items()}
    assert sorted(batch) == sorted(single)
    rm.zero_grad(set_to_none=True)
    print(f"\n{name}: loss clip batch {float(loss.detach()):.5f} single-video {single_loss:.5f} float64 {ref_loss:.5f}")
    assert abs(float(loss.detach()) - single_loss) <= 1e-3 * abs(single_loss) + 1e-3
    worst, worst_single, fails = _grad_errors(name, batch, ref, single)
    print(f"{name}: worst-parameter rel-L2 vs float64: clip batch {worst:.3e}, {len(frames)} single-video passes {worst_single:.3e}")
    assert not fails, fails
    assert worst <= 1.5 * worst_single, (worst, worst_single)
    return worst, worst_single


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_clip_gradients_vs_float64_oracle_and_single_video_path(mode):
    """loss = sum over the clips of <memory, cotangent>, hidden 896 / 2 heads of 448, clips of 4, 2 and 1 frames: the variable-length
    448 backward in every formation layer.  Relative gate: 1.5 x the single-video passes' error (the factor of
    tests/test_gpu_clip_train.py); absolute gate GRAD_TOL[mode] where the single-video passes meet it at this shape.
    Measured (MI355X): see DESIGN.md section 9."""
    worst, worst_single = _clip_batch_vs_single_passes(_wide(mode), FRAMES, 4, 2, 9900, f"wide {mode}")
    if worst_single <= GRAD_TOL[mode]:
        assert worst <= GRAD_TOL[mode], (worst, GRAD_TOL[mode])
    else:
        print(f"wide {mode}: the single-video passes miss GRAD_TOL ({worst_single:.3e} > {GRAD_TOL[mode]}): no absolute gate at this shape")


# ---- 4. nothing leaks between clips -------------------------------------------------------------------------------------------------------------
def test_no_leak_between_clips():
    """the 2-frame clip (the middle of the packed keys) holds other frames with rows of 1e4: the other clips' memories and frame
    scores stay bit for bit, and so do the gradients of a loss over THEIR memories"""
    st = _wide()
    cots = _cots(st, 3, 9960)
    rm = st.rm
    runs = []
    for alt in (None, 1):
        _, xs = _clips(st, FRAMES, 9900, alt=alt)
        bp = BatchedProjector(rm, 4)
        rm.zero_grad(set_to_none=True)
        bp.reset()
        with _switch():
            scores = [s.clone() for s in bp.step_train_frames(xs)]
            mems = [bp.memory_cache(b)[-1].detach().clone() for b in range(3)]
            _loss(bp, cots, (0, 2)).backward()
        bp.reset()
        runs.append((mems, scores, _grads(rm)))
    rm.zero_grad(set_to_none=True)
    (ma, sa, ga), (mb, sb, gb) = runs
    assert not torch.equal(ma[1], mb[1]) and torch.isfinite(mb[1].float()).all()
    for v in (0, 2):
        assert torch.equal(ma[v], mb[v]), f"clip {v}: memory moved with another clip's frames"
        assert torch.equal(sa[v], sb[v]), f"clip {v}: frame scores moved with another clip's frames"
    assert sorted(ga) == sorted(gb)
    for k in ga:
        assert torch.isfinite(gb[k].float()).all() and (k.endswith("k_proj.bias") or ga[k].float().abs().sum() > 0), k
        assert torch.equal(ga[k], gb[k]), f"{k}: the gradient of the other clips' loss moved with another clip's frames"


# ---- 5. the entry point ---------------------------------------------------------------------------------------------------------------------------
FRAMES7 = [9, 17, 12, 64]                     # three clips: one group on the engine of 4; the 64-frame video runs alone


def test_entry_point_clip_training_group_at_448(monkeypatch):
    """hidden 896 / 2 heads of 448 behind `prepare_inputs_labels_for_multimodal`: with `enable_clip_row_batches(True, training=True)`
    the switch decides whether the three clips take one `step_train_frames`; `inputs_embeds` against the switch-off result under
    the entry-point gate of tests/test_gpu_clip_train.py (6e-3)"""
    import test_gpu_video_batch as vb
    monkeypatch.setattr(vb, "CFG", O.PathConfig(hidden=896, heads=8, mem_tokens=2, depth=2))
    lm, model, hf, _, _ = vb._host()
    old = model.recurrent_memory_transformer                    # LlavaMetaModel builds 8 heads: the same weights as 2 heads of 448
    c = old.config
    c.mm_num_attention_heads = 2
    rm = TransformerProjector(c)
    rm.load_state_dict(old.state_dict())
    rm = rm.to("cuda").to(torch.bfloat16)
    rm.bind_fuser(model.memory_fuser, model.token_type_embedding)
    model.recurrent_memory_transformer = rm
    assert rm.layers[0].memory_segment_fusion_attention.attention_head_size == HD
    lm.train()
    model.embed_tokens.weight.requires_grad_(False)
    assert arch.plan_clip_batches(FRAMES7) == ([(4, [1, 2, 0])], [3])
    prompts = vb.PROMPTS5[:4]
    videos = [vb._video(f, v) for v, f in enumerate(FRAMES7)]
    ids, mask, labels, pos = vb._samples(prompts)
    lm.enable_clip_row_batches(True, training=True)
    off = vb._call(lm, ids, mask, labels, pos, videos)          # the switch off: today's grouping (no clip step at this width)
    off_emb = off[4].detach().clone()
    assert off[4].requires_grad and rm.row_batcher(4)._tragged is None
    model.zero_grad(set_to_none=True)
    with _switch():
        out = vb._call(lm, ids, mask, labels, pos, videos)
        emb = out[4]
        bp = rm.row_batcher(4)
        assert bp._tragged is True and [bp.video_steps(b) for b in range(4)] == [1, 1, 1, 0]
        assert emb.requires_grad and emb.shape == off_emb.shape
        assert torch.equal(out[5], off[5]) and torch.equal(out[2], off[2])
        err = O.rel_l2(to_np(emb.detach()), to_np(off_emb))
        print(f"\nentry point at 448, training forward: clip row batch (switch on) vs the switch off rel-L2 {err:.3e}")
        assert err <= ROW_BATCH_ROWS
        assert torch.equal(emb[3].detach(), off_emb[3]), "the 64-frame video's sample moved"
        cot = to_dev(O.bf16_round(O.hash_normal_like(tuple(emb.shape), 9995, 0.05))).float()
        (emb.float() * cot).sum().backward()
    n = 0
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad.float()).all(), k
            n += int(p.grad.float().abs().sum() > 0)
    assert n > 10
    lm.enable_clip_row_batches(False)
    bp.reset()
    rm.memory_cache = []
    model.zero_grad(set_to_none=True)


# ---- 6. the full width once -----------------------------------------------------------------------------------------------------------------------
def test_full_width_forward_and_backward_once():
    """D = 3584 (8 heads of 448), M = 1, clips of 3 and 1 frames on an engine of 2: one forward + backward; gradients finite and
    within the relative gate (1.5 x the single-video passes' error against float64)"""
    st = _setup("bf16", 3584, 8, 1)
    worst, worst_single = _clip_batch_vs_single_passes(st, (3, 1), 2, 1, 9800, "D = 3584")
    assert np.isfinite(worst) and np.isfinite(worst_single)
