"""-m gpu: clip row batches under autograd - videos of fewer than 32 frames and DIFFERENT frame counts train as one row batch.
The variable-length attention backward (`mavlm_attention_bwd_batch_varlen`, `ops.attention_bwd_batch_varlen`), the step
(`BatchedProjector.step_train_frames`), the token block (`video_memory_tokens_clips_train`) and the entry-point switch
(`enable_clip_row_batches(True, training=True)`).

Yardsticks: the single-video operators on separately allocated copies of each video's operands (bit for bit: every output row
has one owner, every video runs the plain grid of its own shape), oracle/backward.py at the operator gate of 1e-3,
oracle/torch_path.py float64 autograd summed over the videos at the project's gradient gates, and the single-video training
path (gates and statistic of tests/test_gpu_batch_train.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from memory_augmented_vlm_amd.model import llava_arch as arch
from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
from oracle import memory_path as O
from oracle import backward as OB
from oracle import torch_path as TP
from gpu_util import DT, to_dev, to_np
from test_gpu_batch_train import GRAD_TOL, OP_TOL
from test_gpu_ragged_batch import ROW_BATCH_ROWS, ROW_BATCH_SCORES
from test_gpu_ragged_train import CAP, _assert_no_unit_is_cut, _setup
from test_gpu_streamk_levels import _randn

pytestmark = pytest.mark.gpu
P = 196
FRAMES = (4, 2, 1)          # the clips of the step tests: 784, 392 and 196 keys
BIG = 3.0e4          # the sentinel of every gradient buffer: a row written that has no owner cannot go unnoticed
TAIL = 70            # sentinel rows behind the last video (more than one 64-row tile)


def _i32(v):
    return (capi.i32 * len(v))(*v)


def _i64(v):
    return (ctypes.c_int64 * len(v))(*v)


# ---- 1. the variable-length backward operator, bit for bit ------------------------------------------------------------------------------
def _bwd_varlen(q, k, v, o, do, lse, S, Hv, R, scale, want=(True, True, True)):
    """the export itself, into sentinel-filled buffers with a tail behind the last video: (dq, dk, dv) incl. their tails"""
    nb, tot, W = len(S), sum(S), Hv * 128
    dq = torch.full((nb * R + TAIL, W), -BIG, device="cuda", dtype=q.dtype)
    dk = torch.full((tot + TAIL, W), -BIG, device="cuda", dtype=q.dtype)
    dv = torch.full((tot + TAIL, W), -BIG, device="cuda", dtype=q.dtype)
    delta = torch.empty((nb * Hv, R), device="cuda", dtype=torch.float32)
    offs = [sum(S[:b]) * W for b in range(nb)]
    p = lambda t, on: t.data_ptr() if on else None
    capi.check(capi.lib().mavlm_attention_bwd_batch_varlen(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                                           o.data_ptr(), o.stride(0), do.data_ptr(), do.stride(0), lse.data_ptr(),
                                                           delta.data_ptr(), p(dq, want[0]), W, p(dk, want[1]), W, p(dv, want[2]), W, R,
                                                           _i32(S), _i64(offs), _i64(offs), nb * Hv, scale, nb, 128,
                                                           ops.dtype_code(q.dtype), ops.stream_ptr()), "mavlm_attention_bwd_batch_varlen")
    torch.cuda.synchronize()
    return dq, dk, dv


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("S", [(40, 64, 980), (128, 192)], ids=["lt1-1-15.3tiles", "2-3tiles"])
def test_varlen_backward_equals_the_single_video_backward_per_video(S, mode):
    """2 heads per video, R = 196 (two 128-query blocks, the second ragged).  Key counts: less than one 64-key tile, exactly one,
    15 tiles + 20 keys (eight 128-row key blocks, the last ragged); and one and two key blocks exactly (the dK / dV grid of the
    longer video is one block larger: the shorter video's surplus workgroups leave).  K / V / dK / dV are packed back to back: a
    load past a video's last key reads its neighbour's first (row 0 of every video is scaled up), a store past it lands in the
    neighbour's gradient or in the sentinel tail."""
    S = list(S)
    Hv, R, W = 2, 196, 256
    nb, tot = len(S), sum(S)
    q = _randn((nb * R, W), 9300, mode)
    do = _randn((nb * R, W), 9303, mode) * 0.5
    k, v = _randn((tot, W), 9301, mode), _randn((tot, W), 9302, mode)
    starts = [sum(S[:b]) for b in range(nb)]
    for s0 in starts:
        k[s0] *= 6.0
        v[s0] *= 50.0
    scale = ops.attn_scale(128)
    # forward per video on the plain grid; the variable-length forward operator gives the same rows
    fw = [ops.attention(q[b * R:(b + 1) * R], k[starts[b]:starts[b] + S[b]].clone(), v[starts[b]:starts[b] + S[b]].clone(), Hv,
                        want_lse=True, scale=scale, plain=True) for b in range(nb)]
    o, lse = torch.cat([f[0] for f in fw]), torch.cat([f[1] for f in fw]).contiguous()
    o_vl, lse_vl = ops.attention_batch_varlen(q, k, v, Hv, S, want_lse=True, scale=scale)
    assert torch.equal(o_vl, o) and torch.equal(lse_vl, lse)

    dq, dk, dv = _bwd_varlen(q, k, v, o, do, lse, S, Hv, R, scale)
    dq2, dk2, dv2 = _bwd_varlen(q, k, v, o, do, lse, S, Hv, R, scale)
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2), "a second launch differs from the first"
    for name, t, n in (("dQ", dq, nb * R), ("dK", dk, tot), ("dV", dv, tot)):
        assert bool((t[n:] == -BIG).all()), f"{name}: the tail behind the last video was written"
    r = O.rounder(mode)
    for b in range(nb):
        sl, kl = slice(b * R, (b + 1) * R), slice(starts[b], starts[b] + S[b])
        qb, kb, vb, ob, dob, lb = (q[sl].clone(), k[kl].clone(), v[kl].clone(), o[sl].clone(), do[sl].clone(),
                                   lse[b * Hv:(b + 1) * Hv].clone())              # separately allocated copies
        wq, wk, wv = ops.attention_bwd(qb, kb, vb, ob, dob, lb, Hv, scale=scale)
        torch.cuda.synchronize()
        assert torch.equal(dq[sl], wq), f"video {b} (S = {S[b]}): dQ differs from mavlm_attention_bwd"
        assert torch.equal(dk[kl], wk), f"video {b} (S = {S[b]}): dK differs from mavlm_attention_bwd"
        assert torch.equal(dv[kl], wv), f"video {b} (S = {S[b]}): dV differs from mavlm_attention_bwd"
        rq, rk, rv = OB.attention_bwd(to_np(qb), to_np(kb), to_np(vb), to_np(ob), to_np(dob), to_np(lb), Hv, mode)
        errs = (O.rel_l2(to_np(dq[sl]), r(rq)), O.rel_l2(to_np(dk[kl]), r(rk)), O.rel_l2(to_np(dv[kl]), r(rv)))
        print(f"\n[varlen bwd {mode} video {b} S={S[b]}] dq / dk / dv rel-L2 vs oracle {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
        assert max(errs) <= OP_TOL, (b, errs)
    # a gradient that is not asked for is not written, and the others keep their bits
    q_only = _bwd_varlen(q, k, v, o, do, lse, S, Hv, R, scale, want=(True, False, False))
    assert torch.equal(q_only[0], dq) and bool((q_only[1] == -BIG).all()) and bool((q_only[2] == -BIG).all())
    kv_only = _bwd_varlen(q, k, v, o, do, lse, S, Hv, R, scale, want=(False, True, True))
    assert bool((kv_only[0] == -BIG).all()) and torch.equal(kv_only[1], dk) and torch.equal(kv_only[2], dv)
    # the wrapper: its own destinations, and caller-owned ones that are column views of one wider buffer
    gq, gk, gv = ops.attention_bwd_batch_varlen(q, k, v, o, do, lse, Hv, S, scale=scale)
    assert torch.equal(gq, dq[:nb * R]) and torch.equal(gk, dk[:tot]) and torch.equal(gv, dv[:tot])
    dst = torch.full((tot + 3, 2 * W), -BIG, device="cuda", dtype=DT[mode])
    gq, gk, gv = ops.attention_bwd_batch_varlen(q, k, v, o, do, lse, Hv, S, need_dq=False, scale=scale, dk_out=dst[:tot, :W],
                                                dv_out=dst[:tot, W:])
    torch.cuda.synchronize()
    assert gq is None and torch.equal(dst[:tot, :W], dk[:tot]) and torch.equal(dst[:tot, W:], dv[:tot]) and bool((dst[tot:] == -BIG).all())


# ---- 2. the step: forward -------------------------------------------------------------------------------------------------------------------


def _clips(st, frames, seed, alt=None):
    """(host arrays on the 16-bit grid, device tensors) of clips of `frames` frames each, every clip its own data; `alt`: that
    clip holds other frames with rows of 1e4"""
    r = O.rounder(st.mode)
    xs = [r(O.hash_normal_like((f, P, st.D), seed + b) + O.hash_normal_like((f, 1, st.D), seed + 50 + b)) for b, f in enumerate(frames)]
    if alt is not None:
        x = np.array(r(O.hash_normal_like(xs[alt].shape, seed + 900)))
        x[0, :7] = 1e4
        xs[alt] = x
    return xs, [to_dev(x, st.mode) for x in xs]


def _cots(st, n, seed0):
    return [O.bf16_round(O.hash_normal_like((2, P, st.D), seed0 + 10 * b, 0.05)) for b in range(n)]


def _grads(rm):
    """the gradients a backward pass left (a clip takes one step: the evolution attention is not run and gets none)"""
    g = {k: p.grad.clone() for k, p in rm.named_parameters() if p.grad is not None}
    assert any(k.startswith("layers.") for k in g) and "initial_memory" in g
    return g


def _loss(bp, cots, videos):
    return sum((bp.memory_cache(b)[-1].float() * torch.from_numpy(cots[b]).cuda()).sum() for b in videos)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_step_forward_equals_clip_inference_and_single_video_training(mode):
    """clips of 4, 2 and 1 frames on an engine of 4: memories and frame scores of `step_train_frames` equal `step_frames`'s bit for
    bit, and - no attention plan cuts a unit at these key counts for 1 .. 3 videos (asserted) - the single-video training forward's"""
    st = _setup(mode)
    _assert_no_unit_is_cut(2 * P, 2, tuple(f * P for f in FRAMES))
    _, xs = _clips(st, FRAMES, 9900)
    bp = BatchedProjector(st.rm, 4)
    with torch.no_grad():
        bp.reset()
        views = [v.clone() for v in bp.step_frames(xs)]
        ref = [bp.memory_cache(b)[-1].clone() for b in range(3)]
        padded = bp.frame_scores[-1].clone()
    bp.reset()
    got = bp.step_train_frames(xs)
    torch.cuda.synchronize()
    assert bp._tragged is True and [bp.video_steps(b) for b in range(4)] == [1, 1, 1, 0]
    assert len(bp.frame_scores) == 1 and torch.equal(bp.frame_scores[-1], padded)
    rm = st.rm
    for b, f in enumerate(FRAMES):
        cache = bp.memory_cache(b)
        assert len(cache) == 1 and cache[0].requires_grad and tuple(cache[0].shape) == (2, P, st.D)
        assert torch.equal(cache[0].detach(), ref[b]), f"clip {b}: memory differs from the inference clip step"
        assert tuple(got[b].shape) == (f,) and not got[b].requires_grad and torch.equal(got[b], views[b]), f"clip {b}: frame scores"
        rm.memory_cache = []
        n0 = len(rm.frame_attn_scores)
        single, scores = rm(xs[b])
        assert single[-1].requires_grad
        assert torch.equal(single[-1].detach(), ref[b]), f"clip {b}: differs from the single-video training forward"
        assert torch.equal(scores[n0], views[b])
    rm.memory_cache = []
    bp.reset()


def test_equal_frame_counts_are_the_ragged_training_step():
    """clips of 3, 3 and 3 frames: `step_train_frames` takes the launches of `step_train(ragged=True)` - memories, frame scores and,
    after one backward pass of the same scalar, every parameter gradient are equal bit for bit"""
    st = _setup("bf16")
    rm = st.rm
    _, xs = _clips(st, (3, 3, 3), 9950)
    cots = _cots(st, 3, 9960)
    bp = BatchedProjector(rm, 4)
    runs = []
    for frames_form in (True, False):
        rm.zero_grad(set_to_none=True)
        bp.reset()
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
def _oracle_grads(mode, hidden=256, heads=2, frames=FRAMES, seed=9900):
    """float64 autograd of oracle/torch_path.py: every clip is one chunk of all its frames; summed over the clips (once per grid)"""
    st = _setup(mode, hidden, heads)
    host, _ = _clips(st, frames, seed)
    cots = _cots(st, len(frames), 9960)
    p = TP.params_from(st.w)
    loss = 0.0
    for b in range(len(frames)):
        cache = TP.run_steps(p, st.cfg, [host[b]], cache_cap=CAP)
        loss = loss + (cache[-1] * torch.from_numpy(cots[b]).double()).sum()
    return float(loss.detach()), TP.grads(p, loss)


def _grad_errors(name, grads, ref, single=None):
    """the statistic of tests/test_gpu_batch_train.py: rel-L2 per parameter against float64 (k_proj.bias: its norm against the
    largest gradient norm).  Returns (worst rel-L2, worst single-video rel-L2, failures of the k_proj.bias rule)"""
    scale = max(np.linalg.norm(v) for v in ref.values())
    worst, worst_single, fails = 0.0, 0.0, []
    for pname, g in grads.items():
        r = ref[TP.PFX + "." + pname]
        assert np.isfinite(g).all(), pname
        if pname.endswith("k_proj.bias"):                      # true gradient is 0 (softmax shift invariance)
            if np.linalg.norm(g) > 2e-3 * scale:
                fails.append((pname, "k_proj.bias", np.linalg.norm(g) / scale))
            continue
        eb = O.rel_l2(g, r)
        es = O.rel_l2(single[pname], r) if single is not None else float("nan")
        print(f"{name} {pname}: rel-L2 vs float64 clip batch {eb:.3e} single-video {es:.3e}")
        worst, worst_single = max(worst, eb), max(worst_single, es if single is not None else 0.0)
    return worst, worst_single, fails


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_clip_gradients_vs_float64_oracle_and_single_video_path(mode):
    """loss = sum over the clips of <memory, cotangent>: ONE backward pass over the clip batch (the variable-length attention
    backward in every formation layer) against the float64 oracle summed over the clips, and against three single-video backward
    passes accumulated by autograd"""
    st = _setup(mode)
    ref_loss, ref = _oracle_grads(mode)
    _, xs = _clips(st, FRAMES, 9900)
    cots = _cots(st, 3, 9960)
    rm = st.rm
    rm.zero_grad(set_to_none=True)
    single_loss = 0.0
    for b in range(3):
        rm.memory_cache = []
        cache, _ = rm(xs[b])
        l1 = (cache[-1].float() * torch.from_numpy(cots[b]).cuda()).sum()
        l1.backward()
        single_loss += float(l1.detach())
    rm.memory_cache = []
    single = {k: to_np(g) for k, g in _grads(rm).items()}
    rm.zero_grad(set_to_none=True)
    bp = BatchedProjector(rm, 4)
    bp.reset()
    bp.step_train_frames(xs)
    loss = _loss(bp, cots, range(3))
    loss.backward()
    bp.reset()
    batch = {k: to_np(g) for k, g in _grads(rm).items()}
    assert sorted(batch) == sorted(single)
    rm.zero_grad(set_to_none=True)
    print(f"\n{mode}: loss clip batch {float(loss.detach()):.5f} single-video {single_loss:.5f} float64 {ref_loss:.5f}")
    assert abs(float(loss.detach()) - single_loss) <= 1e-3 * abs(single_loss) + 1e-3
    worst, worst_single, fails = _grad_errors(mode, batch, ref, single)
    print(f"{mode}: worst-parameter rel-L2 vs float64: clip batch {worst:.3e}, three single-video passes {worst_single:.3e}")
    assert not fails, fails
    assert worst <= GRAD_TOL[mode], (worst, GRAD_TOL[mode])
    assert worst <= 1.5 * worst_single, (worst, worst_single)


# ---- 4. nothing leaks between clips -------------------------------------------------------------------------------------------------------------
def test_no_leak_between_clips():
    """the 2-frame clip (the middle of the packed keys) holds other frames with rows of 1e4: the other clips' memories and frame
    scores stay bit for bit, and so do the gradients of a loss over THEIR memories (the changed clip's rows then carry an upstream
    gradient of exactly 0 through every stacked operator)"""
    st = _setup("bf16")
    cots = _cots(st, 3, 9960)
    rm = st.rm
    runs = []
    for alt in (None, 1):
        _, xs = _clips(st, FRAMES, 9900, alt=alt)
        bp = BatchedProjector(rm, 4)
        rm.zero_grad(set_to_none=True)
        bp.reset()
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


# ---- 5. the token block -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["one_token", "grid"])
def test_clip_token_block_forward_and_gradients(layout):
    """`video_memory_tokens_clips_train`, the clips handed over shortest first: the blocks are `video_memory_tokens_clips`'s bits
    (the fuser's GEMM pair over the 3 * R stacked rows does not split its contraction - asserted); gradients reach the fuser,
    token_type_embedding, both prompts, image_newline and the recurrent module"""
    st = _setup("bf16")
    model, rm = st.model, st.rm
    with torch.no_grad():
        model.image_newline.copy_(to_dev(st.w["image_newline"]))
    caller = [1, 2, 4]
    _, vids = _clips(st, caller, 9970)
    idxs = [torch.arange(f) * 2 + b for b, f in enumerate(caller)]
    lib = capi.lib()
    rows, inter = 3 * 2 * P, model.memory_fuser[0].weight.shape[0]
    assert lib.mavlm_linear_ws_floats(rows, inter, st.D, capi.EPI_GELU, inter) == 0
    assert lib.mavlm_linear_ws_floats(rows, st.D, inter, capi.EPI_BIAS, st.D) == 0
    bp = BatchedProjector(rm, 4)
    with torch.no_grad():
        ref_toks, ref_info = arch.video_memory_tokens_clips(model, bp, vids, idxs, st.mp, st.fp, model.image_newline, layout=layout)
        ref_toks = [t.clone() for t in ref_toks]
    mp, fp = st.mp.clone().requires_grad_(True), st.fp.clone().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    toks, info = arch.video_memory_tokens_clips_train(model, bp, vids, idxs, mp, fp, model.image_newline, layout=layout)
    assert info["order"] == ref_info["order"] == [2, 1, 0] and info["num_memories"] == ref_info["num_memories"] == [1, 1, 1]
    assert info["block_rows"] == ref_info["block_rows"] == [t.shape[0] for t in toks]
    for b in range(3):
        assert toks[b].requires_grad and torch.equal(toks[b].detach(), ref_toks[b]), f"{layout} clip {b}: block"
    cots = [to_dev(O.bf16_round(O.hash_normal_like(tuple(t.shape), 9980 + b, 0.05))).float() for b, t in enumerate(toks)]
    sum((t.float() * c).sum() for t, c in zip(toks, cots)).backward()
    bp.reset()
    params = dict(model.named_parameters())
    # (a clip takes one step: the evolution attention is not run)
    watch = [k for k in params if k.startswith(("memory_fuser", "token_type_embedding", "image_newline", "recurrent_memory_transformer"))
             and "memory_update_attention" not in k]
    assert any(k.startswith("memory_fuser") for k in watch) and any(k.startswith("token_type_embedding") for k in watch)
    for k in watch:
        g = params[k].grad
        assert g is not None and torch.isfinite(g.float()).all(), k
        assert k.endswith("k_proj.bias") or g.float().abs().sum() > 0, k
    for name, t in (("memory prompt", mp), ("frame prompt", fp), ("image_newline", model.image_newline)):
        assert t.grad is not None and torch.isfinite(t.grad.float()).all() and t.grad.float().abs().sum() > 0, name
    model.zero_grad(set_to_none=True)


# ---- 6. hidden 896 ------------------------------------------------------------------------------------------------------------------------------
def test_hidden_896_step_token_block_and_gradients():
    """D = 896, 8 heads of 112 (zero-padded to 128 columns), M = 2, clips of 3 and 2 frames - the width the inference clip emit
    refuses.  The step against the single-video training forward (row-batch gates: the schedules may differ), the token block
    against the single-video training block, the gradients of the step against float64"""
    st = _setup("bf16", 896, 8)
    model, rm = st.model, st.rm
    frames = (3, 2)
    host, xs = _clips(st, frames, 9990)
    cots = _cots(st, 2, 9960)
    bp = BatchedProjector(rm, 2)
    rm.zero_grad(set_to_none=True)
    bp.reset()
    scores = bp.step_train_frames(xs)
    mems = [bp.memory_cache(b)[-1] for b in range(2)]
    _loss(bp, cots, range(2)).backward()
    batch = {k: to_np(g) for k, g in _grads(rm).items()}
    rm.zero_grad(set_to_none=True)
    for b, f in enumerate(frames):
        rm.memory_cache = []
        n0 = len(rm.frame_attn_scores)
        single, sc = rm(xs[b])
        err = O.rel_l2(to_np(mems[b].detach()), to_np(single[-1].detach()))
        serr = O.rel_l2(to_np(scores[b]), to_np(sc[n0]))
        print(f"\nhidden 896 clip {b} ({f} frames): memory vs single-video training forward {err:.2e}, frame scores {serr:.2e}")
        assert tuple(scores[b].shape) == (f,) and err <= ROW_BATCH_ROWS and serr <= ROW_BATCH_SCORES
    rm.memory_cache = []
    bp.reset()
    ref_loss, ref = _oracle_grads("bf16", 896, 8, frames, 9990)
    worst, _, fails = _grad_errors("hidden 896", batch, ref)
    print(f"hidden 896: worst-parameter rel-L2 vs float64 {worst:.3e}")
    assert not fails, fails
    assert worst <= GRAD_TOL["bf16"]
    # the token block
    with torch.no_grad():
        model.image_newline.copy_(to_dev(st.w["image_newline"]))
    idxs = [torch.arange(f) * 2 + b for b, f in enumerate(frames)]
    with pytest.raises(capi.MavlmError, match="multiple of 256"):
        with torch.no_grad():
            arch.video_memory_tokens_clips(model, bp, xs, idxs, st.mp, st.fp, model.image_newline)
    toks, info = arch.video_memory_tokens_clips_train(model, bp, xs, idxs, st.mp, st.fp, model.image_newline)
    for b, f in enumerate(frames):
        want, _ = arch.video_memory_tokens(model, xs[b], idxs[b], st.mp, st.fp, model.image_newline)
        assert toks[b].requires_grad and toks[b].shape == want.shape == (arch.video_token_rows(f, 2, P, True, 32, 32, CAP), 896)
        err = O.rel_l2(to_np(toks[b].detach()), to_np(want.detach()))
        print(f"hidden 896 clip {b}: token block vs the single-video training block {err:.2e}")
        assert err <= ROW_BATCH_ROWS
    sum(t.float().sum() for t in toks).backward()
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad.float()).all(), k
    assert model.memory_fuser[0].weight.grad is not None and model.memory_fuser[0].weight.grad.float().abs().sum() > 0
    rm.memory_cache = []
    bp.reset()
    model.zero_grad(set_to_none=True)


# ---- 7. the entry point ---------------------------------------------------------------------------------------------------------------------------
FRAMES7 = [9, 17, 12, 64]                     # three clips: one group on the engine of 4 (2 * 9 >= 17); the 64-frame video runs alone


def test_entry_point_clip_training_group():
    from test_gpu_video_batch import _host as lm_host, _video, _samples, _call, PROMPTS5
    lm, model, hf, _, _ = lm_host()
    lm.train()
    model.embed_tokens.weight.requires_grad_(False)
    rm = model.recurrent_memory_transformer
    assert [arch.sample_frame_count(f) for f in FRAMES7] == FRAMES7
    assert arch.plan_clip_batches(FRAMES7) == ([(4, [1, 2, 0])], [3])
    prompts = PROMPTS5[:4]
    videos = [_video(f, v) for v, f in enumerate(FRAMES7)]
    ids, mask, labels, pos = _samples(prompts)
    d0 = lm.draws
    off = _call(lm, ids, mask, labels, pos, videos)
    off_emb = off[4].detach().clone()
    assert off[4].requires_grad and lm.draws == d0 + 1
    model.zero_grad(set_to_none=True)
    lm.enable_clip_row_batches(True)                            # the inference switch alone: a training forward keeps its grouping
    same = _call(lm, ids, mask, labels, pos, videos)
    assert torch.equal(same[4].detach(), off_emb) and rm.row_batcher(4)._tragged is None and lm.draws == d0 + 2
    lm.enable_clip_row_batches(True, training=True)
    out = _call(lm, ids, mask, labels, pos, videos)
    emb = out[4]
    bp = rm.row_batcher(4)
    assert lm.draws == d0 + 3, "one dropout draw per forward"
    assert bp._tragged is True and [bp.video_steps(b) for b in range(4)] == [1, 1, 1, 0]
    assert emb.requires_grad and emb.shape == off_emb.shape
    assert torch.equal(out[5], off[5]) and torch.equal(out[2], off[2])
    err = O.rel_l2(to_np(emb.detach()), to_np(off_emb))
    print(f"\nentry point, training forward: clip row batch vs the switch off rel-L2 {err:.3e}")
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
    assert lm._clip_row_batches_train is False
    bp.reset()
    rm.memory_cache = []
    model.zero_grad(set_to_none=True)
