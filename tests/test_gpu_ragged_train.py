"""-m gpu: ragged row batches under autograd - `BatchedProjector.step_train(ragged=True)`, the ragged training token block
(`video_memory_tokens_ragged_train`) and the entry-point switch `enable_ragged_row_batches(True, training=True)`.

Default shape (that of tests/test_gpu_ragged_batch.py): D = 256 (2 heads of 128), M = 2, P = 196, chunks of 4 frames, FIFO of 2,
chunk counts (4, 2, 1) on a batch of 4: the active counts are 3, 2, 1, 1 and the longest video wraps the FIFO.  Every video carries
its own data.  Yardsticks: the ragged inference `step` and single-video training runs (bit for bit where the attention schedules
coincide - asserted through mavlm_attention_plan), oracle/torch_path.py float64 autograd per video with its own chunk list, summed
(gates of tests/test_gpu_batch_train.py, restated: 6e-2 bf16 / 2e-2 fp16 rel-L2 per parameter, k_proj.bias <= 2e-3 of the largest
gradient norm, ragged error <= 1.5 x the error of the single-video passes accumulated by autograd), and the row-batch gate 6e-3 of
tests/test_gpu_batch.py for the entry point."""
import functools
import types

import numpy as np
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd.model import llava_arch as arch
from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
from oracle import memory_path as O
from oracle import torch_path as TP
from gpu_util import to_dev, to_np
from test_gpu_batch import _host, _prompts

pytestmark = pytest.mark.gpu
GRAD_TOL = {"bf16": 6e-2, "fp16": 2e-2}       # tests/test_gpu_batch_train.py
ROW_BATCH_ROWS = 6e-3                         # tests/test_gpu_batch.py
P, CHUNK, CAP, FINE = 196, 4, 2, 3
CHUNKS = (4, 2, 1)


@functools.lru_cache(maxsize=None)
def _setup(mode="bf16", hidden=256, heads=2, M=2, seed=71):
    cfg = O.PathConfig(hidden=hidden, heads=heads, mem_tokens=M, depth=2, cache_cap=CAP, chunk=CHUNK, fine_frames=FINE)
    w = O.make_weights(cfg, seed=seed, grid=mode)
    model = _host(cfg, w, mode, cap=CAP)
    mp, fp = _prompts(hidden, mode)
    return types.SimpleNamespace(cfg=cfg, w=w, model=model, rm=model.recurrent_memory_transformer, mp=mp, fp=fp, mode=mode, D=hidden)


def _videos(st, chunks, seed, alt=False):
    """(host arrays on the 16-bit grid, device tensors) of videos of `chunks` chunks each; `alt`: the shortest (last) video holds
    other frames with rows of 1e4"""
    r = O.rounder(st.mode)
    xs = [r(O.hash_normal_like((c * CHUNK, P, st.D), seed + b) + O.hash_normal_like((c * CHUNK, 1, st.D), seed + 50 + b))
          for b, c in enumerate(chunks)]
    if alt:
        x = np.array(r(O.hash_normal_like(xs[-1].shape, seed + 900)))
        x[0, :7] = 1e4
        x[-1, 100:103] = -1e4
        xs[-1] = x
    return xs, [to_dev(x, st.mode) for x in xs]


def _segs(xs, chunks, i):
    return [x[i * CHUNK:(i + 1) * CHUNK] for x, c in zip(xs, chunks) if c > i]


def _ragged_train(bp, xs, chunks, per_step=False):
    """steps the videos (longest first) as a shrinking prefix under autograd; per_step: [(k, [newest memory per active video])]"""
    bp.reset()
    out = []
    for i in range(chunks[0]):
        segs = _segs(xs, chunks, i)
        sc = bp.step_train(segs, ragged=True)
        assert tuple(sc.shape) == (len(segs), CHUNK) and not sc.requires_grad
        if per_step:
            out.append((len(segs), [bp.memory_cache(b)[-1].detach().clone() for b in range(len(segs))]))
    return out


def _assert_no_unit_is_cut(R, H, keys):
    info = (capi.i32 * 4)()
    for S in keys:
        for nb in (1, 2, 3):
            capi.check(capi.lib().mavlm_attention_plan(R, S, H * nb, info), "plan")
            assert info[1] == 0 and (nb > 1 or info[3] <= 1), f"S={S} nb={nb}: plan {list(info)} cuts a unit"


# ---- 1. / 2. forward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_forward_equals_ragged_inference_and_single_video_training(mode):
    """memories and frame scores of ragged `step_train` equal ragged `step`'s bit for bit at every step (k = 3, 2, 1, 1: no
    attention plan cuts a unit at 1, 2, 3 videos - asserted -, which makes the lone steps comparable too), and three single-video
    training runs `rm(seg)`; FIFO bookkeeping per video."""
    st = _setup(mode)
    chunks = list(CHUNKS)
    _assert_no_unit_is_cut(2 * P, 2, (CHUNK * P, 2 * P, 4 * P))
    _, xs = _videos(st, chunks, 7200)
    bp = BatchedProjector(st.rm, 4)
    with torch.no_grad():
        bp.reset()
        ref_steps = []
        for i in range(chunks[0]):
            segs = _segs(xs, chunks, i)
            bp.step(segs)
            ref_steps.append([bp.memory_cache(b)[-1].clone() for b in range(len(segs))])
        ref_cache = [[m.clone() for m in bp.memory_cache(b)] for b in range(3)]
        ref_scores = [s.clone() for s in bp.frame_scores]
    steps = _ragged_train(bp, xs, chunks, per_step=True)
    torch.cuda.synchronize()
    assert [k for k, _ in steps] == [3, 2, 1, 1]
    assert [bp.video_steps(b) for b in range(4)] == [4, 2, 1, 0]
    for t, ((k, mems), ref) in enumerate(zip(steps, ref_steps)):
        for b in range(k):
            assert torch.equal(mems[b], ref[b]), f"step {t} video {b}: memory differs from the ragged inference step"
    assert len(bp.frame_scores) == 4
    for t, (sc, ref) in enumerate(zip(bp.frame_scores, ref_scores)):
        assert tuple(sc.shape) == tuple(ref.shape) and torch.equal(sc, ref), f"step {t}: frame scores"
    got = []
    for b, c in enumerate(chunks):
        cache = bp.memory_cache(b)
        assert len(cache) == min(c, CAP) and all(m.requires_grad and tuple(m.shape) == (2, P, st.D) for m in cache)
        for m, ref in zip(cache, ref_cache[b]):
            assert torch.equal(m.detach(), ref), f"video {b}: FIFO entry differs from the ragged inference batch"
        got.append([m.detach().clone() for m in cache])
    got_scores = [s.clone() for s in bp.frame_scores]
    # the finished videos' rows stay until the batch is reset: video 1 owns steps 0, 1, video 2 step 0, video 0 steps 2, 3
    assert bp._tsteps == [0, 1, 2, 3] and [m.shape[0] // (2 * P) for m in bp._tcache] == [3, 2, 1, 1]
    bp.reset()
    assert bp._tcache == [] and bp.frame_scores == [] and bp._tsteps == [] and bp._tevo == []
    rm = st.rm
    for b, c in enumerate(chunks):                                   # three single-video training runs
        rm.memory_cache = []
        n0 = len(rm.frame_attn_scores)
        for i in range(c):
            cache, scores = rm(xs[b][i * CHUNK:(i + 1) * CHUNK])
        assert all(m.requires_grad for m in cache) and len(cache) == len(got[b])
        for m, ref in zip(cache, got[b]):
            assert torch.equal(m.detach(), ref), f"video {b}: differs from the single-video training run"
        for i, sc in enumerate(scores[n0:]):
            assert torch.equal(sc, got_scores[i][b]), f"video {b} chunk {i}: frame scores"
    rm.memory_cache = []


# ---- 3. wide heads ---------------------------------------------------------------------------------------------------------------------
def test_forward_wide_heads():
    """D = 896, 2 heads of 448, chunk counts (3, 2, 1): the steps over k >= 2 videos are ragged `step`'s bits; the lone step is
    compared against the single-video training step fed the same state (video 0's two cached memories): the same launches."""
    st = _setup("bf16", 896, 2)
    chunks = [3, 2, 1]
    _, xs = _videos(st, chunks, 7500)
    bp = BatchedProjector(st.rm, 4)
    with torch.no_grad():
        bp.reset()
        ref_steps = []
        for i in range(chunks[0]):
            segs = _segs(xs, chunks, i)
            bp.step(segs)
            ref_steps.append([bp.memory_cache(b)[-1].clone() for b in range(len(segs))])
        ref_scores = [s.clone() for s in bp.frame_scores]
    steps = _ragged_train(bp, xs, chunks, per_step=True)
    torch.cuda.synchronize()
    assert [k for k, _ in steps] == [3, 2, 1]
    for t in (0, 1):
        for b in range(steps[t][0]):
            assert torch.equal(steps[t][1][b], ref_steps[t][b]), f"step {t} video {b}"
        assert torch.equal(bp.frame_scores[t], ref_scores[t]), f"step {t}: frame scores"
    lone, lone_scores = steps[2][1][0], bp.frame_scores[2][0].clone()
    err = O.rel_l2(to_np(lone), to_np(ref_steps[2][0]))
    print(f"wide heads, lone step: memory vs the ragged inference step rel-L2 {err:.2e}")       # (not gated: other launches)
    assert [len(bp.memory_cache(b)) for b in range(3)] == [2, 2, 1]
    # the single-video training step on the state the lone step started from (steps 0 and 1 of video 0)
    rm = st.rm
    rm.memory_cache = []
    rm._memory_cache = [steps[0][1][0].clone(), steps[1][1][0].clone()]
    rm._evo_kv, rm._train_steps, rm._cache_mode = [], 2, "autograd"
    n0 = len(rm.frame_attn_scores)
    cache, scores = rm(xs[0][2 * CHUNK:3 * CHUNK])
    assert torch.equal(cache[-1].detach(), lone), "the lone step differs from the single-video training step"
    assert torch.equal(scores[n0], lone_scores)
    rm._memory_cache = []
    rm.memory_cache = []
    bp.reset()


# ---- 4. gradients ----------------------------------------------------------------------------------------------------------------------
def _cots(st, chunks, seed0):
    return [[O.bf16_round(O.hash_normal_like((2, P, st.D), seed0 + 10 * b + t, 0.05)) for t in range(min(c, CAP))]
            for b, c in enumerate(chunks)]


def _loss(bp, cots, videos):
    return sum((c.float() * torch.from_numpy(g).cuda()).sum() for b in videos for c, g in zip(bp.memory_cache(b), cots[b]))


@functools.lru_cache(maxsize=None)
def _oracle_grads(mode):
    """float64 autograd of oracle/torch_path.py: every video with its own chunk list, summed (once per grid)"""
    st = _setup(mode)
    chunks = list(CHUNKS)
    host, _ = _videos(st, chunks, 7300)
    cots = _cots(st, chunks, 7400)
    p = TP.params_from(st.w)
    loss = 0.0
    for b, c in enumerate(chunks):
        cache = TP.run_steps(p, st.cfg, [host[b][i * CHUNK:(i + 1) * CHUNK] for i in range(c)], cache_cap=CAP)
        assert len(cache) == len(cots[b])
        loss = loss + sum((m * torch.from_numpy(g).double()).sum() for m, g in zip(cache, cots[b]))
    return float(loss.detach()), TP.grads(p, loss)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_ragged_gradients_vs_float64_oracle_and_single_video_path(mode):
    """loss = sum over videos and each video's own FIFO entries of <memory, cotangent>: ONE ragged backward pass against the float64
    oracle summed over the videos, and against three single-video backward passes accumulated by autograd."""
    st = _setup(mode)
    chunks = list(CHUNKS)
    ref_loss, ref = _oracle_grads(mode)
    _, xs = _videos(st, chunks, 7300)
    cots = _cots(st, chunks, 7400)
    rm = st.rm
    rm.zero_grad(set_to_none=True)
    single_loss = 0.0
    for b, c in enumerate(chunks):
        rm.memory_cache = []
        for i in range(c):
            cache, _ = rm(xs[b][i * CHUNK:(i + 1) * CHUNK])
        l1 = sum((m.float() * torch.from_numpy(g).cuda()).sum() for m, g in zip(cache, cots[b]))
        l1.backward()
        single_loss += float(l1.detach())
    rm.memory_cache = []
    single = {k: to_np(p.grad) for k, p in rm.named_parameters()}
    rm.zero_grad(set_to_none=True)
    bp = BatchedProjector(rm, 4)
    _ragged_train(bp, xs, chunks)
    loss = _loss(bp, cots, range(3))
    loss.backward()
    bp.reset()
    ragged = {k: to_np(p.grad) for k, p in rm.named_parameters()}
    rm.zero_grad(set_to_none=True)
    print(f"{mode}: loss ragged {float(loss.detach()):.5f} single-video {single_loss:.5f} float64 {ref_loss:.5f}")
    # (the forward is the single-video forward's bits - case 2 -: the two losses differ by fp32 summation order only)
    assert abs(float(loss.detach()) - single_loss) <= 1e-3 * abs(single_loss) + 1e-3
    scale = max(np.linalg.norm(v) for v in ref.values())
    tol = GRAD_TOL[mode]
    fails = []
    for pname, g in ragged.items():
        r = ref[TP.PFX + "." + pname]
        assert np.isfinite(g).all(), pname
        if pname.endswith("k_proj.bias"):                      # true gradient is 0 (softmax shift invariance)
            print(f"{mode} {pname}: |g| / largest norm ragged {np.linalg.norm(g) / scale:.2e} single {np.linalg.norm(single[pname]) / scale:.2e}")
            if np.linalg.norm(g) > 2e-3 * scale:
                fails.append((pname, "k_proj.bias", np.linalg.norm(g) / scale))
            continue
        eb, es = O.rel_l2(g, r), O.rel_l2(single[pname], r)
        print(f"{mode} {pname}: rel-L2 vs float64 ragged {eb:.3e} single-video {es:.3e} ratio {eb / max(es, 1e-30):.2f}")
        if not eb < tol:
            fails.append((pname, "gate", eb))
        if not eb <= 1.5 * es:
            fails.append((pname, "1.5 x single", eb, es))
    assert not fails, fails


# ---- 5. nothing leaks between videos ---------------------------------------------------------------------------------------------------
def test_no_leak_between_videos():
    """the shortest video holds other frames with rows of 1e4: the longer videos' memories stay bit for bit, and so do the
    gradients of a loss over THEIR FIFO entries (the other video's rows then carry an upstream gradient of exactly 0 through every
    stacked operator: they add zeros to each contraction, whatever they hold)."""
    st = _setup("bf16")
    chunks = list(CHUNKS)
    cots = _cots(st, chunks, 7400)
    rm = st.rm
    runs = []
    for alt in (False, True):
        _, xs = _videos(st, chunks, 7200, alt=alt)
        bp = BatchedProjector(rm, 4)
        rm.zero_grad(set_to_none=True)
        _ragged_train(bp, xs, chunks)
        mems = [[m.detach().clone() for m in bp.memory_cache(b)] for b in range(3)]
        scores = [s.clone() for s in bp.frame_scores]
        _loss(bp, cots, (0, 1)).backward()
        bp.reset()
        runs.append((mems, scores, {k: p.grad.clone() for k, p in rm.named_parameters()}))
    rm.zero_grad(set_to_none=True)
    (ma, sa, ga), (mb, sb, gb) = runs
    assert not torch.equal(ma[2][0], mb[2][0]) and torch.isfinite(mb[2][0].float()).all()
    for v in (0, 1):
        for x, y in zip(ma[v], mb[v]):
            assert torch.equal(x, y), f"video {v}: memory moved with another video's frames"
    for t, (x, y) in enumerate(zip(sa, sb)):
        n = min(2, x.shape[0])
        assert torch.equal(x[:n], y[:n]), f"step {t}: frame scores moved with another video's frames"
    for k in ga:
        assert torch.isfinite(gb[k].float()).all() and (k.endswith("k_proj.bias") or ga[k].float().abs().sum() > 0), k
        assert torch.equal(ga[k], gb[k]), f"{k}: the gradient of the longer videos' loss moved with another video's frames"


# ---- 6. the token block ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["one_token", "grid"])
def test_ragged_token_block_forward_and_gradients(layout):
    """`video_memory_tokens_ragged_train`, the videos handed over in a caller order other than longest first: the blocks are
    `video_memory_tokens_batched(ragged=True)`'s bits; the gradients of the fuser, token_type_embedding, image_newline and the
    recurrent module are finite, non-zero and within 6e-2 of the summed single-video training path."""
    st = _setup("bf16")
    model, rm = st.model, st.rm
    with torch.no_grad():
        model.image_newline.copy_(to_dev(st.w["image_newline"]))
    caller = [2, 1, 4]                                          # chunk counts in the caller's order: longest last
    _, vids = _videos(st, caller, 7600)
    idxs = [torch.arange(c * CHUNK) * 2 + b for b, c in enumerate(caller)]
    bp = BatchedProjector(rm, 4)
    kw = dict(chunk=CHUNK, fine_frames=FINE, layout=layout)
    with torch.no_grad():
        ref_toks, ref_info = arch.video_memory_tokens_batched(model, bp, vids, idxs, st.mp, st.fp, model.image_newline, ragged=True, **kw)
        ref_toks = [t.clone() for t in ref_toks]
    cots = [to_dev(O.bf16_round(O.hash_normal_like(tuple(t.shape), 7700 + b, 0.05))).float() for b, t in enumerate(ref_toks)]
    params = dict(model.named_parameters())
    watch = [k for k in params if k.startswith(("memory_fuser", "token_type_embedding", "image_newline",
                                                "recurrent_memory_transformer"))]
    model.zero_grad(set_to_none=True)
    for b in range(3):                                          # summed single-video training path
        toks1, _ = arch.video_memory_tokens(model, vids[b], idxs[b], st.mp, st.fp, model.image_newline, **kw)
        assert toks1.shape == ref_toks[b].shape
        (toks1.float() * cots[b]).sum().backward()
    rm.memory_cache = []
    single = {k: to_np(params[k].grad) for k in watch}
    model.zero_grad(set_to_none=True)
    toks, info = arch.video_memory_tokens_ragged_train(model, bp, vids, idxs, st.mp, st.fp, model.image_newline, **kw)
    assert info["order"] == ref_info["order"] == [2, 0, 1] and info["num_memories"] == ref_info["num_memories"] == [2, 1, 2]
    assert info["block_rows"] == ref_info["block_rows"] == [t.shape[0] for t in toks]
    for b in range(3):
        assert toks[b].requires_grad and torch.equal(toks[b].detach(), ref_toks[b]), f"{layout} video {b}: block"
    sum((t.float() * c).sum() for t, c in zip(toks, cots)).backward()
    bp.reset()
    scale = max(np.linalg.norm(v) for v in single.values())
    fails = []
    for k in watch:
        g = to_np(params[k].grad)
        assert np.isfinite(g).all(), k
        if k.endswith("k_proj.bias"):
            if np.linalg.norm(g) > 2e-3 * scale:
                fails.append((k, np.linalg.norm(g) / scale))
            continue
        assert g.any(), k
        e = O.rel_l2(g, single[k])
        print(f"{layout} {k}: ragged vs summed single-video rel-L2 {e:.3e}")
        if not e < GRAD_TOL["bf16"]:
            fails.append((k, e))
    model.zero_grad(set_to_none=True)
    assert not fails, fails


# ---- 6b. the equal-length step is the ragged step at k = B ------------------------------------------------------------------------------
def test_equal_length_step_is_the_ragged_step_at_k_equal_B():
    """3 videos of 4 chunks each on a batch of 3, FIFO of 2 (it wraps twice): `step_train(segs)` and, after `reset()`,
    `step_train(segs, ragged=True)` give the same memories of every video at every step, the same frame scores and - after one
    backward pass of the same scalar - the same gradients of `initial_memory`, an evolution-attention weight and a formation-layer
    weight, all bit for bit: a step over all videos of a cached entry uses the entry itself (no view node), so the graphs agree."""
    st = _setup("bf16")
    rm = st.rm
    chunks = [4, 4, 4]
    _, xs = _videos(st, chunks, 7800)
    cots = _cots(st, chunks, 7400)
    watch = ["initial_memory", "memory_update_attention.q_proj.weight", "layers.0.mlp.0.weight"]
    params = dict(rm.named_parameters())
    bp = BatchedProjector(rm, 3)
    runs = []
    for kw in ({}, {"ragged": True}):
        rm.zero_grad(set_to_none=True)
        bp.reset()
        mems = []
        for i in range(chunks[0]):
            sc = bp.step_train(_segs(xs, chunks, i), **kw)
            assert tuple(sc.shape) == (3, CHUNK)
            mems.append([[m.detach().clone() for m in bp.memory_cache(b)] for b in range(3)])
        assert bp._tragged is bool(kw) and all(len(c) == CAP for c in mems[-1])
        scores = [s.clone() for s in bp.frame_scores]
        _loss(bp, cots, range(3)).backward()
        bp.reset()
        runs.append((mems, scores, {k: params[k].grad.clone() for k in watch}))
    rm.zero_grad(set_to_none=True)
    (ma, sa, ga), (mb, sb, gb) = runs
    for t, (a, b) in enumerate(zip(ma, mb)):
        for v in range(3):
            assert len(a[v]) == len(b[v]) == min(t + 1, CAP)
            for x, y in zip(a[v], b[v]):
                assert torch.equal(x, y), f"step {t} video {v}: memory"
    assert len(sa) == len(sb) == 4 and all(torch.equal(x, y) for x, y in zip(sa, sb)), "frame scores"
    for k in watch:
        assert torch.isfinite(ga[k].float()).all() and ga[k].float().abs().sum() > 0, k
        assert torch.equal(ga[k], gb[k]), f"{k}: gradient of the equal-length step differs from the ragged step's at k = B"


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    st = _setup("bf16")
    bp = BatchedProjector(st.rm, 3)
    seg = lambda f=2, d=256: torch.zeros((f, P, d), device="cuda", dtype=torch.bfloat16)

    def idle():
        return bp._tcache == [] and bp.frame_scores == [] and bp._n == 0

    bp.reset()
    with pytest.raises(capi.MavlmError, match="first step"):
        bp.step_train([seg()], ragged=True)                     # a first step with one chunk
    with pytest.raises(capi.MavlmError, match="first step"):
        bp.step_train([seg()] * 4, ragged=True)                 # more than the batch
    with pytest.raises(capi.MavlmError, match="one shape"):
        bp.step_train([seg(), seg(3)], ragged=True)
    with pytest.raises(capi.MavlmError, match="3 chunks"):      # no keyword: exactly as before
        bp.step_train([seg(), seg()])
    assert idle()
    bp.step_train([seg() + b for b in range(2)], ragged=True)
    n = (len(bp._tcache), len(bp.frame_scores), bp._n)
    with pytest.raises(capi.MavlmError, match="never grows"):
        bp.step_train([seg()] * 3, ragged=True)                 # growing prefix
    with pytest.raises(capi.MavlmError, match="reset"):
        bp.step_train([seg()] * 3)                              # non-ragged after a ragged step
    with pytest.raises(capi.MavlmError, match="reset"):
        with torch.no_grad():
            bp.step([seg()] * 2)                                # `step` after `step_train`
    assert (len(bp._tcache), len(bp.frame_scores), bp._n) == n
    bp.step_train([seg()], ragged=True)
    with pytest.raises(capi.MavlmError, match="never grows"):
        bp.step_train([seg()] * 2, ragged=True)
    assert [bp.video_steps(b) for b in range(3)] == [2, 1, 0]
    bp.reset()
    assert idle()
    bp.step_train([seg()] * 3)
    with pytest.raises(capi.MavlmError, match="reset"):
        bp.step_train([seg()] * 3, ragged=True)                 # ragged after a non-ragged step
    assert len(bp._tcache) == 1
    bp.reset()
    with torch.no_grad():
        bp.step([seg()] * 3)
    with pytest.raises(capi.MavlmError, match="reset"):
        bp.step_train([seg()] * 2, ragged=True)
    bp.reset()


# ---- 8. the entry point ----------------------------------------------------------------------------------------------------------------
FRAMES8 = [70, 100, 110]                      # sampled 64, 96, 96: one ragged group of three (chunk counts 2, 3, 3)


def test_entry_point_ragged_training_group():
    from test_gpu_video_batch import _host as lm_host, _video, _samples, _call, PROMPTS3
    lm, model, hf, _, _ = lm_host()
    lm.train()
    model.embed_tokens.weight.requires_grad_(False)
    rm = model.recurrent_memory_transformer
    assert [arch.sample_frame_count(f) for f in FRAMES8] == [64, 96, 96]
    videos = [_video(f, v) for v, f in enumerate(FRAMES8)]
    ids, mask, labels, pos = _samples(PROMPTS3)
    off = _call(lm, ids, mask, labels, pos, videos)
    off_emb = off[4].detach().clone()
    assert off[4].requires_grad
    model.zero_grad(set_to_none=True)
    lm.enable_ragged_row_batches(True)                          # the inference switch alone: a training forward keeps its grouping
    same = _call(lm, ids, mask, labels, pos, videos)
    assert torch.equal(same[4].detach(), off_emb) and rm.row_batcher(4)._tragged is None
    lm.enable_ragged_row_batches(True, training=True)
    out = _call(lm, ids, mask, labels, pos, videos)
    emb = out[4]
    bp = rm.row_batcher(4)
    assert bp._tragged is True and [bp.video_steps(b) for b in range(4)] == [3, 3, 2, 0]
    assert emb.requires_grad and emb.shape == off_emb.shape
    assert torch.equal(out[5], off[5]) and torch.equal(out[2], off[2])
    err = O.rel_l2(to_np(emb.detach()), to_np(off_emb))
    print(f"entry point, training forward: ragged row batch vs the switch off rel-L2 {err:.3e}")
    assert err < ROW_BATCH_ROWS
    cot = to_dev(O.bf16_round(O.hash_normal_like(tuple(emb.shape), 8500, 0.05))).float()
    (emb.float() * cot).sum().backward()
    n = 0
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad.float()).all(), k
            n += int(p.grad.float().abs().sum() > 0)
    assert n > 10
    lm.enable_ragged_row_batches(False)
    assert lm._ragged_row_batches_train is False
    bp.reset()
    rm.memory_cache = []
    model.zero_grad(set_to_none=True)
