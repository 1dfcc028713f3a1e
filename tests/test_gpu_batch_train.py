"""-m gpu: row-batched training - forward and backward of several videos in one pass (`BatchedProjector.step_train`,
`mavlm_attention_batch`, `mavlm_attention_bwd_batch` / `_hd_batch`, `video_memory_tokens_batched_train`).

Every video of every case carries its own data: identical videos would hide a wrong video offset.  Yardsticks: per-video
launches of the single-video operators (bit for bit - no atomics, one owner per output row), the batched inference step (bit
for bit: same launches), oracle/backward.py at the operator gate of 1e-3, oracle/torch_path.py float64 autograd summed over the
videos at the project's gradient gates (6e-2 bf16, 2e-2 fp16, k_proj.bias <= 2e-3 of the largest gradient norm), and the
single-video training path (the batched gradients' error against the oracle <= 1.5 x the error of B single-video backward
passes accumulated by autograd - the factor of the envelope gate)."""
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
from gpu_util import to_dev, to_np, DT
from test_gpu_path import make_projector
from test_gpu_batch import _host, _prompts

pytestmark = pytest.mark.gpu
OP_TOL = 1e-3
GRAD_TOL = {"bf16": 6e-2, "fp16": 2e-2}
BIG = 3.0e4          # what the rows BETWEEN two videos hold: one of them read as a key, or written, cannot go unnoticed


# ---- 1. the batched backward operator ----------------------------------------------------------------------------------------------
@pytest.fixture(params=[0, 1])
def bwd_fused(request):
    """head width 128: separate dK / dV kernels and the fused dK+dV kernel (experiment switch)"""
    capi.check(capi.lib().mavlm_set_attention_bwd_fused(request.param), "set fused")
    yield request.param
    capi.lib().mavlm_set_attention_bwd_fused(0)


def _op_case(mode, hw, nb, Hv, R, S, seed):
    """Q / dO stacked [nb*R, W]; K / V column slices of ONE wider buffer [nb, S + gap, 2W + 64] whose other rows and columns hold
    BIG; distinct data per video."""
    r = O.rounder(mode)
    W = Hv * hw
    gap = 5
    Q = r(O.hash_normal_like((nb * R, W), seed, 1.0))
    dO = r(O.hash_normal_like((nb * R, W), seed + 1, 0.5))
    K = r(O.hash_normal_like((nb, S, W), seed + 2, 1.0))
    V = r(O.hash_normal_like((nb, S, W), seed + 3, 1.0))
    buf = torch.full((nb, S + gap, 2 * W + 64), BIG, device="cuda", dtype=DT[mode])
    buf[:, :S, 32:32 + W] = to_dev(K, mode)                      # (column offsets of 32 elements: 64-byte aligned heads)
    buf[:, :S, 32 + W:32 + 2 * W] = to_dev(V, mode)
    k, v = buf[:, :S, 32:32 + W], buf[:, :S, 32 + W:32 + 2 * W]
    assert k.stride(0) > S * k.stride(1)
    return Q, K, V, dO, to_dev(Q, mode), k, v, to_dev(dO, mode), gap


def _single_fwd(q, k, v, nb, Hv, R, hw):
    """per-video forwards on the never-split grid: (o [nb*R, W], lse [nb*Hv, R])"""
    os_, ls = [], []
    for b in range(nb):
        if hw == 128:
            o, l = ops.attention(q[b * R:(b + 1) * R], k[b], v[b], Hv, want_lse=True, plain=True, scale=ops.attn_scale(hw))
        else:
            o, l = ops.attention(q[b * R:(b + 1) * R], k[b], v[b], Hv, want_lse=True, head_dim=hw, scale=ops.attn_scale(hw))
        os_.append(o)
        ls.append(l)
    return torch.cat(os_), torch.cat(ls)


def _check_batched_bwd(mode, hw, nb, Hv, R, S, seed, oracle_video):
    Q, K, V, dO, q, k, v, do, gap = _op_case(mode, hw, nb, Hv, R, S, seed)
    W = Hv * hw
    scale = ops.attn_scale(hw)
    o, lse = _single_fwd(q, k, v, nb, Hv, R, hw)
    if hw == 128:
        # the batched forward operator on a shape without a stream-K plan: the plain grid per (video, head) = per-video launches
        ob, lb = ops.attention_batch(q, k, v, Hv, nb, want_lse=True, head_dim=128, scale=scale)
        assert torch.equal(ob, o) and torch.equal(lb, lse)
    single = []
    for b in range(nb):
        args = (q[b * R:(b + 1) * R], k[b], v[b], o[b * R:(b + 1) * R], do[b * R:(b + 1) * R], lse[b * Hv:(b + 1) * Hv], Hv)
        single.append(ops.attention_bwd(*args, scale=scale) if hw == 128 else ops.attention_bwd_hd(*args, hw, scale))
    sq = torch.cat([s[0] for s in single])
    sk, sv = torch.stack([s[1] for s in single]), torch.stack([s[2] for s in single])
    for need in ((True, False, False), (False, True, True), (True, True, True)):
        dst = torch.full((nb, S + gap, 2 * W), -BIG, device="cuda", dtype=DT[mode])
        dk_out, dv_out = dst[:, :S, :W], dst[:, :S, W:]
        dq, dk, dv = ops.attention_bwd_batch(q, k, v, o, do, lse, Hv, nb, *need, scale=scale, head_dim=hw, dk_out=dk_out, dv_out=dv_out)
        torch.cuda.synchronize()
        assert (dq is None) == (not need[0]) and (dk is None) == (not need[1]) and (dv is None) == (not need[2])
        if need[0]:
            assert torch.equal(dq, sq), need
        if need[1]:
            assert torch.equal(dk, sk) and torch.equal(dv, sv), need
        else:
            assert bool((dst == -BIG).all()), "dK / dV written although not asked for"
        assert bool((dst[:, S:] == -BIG).all()), "rows between two videos of the dK / dV destination were written"
    # default destinations: contiguous [nb, S, W]
    dq, dk, dv = ops.attention_bwd_batch(q, k, v, o, do, lse, Hv, nb, scale=scale, head_dim=hw)
    assert dk.is_contiguous() and torch.equal(dq, sq) and torch.equal(dk, sk) and torch.equal(dv, sv)
    if oracle_video is not None:
        r = O.rounder(mode)
        for b in oracle_video:
            sl = slice(b * R, (b + 1) * R)
            rq, rk, rv = OB.attention_bwd(Q[sl], K[b], V[b], to_np(o[sl]), dO[sl], to_np(lse[b * Hv:(b + 1) * Hv]), Hv, mode)
            errs = (O.rel_l2(to_np(dq[sl]), r(rq)), O.rel_l2(to_np(dk[b]), r(rk)), O.rel_l2(to_np(dv[b]), r(rv)))
            print(f"head {hw} {mode} video {b}: dq / dk / dv rel-L2 vs oracle {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
            assert max(errs) < OP_TOL, (b, errs)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_batched_attention_backward_equals_per_video_launches_head_128(mode, bwd_fused):
    """nb = 3 videos of Hv = 2 heads, R = 200 query rows (ragged against 32 / 64 / 128: more than one block), S = 260 keys
    (ragged too: the last tile of a video must read zeros, not the rows behind it - they hold 3e4); every video against the
    oracle (bf16, separate kernels)."""
    _check_batched_bwd(mode, 128, 3, 2, 200, 260, 4100, range(3) if (mode == "bf16" and not bwd_fused) else None)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_batched_attention_backward_equals_per_video_launches_head_448(mode):
    """the wide heads: nb = 2, Hv = 2, R = 100, S = 150 (ragged against the 32-row tiles and the 64 / 128-row blocks)"""
    _check_batched_bwd(mode, 448, 2, 2, 100, 150, 4200, range(2) if mode == "bf16" else None)


# ---- 3. training forward = batched inference forward ---------------------------------------------------------------------------------
SMALL = dict(hidden=256, heads=2, M=2, B=3, chunks=[4, 4, 4, 2], cap=2)      # T = 14 in chunks of 4: the FIFO (cap 2) wraps
WIDE = dict(hidden=896, heads=2, M=2, B=2, chunks=[1, 2], cap=10)            # 2 heads of 448


def _cfg(s):
    return O.PathConfig(hidden=s["hidden"], heads=s["heads"], mem_tokens=s["M"], depth=2)


def _videos(s, mode, seed0):
    """B distinct videos as lists of chunks (numpy, on the grid of `mode`)"""
    r = O.rounder(mode)
    T = sum(s["chunks"])
    bounds = np.cumsum([0] + s["chunks"])
    vids = [r(O.hash_normal_like((T, 196, s["hidden"]), seed0 + b)) for b in range(s["B"])]
    return [[v[bounds[i]:bounds[i + 1]] for i in range(len(s["chunks"]))] for v in vids]


def _train_steps(bp, vids, mode):
    bp.reset()
    for c in range(len(vids[0])):
        bp.step_train([to_dev(v[c], mode) for v in vids])


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_training_forward_equals_batched_inference_and_single_training(mode):
    """hidden 256, 2 heads, M = 2, B = 3, chunks 4 4 4 2 with a FIFO of 2 (it wraps; ragged last chunk) - the shape of
    test_row_batch_bit_identical_when_the_schedules_coincide: caches and frame scores of `step_train` equal `step`'s, and -
    the schedules coincide - those of three single-video training runs."""
    s = SMALL
    cfg = _cfg(s)
    rm = make_projector(cfg, O.make_weights(cfg, seed=61, grid=mode), mode, cache_cap=s["cap"])
    vids = _videos(s, mode, 7100)
    B = s["B"]
    bp = BatchedProjector(rm, B)
    with torch.no_grad():
        bp.reset()
        for c in range(len(s["chunks"])):
            bp.step([to_dev(v[c], mode) for v in vids])
        ref_cache = [[m.clone() for m in bp.memory_cache(b)] for b in range(B)]
        ref_scores = [sc.clone() for sc in bp.frame_scores]
    rm.train()
    _train_steps(bp, vids, mode)
    torch.cuda.synchronize()
    assert len(bp.frame_scores) == len(s["chunks"])
    for sc, ref in zip(bp.frame_scores, ref_scores):
        assert tuple(sc.shape) == tuple(ref.shape) and not sc.requires_grad and torch.equal(sc, ref)
    for b in range(B):
        cache = bp.memory_cache(b)
        assert len(cache) == s["cap"] and all(m.requires_grad and tuple(m.shape) == (s["M"], 196, s["hidden"]) for m in cache)
        for m, ref in zip(cache, ref_cache[b]):
            assert torch.equal(m.detach(), ref), f"video {b}"
    got = [[m.detach().clone() for m in bp.memory_cache(b)] for b in range(B)]
    got_scores = [sc.clone() for sc in bp.frame_scores]
    bp.reset()
    assert bp.frame_scores == [] and bp._tcache == []
    for b in range(B):                                         # three single-video training runs
        rm.memory_cache = []
        n0 = len(rm.frame_attn_scores)
        for c in range(len(s["chunks"])):
            cache, scores = rm(to_dev(vids[b][c], mode))
        assert all(m.requires_grad for m in cache)
        for m, ref in zip(cache, got[b]):
            assert torch.equal(m.detach(), ref), f"video {b}"
        for c, sc in enumerate(scores[n0:]):
            assert torch.equal(sc, got_scores[c][b]), f"video {b} chunk {c}"
    rm.memory_cache = []


def test_training_forward_equals_batched_inference_8_tokens():
    """hidden 1024, 8 heads, M = 8 (the checkpoint shape: 1568 query rows per video), B = 2, chunks of 32 and 7 frames: the
    caches of `step_train` against `step`'s (the stacked grid takes its own attention schedule: no single-video comparison)"""
    cfg = O.PathConfig(hidden=1024, heads=8, mem_tokens=8, depth=2)
    rm = make_projector(cfg, O.make_weights(cfg, seed=62), "bf16")
    vids = [[O.bf16_round(O.hash_normal_like((f, 196, 1024), 7200 + 10 * b + c)) for c, f in enumerate((32, 7))] for b in range(2)]
    bp = BatchedProjector(rm, 2)
    with torch.no_grad():
        bp.reset()
        for c in range(2):
            bp.step([to_dev(v[c]) for v in vids])
        ref = [[m.clone() for m in bp.memory_cache(b)] for b in range(2)]
    rm.train()
    _train_steps(bp, vids, "bf16")
    for b in range(2):
        cache = bp.memory_cache(b)
        assert len(cache) == 2
        for m, r_ in zip(cache, ref[b]):
            assert m.requires_grad and torch.equal(m.detach(), r_), f"video {b}"
    bp.reset()


# ---- 4. gradients ------------------------------------------------------------------------------------------------------------------
def _cots(s, n, seed0):
    return [[O.bf16_round(O.hash_normal_like((s["M"], 196, s["hidden"]), seed0 + 10 * b + t, 0.05)) for t in range(n)]
            for b in range(s["B"])]


@functools.lru_cache(maxsize=None)
def _oracle_grads(name, mode):
    """float64 autograd of oracle/torch_path.py, summed over the videos (computed once per shape and grid)"""
    s = {"small": SMALL, "wide": WIDE}[name]
    cfg = _cfg(s)
    w = O.make_weights(cfg, seed=17, grid=mode)
    vids = _videos(s, mode, 7300)
    n = min(len(s["chunks"]), s["cap"])
    cots = _cots(s, n, 7400)
    p = TP.params_from(w)
    loss = 0.0
    for b in range(s["B"]):
        cache = TP.run_steps(p, cfg, vids[b], cache_cap=s["cap"])
        loss = loss + sum((c * torch.from_numpy(g).double()).sum() for c, g in zip(cache, cots[b]))
    return w, vids, cots, float(loss.detach()), TP.grads(p, loss)


@pytest.mark.parametrize("name,mode", [("small", "bf16"), ("small", "fp16"), ("wide", "bf16")])
def test_batched_gradients_vs_float64_oracle_and_single_video_path(name, mode):
    """loss = sum over videos and cache entries of <cache, cotangent>; every parameter gradient of ONE batched backward pass
    against the float64 oracle summed over the videos, and against B single-video backward passes accumulated by autograd."""
    s = {"small": SMALL, "wide": WIDE}[name]
    cfg = _cfg(s)
    w, vids, cots, ref_loss, ref = _oracle_grads(name, mode)
    rm = make_projector(cfg, w, mode, cache_cap=s["cap"]).train()
    B = s["B"]
    # B single-video passes, gradients accumulated in the parameters' .grad
    rm.zero_grad(set_to_none=True)
    single_loss = 0.0
    for b in range(B):
        rm.memory_cache = []
        for seg in vids[b]:
            cache, _ = rm(to_dev(seg, mode))
        l1 = sum((c.float() * torch.from_numpy(g).cuda()).sum() for c, g in zip(cache, cots[b]))
        l1.backward()
        single_loss += float(l1.detach())
    rm.memory_cache = []
    single = {k: to_np(p.grad) for k, p in rm.named_parameters()}
    # one batched pass
    rm.zero_grad(set_to_none=True)
    bp = BatchedProjector(rm, B)
    _train_steps(bp, vids, mode)
    loss = sum((c.float() * torch.from_numpy(g).cuda()).sum() for b in range(B) for c, g in zip(bp.memory_cache(b), cots[b]))
    loss.backward()
    bp.reset()
    batched = {k: to_np(p.grad) for k, p in rm.named_parameters()}
    print(f"{name} {mode}: loss batched {float(loss.detach()):.5f} single-video {single_loss:.5f} float64 {ref_loss:.5f}")
    # (the forward of these shapes is the single-video forward's bits - case 3 - so the two losses differ by fp32 summation order
    #  only; the float64 loss is printed, not gated: a sum of cancelling terms of a 16-bit forward)
    assert abs(float(loss.detach()) - single_loss) <= 1e-3 * abs(single_loss) + 1e-3
    scale = max(np.linalg.norm(v) for v in ref.values())
    tol = GRAD_TOL[mode]
    fails = []
    for pname, g in batched.items():
        r = ref[TP.PFX + "." + pname]
        assert np.isfinite(g).all(), pname
        if pname.endswith("k_proj.bias"):                      # true gradient is 0 (softmax shift invariance)
            print(f"{name} {mode} {pname}: |g| / largest norm batched {np.linalg.norm(g) / scale:.2e} single {np.linalg.norm(single[pname]) / scale:.2e}")
            if np.linalg.norm(g) > 2e-3 * scale:
                fails.append((pname, "k_proj.bias", np.linalg.norm(g) / scale))
            continue
        eb, es = O.rel_l2(g, r), O.rel_l2(single[pname], r)
        print(f"{name} {mode} {pname}: rel-L2 vs float64 batched {eb:.3e} single-video {es:.3e} ratio {eb / max(es, 1e-30):.2f}")
        if not eb < tol:
            fails.append((pname, "gate", eb))
        if not eb <= 1.5 * es:
            fails.append((pname, "1.5 x single", eb, es))
    assert not fails, fails


# ---- 5. the whole token block ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["one_token", "grid"])
def test_batched_token_block_forward_and_gradients(layout):
    """`video_memory_tokens_batched_train` on the small shape (PE add, 4 chunks, fuser over all videos' rows, type rows, layout,
    concat): the tokens are `video_memory_tokens_batched`'s bits; the gradients of the fuser, the token-type embedding,
    image_newline and the recurrent module are finite, non-zero and within the gates against the summed single-video path."""
    s = SMALL
    cfg = _cfg(s)
    w = O.make_weights(cfg, seed=61)
    model = _host(cfg, w, "bf16", cap=s["cap"])
    with torch.no_grad():
        model.image_newline.copy_(to_dev(w["image_newline"]))
    rm = model.recurrent_memory_transformer
    B, T = s["B"], 14
    vids = [to_dev(O.bf16_round(O.hash_normal_like((T, 196, 256), 7500 + b))) for b in range(B)]
    idx = torch.arange(T) * 2
    mp, fp = _prompts(256)
    bp = BatchedProjector(rm, B)
    with torch.no_grad():
        ref_toks, ref_info = arch.video_memory_tokens_batched(model, bp, vids, idx, mp, fp, model.image_newline, chunk=4,
                                                              layout=layout)
        ref_toks = ref_toks.clone()
    model.train()
    cot = to_dev(O.bf16_round(O.hash_normal_like(tuple(ref_toks.shape), 7600, 0.05))).float()
    params = dict(model.named_parameters())
    watch = [k for k in params if k.startswith(("memory_fuser", "token_type_embedding", "image_newline",
                                                "recurrent_memory_transformer"))]
    # summed single-video training path
    model.zero_grad(set_to_none=True)
    for b in range(B):
        toks1, _ = arch.video_memory_tokens(model, vids[b], idx, mp, fp, model.image_newline, chunk=4, layout=layout)
        (toks1.float() * cot[b]).sum().backward()
    rm.memory_cache = []
    single = {k: to_np(params[k].grad) for k in watch}
    model.zero_grad(set_to_none=True)
    toks, info = arch.video_memory_tokens_batched_train(model, bp, vids, idx, mp, fp, model.image_newline, chunk=4, layout=layout)
    assert toks.requires_grad and tuple(toks.shape) == tuple(ref_toks.shape)
    assert info["memory_rows"] == ref_info["memory_rows"] and info["num_memories"] == 2
    assert torch.equal(toks.detach(), ref_toks)
    (toks.float() * cot).sum().backward()
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
        print(f"{layout} {k}: batched vs summed single-video rel-L2 {e:.3e}")
        if not e < GRAD_TOL["bf16"]:
            fails.append((k, e))
    assert not fails, fails


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    cfg = _cfg(SMALL)
    rm = make_projector(cfg, O.make_weights(cfg, seed=61), "bf16").train()
    bp = BatchedProjector(rm, 3)
    seg = lambda f=2, d=256: torch.zeros((f, 196, d), device="cuda", dtype=torch.bfloat16)
    bp.reset()
    with pytest.raises(capi.MavlmError, match="3 chunks"):
        bp.step_train([seg(), seg()])
    with pytest.raises(capi.MavlmError, match="one shape"):
        bp.step_train([seg(), seg(), seg(3)])
    with pytest.raises(capi.MavlmError, match="expected"):
        bp.step_train([seg(2, 128)] * 3)
    bp.record_attention_maps = True
    with pytest.raises(capi.MavlmError, match="record_attention_maps"):
        bp.step_train([seg()] * 3)
    bp.record_attention_maps = False
    assert bp._tcache == [] and bp.frame_scores == []            # nothing ran
    bp.step_train([seg() + b for b in range(3)])
    with pytest.raises(capi.MavlmError, match="reset"):
        bp.step([seg()] * 3)
    bp.reset()
    bp.step([seg()] * 3)
    with pytest.raises(capi.MavlmError, match="reset"):
        bp.step_train([seg()] * 3)
    bp.reset()
    bp.step_train([seg()] * 3)
    assert len(bp.memory_cache(1)) == 1 and bp.memory_cache(1)[0].requires_grad
    bp.reset()
