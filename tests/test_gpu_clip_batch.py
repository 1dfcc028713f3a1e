"""-m gpu: clip row batches - videos of fewer than 32 frames, DIFFERENT frame counts in one step.  The variable-length operators
(`mavlm_attention_batch_varlen`, `mavlm_attention_colsum_batch_varlen`), the step (`mavlm_step_batch_frames`,
`BatchedProjector.step_frames`), the emit (`mavlm_fuse_emit_layout_frames_to`, `video_memory_tokens_clips`) and the entry-point
switch (`enable_clip_row_batches`).

Yardsticks: the single-video operators / engine on each video's own operands (bit for bit where the schedules coincide: the
variable-length forward is the plain grid per video, the column sums run each video's own balanced schedule), float64 through
`gpu_util.attention_gate`, the emulation oracle under `chain_tol`, and the row-batch gates of tests/test_gpu_ragged_batch.py
(ROW_BATCH_ROWS 6e-3, ROW_BATCH_SCORES 5e-3).  Default shape: that file's fixture (D = 256, 2 heads, M = 2, depth 2)."""
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
from gpu_util import DT, attention_gate, to_dev, to_np
from test_gpu_colsum_batch import OP_TOL, _float64_colsum
from test_gpu_layouts import SENTINEL, bits
from test_gpu_path import chain_tol
from test_gpu_ragged_batch import ROW_BATCH_ROWS, ROW_BATCH_SCORES, _pe, _setup
from test_gpu_streamk_levels import _randn, _ref64

pytestmark = pytest.mark.gpu
P = 196


@pytest.fixture(autouse=True)
def _inference_path():
    with torch.no_grad():
        yield


def _i32(v):
    return (capi.i32 * len(v))(*v)


def _i64(v):
    return (ctypes.c_int64 * len(v))(*v)


def _plan(R, S, H):
    info = (capi.i32 * 4)()
    capi.check(capi.lib().mavlm_attention_plan(R, S, H, info), "mavlm_attention_plan")
    return list(info)


# ---- 1. the variable-length forward, bit for bit ------------------------------------------------------------------------------------------
def _varlen_forward(q, kv_k, kv_v, S, offs, Hv, R, scale, lse=True):
    nb = len(S)
    out = torch.full((nb * R, Hv * 128), float("nan"), device="cuda", dtype=q.dtype)
    l2 = torch.full((nb * Hv, R), float("nan"), device="cuda", dtype=torch.float32)
    capi.check(capi.lib().mavlm_attention_batch_varlen(q.data_ptr(), q.stride(0), kv_k.data_ptr(), kv_k.stride(0), kv_v.data_ptr(),
                                                       kv_v.stride(0), out.data_ptr(), out.stride(0), l2.data_ptr() if lse else None, R,
                                                       _i32(S), _i64(offs), nb * Hv, scale, nb, 128, ops.dtype_code(q.dtype),
                                                       ops.stream_ptr()), "mavlm_attention_batch_varlen")
    torch.cuda.synchronize()
    return out, l2


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("S", [(40, 64, 980), (128, 192)], ids=["lt1-1-15.3tiles", "2-3tiles"])
def test_varlen_forward_equals_the_plain_grid_per_video(S, mode):
    """2 heads per video, R = 196 (two query blocks, the second ragged).  Key counts: less than one 64-key tile, exactly one, 15
    tiles + 20 keys; and 2 and 3 tiles (the pipeline prologue).  K / V are packed back to back: a load past a video's last key would
    read its neighbour's rows (row 0 of every video is scaled up, so such a key cannot go unnoticed)."""
    Hv, R, W = 2, 196, 256
    nb, tot = len(S), sum(S)
    q = _randn((nb * R, W), 9100, mode)
    q[3] *= 8.0                                            # (the deferred rescale fires inside the tile loop)
    k, v = _randn((tot, W), 9101, mode), _randn((tot, W), 9102, mode)
    starts = [sum(S[:b]) for b in range(nb)]
    for s0 in starts:
        k[s0] *= 6.0
        v[s0] *= 50.0
    scale = ops.attn_scale(128)
    out, l2 = _varlen_forward(q, k, v, list(S), [s0 * W for s0 in starts], Hv, R, scale)
    again, l2_again = _varlen_forward(q, k, v, list(S), [s0 * W for s0 in starts], Hv, R, scale)
    assert torch.equal(out, again) and torch.equal(l2, l2_again)
    for b in range(nb):
        qb = q[b * R:(b + 1) * R]
        kb, vb = k[starts[b]:starts[b] + S[b]].clone(), v[starts[b]:starts[b] + S[b]].clone()      # separately allocated copies
        want, want_l2 = ops.attention(qb, kb, vb, Hv, want_lse=True, scale=scale, plain=True)
        torch.cuda.synchronize()
        assert torch.equal(out[b * R:(b + 1) * R], want), f"video {b} (S = {S[b]}): O differs from mavlm_attention"
        assert torch.equal(l2[b * Hv:(b + 1) * Hv], want_l2), f"video {b} (S = {S[b]}): lse2 differs from mavlm_attention"
        ref_ctx, ref_lse2, _ = _ref64(qb, kb, vb, Hv, 128, scale)
        g, lerr, ok = attention_gate(out[b * R:(b + 1) * R], l2[b * Hv:(b + 1) * Hv], ref_ctx, ref_lse2, Hv, mode)
        print(f"\n[varlen {mode} video {b} S={S[b]}] {g}; worst lse2 error {lerr:.2e}")
        assert ok, (b, str(g), lerr)
    # without lse2: the same O
    out2, _ = _varlen_forward(q, k, v, list(S), [s0 * W for s0 in starts], Hv, R, scale, lse=False)
    assert torch.equal(out2, out)


# ---- 2. the variable-length column sums, bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_varlen_colsum_equals_per_video_launches(mode):
    """R = 1568, H = 8, S = (980, 6076): the single-video plans write 4 and 3 planes, the grids differ - the launch takes the
    largest and the shorter video's surplus workgroups leave.  Keys packed back to back; `part` pre-filled with a sentinel."""
    R, H, S = 1568, 8, (980, 6076)
    W = H * 128
    lib = capi.lib()
    plans = []
    for s in S:
        info = (capi.i32 * 2)()
        capi.check(lib.mavlm_attention_colsum_plan(R, s, H, info), "mavlm_attention_colsum_plan")
        plans.append(list(info))
    assert [p[1] for p in plans] == [4, 3] and plans[0][0] != plans[1][0], plans
    r = O.rounder(mode)
    Q = r(O.hash_normal_like((2 * R, W), 9200, 1.0))
    K = r(O.hash_normal_like((sum(S), W), 9201, 1.0))
    q, k = to_dev(Q, mode), to_dev(K, mode)
    starts = [0, S[0]]
    scale = ops.attn_scale(128)
    lse, single = [], []
    zeros = torch.zeros_like(k)
    for b in range(2):
        qb, kb = q[b * R:(b + 1) * R], k[starts[b]:starts[b] + S[b]].clone()
        lse.append(ops.attention(qb, kb, zeros[:S[b]], H, want_lse=True, scale=scale, plain=True)[1])
        single.append(ops.attention_colsum(qb, kb, lse[b], H, scale=scale))
    lse = torch.cat(lse).contiguous()
    per = [int(lib.mavlm_attention_colsum_floats(R, s, H)) for s in S]
    need = int(lib.mavlm_attention_colsum_batch_varlen_floats(R, _i32(S), H, 2))
    assert need == sum(per)
    tail = 64
    buf = torch.full((need + tail,), -7.25, device="cuda", dtype=torch.float32)
    capi.check(lib.mavlm_attention_colsum_batch_varlen(q.data_ptr(), W, k.data_ptr(), W, _i64([s0 * W for s0 in starts]), lse.data_ptr(),
                                                       buf.data_ptr(), need, R, _i32(S), H, 2, 128, scale, ops.dtype_code(q.dtype),
                                                       ops.stream_ptr()), "mavlm_attention_colsum_batch_varlen")
    torch.cuda.synchronize()
    at = 0
    for b in range(2):
        got = buf[at:at + H * S[b]].view(H, S[b])
        assert torch.equal(got, single[b]), f"video {b}: column sums differ from mavlm_attention_colsum"
        assert bool((buf[at + plans[b][1] * H * S[b]:at + per[b]] == -7.25).all()), f"video {b}: written behind its planes"
        ref = _float64_colsum(Q[b * R:(b + 1) * R], K[starts[b]:starts[b] + S[b]], H, 128, scale)
        err = O.rel_l2(to_np(got), ref)
        print(f"varlen colsum {mode} video {b} S={S[b]}: rel-L2 vs float64 {err:.2e} (planes {plans[b][1]}, workgroups {plans[b][0]})")
        assert err < OP_TOL
        at += per[b]
    assert bool((buf[need:] == -7.25).all()), "written behind the buffer"


# ---- 3. the step against the single-video engine and the oracle ---------------------------------------------------------------------------
def _clips(st, frames, seed, alt=None):
    """(host arrays on the 16-bit grid, device tensors, frame indices) of clips of `frames` frames each"""
    r = O.rounder(st.mode)
    xs = [r(O.hash_normal_like((f, P, st.D), seed + b) + O.hash_normal_like((f, 1, st.D), seed + 50 + b)) for b, f in enumerate(frames)]
    if alt is not None:
        xs[alt] = np.array(r(O.hash_normal_like(xs[alt].shape, seed + 900)))
        xs[alt][0, :7] = 1e4
    return xs, [to_dev(x, st.mode) for x in xs], [torch.arange(f) * 2 + b for b, f in enumerate(frames)]


def _single_clip(st, vid, idx, layout="one_token", wf=True):
    """the single-video engine on one clip (one chunk of all its frames): block, memory, frame scores"""
    rm = st.rm
    n0 = len(rm.frame_attn_scores)
    tok, info = arch.video_memory_tokens(st.model, vid, idx, st.mp, st.fp, None if layout == "no_token" else st.nl, wf, chunk=32,
                                         fine_frames=32, layout=layout)
    torch.cuda.synchronize()
    assert info["num_memories"] == 1 and len(rm.frame_attn_scores) == n0 + 1
    return tok.clone(), rm.memory_cache[0].clone(), rm.frame_attn_scores[n0].clone()


@functools.lru_cache(maxsize=None)
def _case3(mode="bf16", frames=(4, 2, 1), seed=9300, alt=None, scores=True, score_mode=1):
    st = _setup(mode)
    host, vids, idxs = _clips(st, frames, seed, alt)
    xs = [_pe(st, v, i) for v, i in zip(vids, idxs)]
    bp = BatchedProjector(st.rm, 4)
    bp.compute_frame_scores = scores
    lib = capi.lib()
    capi.check(lib.mavlm_set_frame_score_mode(score_mode), "frame score mode")
    try:
        bp.reset()
        views = bp.step_frames(xs)
        torch.cuda.synchronize()
    finally:
        lib.mavlm_set_frame_score_mode(1)
    eng = bp._engine
    assert lib.mavlm_steps(eng.ctx) == 1 and [lib.mavlm_video_steps(eng.ctx, b) for b in range(4)] == [1] * len(frames) + [0] * (4 - len(frames))
    return dict(st=st, host=host, vids=vids, idxs=idxs, xs=xs, bp=bp, frames=frames,
                mems=[bp.memory_cache(b)[-1].clone() for b in range(len(frames))],
                scores=None if views is None else [v.clone() for v in views],
                padded=None if views is None else bp.frame_scores[-1].clone())


def _oracle_clip(st, host, idx, b, n):
    def run(acc):
        with O.accumulate_in(acc):
            xp = O.pe_add(host, idx.numpy(), st.w["positional_encoding.frame_embed"], st.mode)
            rm = O.RecurrentMemory(st.cfg, st.w, st.mode)
            rm.reset()
            O.ROW_BATCH = (b, n)
            try:
                rm.step(xp)
            finally:
                O.ROW_BATCH = (0, 1)
            return rm.memory_cache[-1].reshape(-1, st.D), rm.frame_attn_scores[-1]
    ref, rsc = run(np.float32)
    ref64, _ = run(np.float64)
    return ref, rsc, O.rel_l2(ref64, ref)


def _check_case3(res, bitwise):
    st = res["st"]
    n = len(res["frames"])
    for b, f in enumerate(res["frames"]):
        _, mem, sc = _single_clip(st, res["vids"][b], res["idxs"][b])
        got = res["mems"][b].flatten(0, 1)
        err = O.rel_l2(to_np(got), to_np(mem.flatten(0, 1)))
        assert tuple(res["scores"][b].shape) == (f,) == tuple(sc.shape)
        serr = O.rel_l2(to_np(res["scores"][b]), to_np(sc))
        ref, rsc, floor = _oracle_clip(st, res["host"][b], res["idxs"][b], b, n)
        oerr = O.rel_l2(to_np(got), ref)
        print(f"clip {b} ({f} frames): memory vs single-video engine {err:.2e}, frame scores {serr:.2e}; vs oracle {oerr:.2e} "
              f"(floor {floor:.2e}), scores vs oracle {O.rel_l2(to_np(res['scores'][b]), rsc):.2e}")
        assert err < ROW_BATCH_ROWS and serr < ROW_BATCH_SCORES
        if bitwise:
            assert torch.equal(got, mem.flatten(0, 1)), f"clip {b}: memory differs from the single-video engine where no unit is cut"
        assert oerr < chain_tol(floor)
        assert O.rel_l2(to_np(res["scores"][b]), rsc) < ROW_BATCH_SCORES
        assert abs(float(res["scores"][b].float().sum()) - 2 * 2) < 2e-2 * 4               # sum_f score_f = H * M


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_clips_step_vs_single_engine_and_oracle(mode):
    """clips of 4, 2 and 1 frames on an engine of 4 (n_active = 3 < B).  At S = 196 .. 784 keys no plan cuts a unit for 1 .. 4
    videos (asserted): the single video runs the plain grid too, and the memories are its bits."""
    R, H = 2 * P, 2
    for S in (P, 2 * P, 4 * P):
        for nb in (1, 2, 3, 4):
            info = _plan(R, S, H * nb)
            assert info[1] == 0 and info[3] == 1, f"S={S} nb={nb}: plan {info} cuts a unit"
    _check_case3(_case3(mode), bitwise=True)


def test_clip_of_seven_frames_where_the_single_video_splits_its_keys():
    """S = 1372: the single video splits its keys in 2 (asserted), the clip batch never does - other bits, the tolerance gates"""
    assert _plan(2 * P, 7 * P, 2)[3] == 2
    _check_case3(_case3("bf16", (7, 4, 2), 9400), bitwise=False)


# ---- 4. equal F is the existing step ------------------------------------------------------------------------------------------------------
def test_equal_frame_counts_are_the_existing_step():
    st = _setup("bf16")
    _, vids, idxs = _clips(st, (2, 2, 2), 9500)
    xs = [_pe(st, v, i) for v, i in zip(vids, idxs)]
    a, b = BatchedProjector(st.rm, 4), BatchedProjector(st.rm, 4)
    a.reset()
    va = a.step_frames(xs)
    b.reset()
    sb = b.step(xs)
    torch.cuda.synchronize()
    assert torch.equal(a.frame_scores[-1], sb) and all(torch.equal(va[i], sb[i]) for i in range(3))
    for v in range(3):
        assert torch.equal(a.memory_cache(v)[-1], b.memory_cache(v)[-1])
    assert not torch.equal(a.memory_cache(0)[-1], a.memory_cache(1)[-1])


# ---- 5. independence ------------------------------------------------------------------------------------------------------------------------
def test_clips_are_independent_and_scores_do_not_touch_the_memory():
    a, b = _case3(), _case3(alt=1)
    assert not torch.equal(a["mems"][1], b["mems"][1]) and torch.isfinite(b["mems"][1].float()).all()
    for v in (0, 2):
        assert torch.equal(a["mems"][v], b["mems"][v]), f"clip {v}: memory moved with another clip's frames"
        assert torch.equal(a["scores"][v], b["scores"][v]), f"clip {v}: frame scores moved with another clip's frames"
    # the memory does not depend on whether scores are requested, nor on the frame-score mode
    for other in (_case3(scores=False), _case3(score_mode=0), _case3(score_mode=2)):
        for v in range(3):
            assert torch.equal(a["mems"][v], other["mems"][v])
    assert torch.equal(a["padded"], _case3(score_mode=0)["padded"])
    # entries behind F[b] of a score row are not touched: the C call into a sentinel-filled [3, 7] buffer
    st, xs, frames = a["st"], a["xs"], a["frames"]
    bp = BatchedProjector(st.rm, 4)
    bp.reset()
    eng = bp.engine(xs[0].device, xs[0].dtype, 4)
    ld = 7
    sc = torch.full((3, ld), SENTINEL, device="cuda", dtype=torch.int16).view(xs[0].dtype)
    capi.check(capi.lib().mavlm_step_batch_frames(eng.ctx, (capi.vp * 3)(*[x.data_ptr() for x in xs]), _i32(frames), 3, sc.data_ptr(), ld, 0,
                                                  ops.stream_ptr()), "mavlm_step_batch_frames")
    torch.cuda.synchronize()
    got = bits(sc)
    for v, f in enumerate(frames):
        assert torch.equal(sc[v, :f], a["scores"][v]) and (got[v, f:] == SENTINEL).all(), f"clip {v}: score row"
    # the prefix never grows
    assert capi.lib().mavlm_step_batch_frames(eng.ctx, (capi.vp * 4)(*[x.data_ptr() for x in xs + xs[:1]]), _i32(list(frames) + [1]), 4,
                                              None, 0, 0, ops.stream_ptr()) == capi.E_STATE


# ---- 6. two steps with different F in each --------------------------------------------------------------------------------------------------
def test_two_steps_with_other_frame_counts_each():
    """step 0 takes F = (3, 1, 2), step 1 takes F = (2, 4): the prefix shrinks, the second step runs the evolution over memories
    formed from different frame counts.  Against single-video engines fed the same chunks and the oracle."""
    st = _setup("bf16")
    F0, F1 = (3, 1, 2), (2, 4)
    r = O.rounder(st.mode)
    host = [[r(O.hash_normal_like((f, P, st.D), 9600 + 10 * t + b)) for b, f in enumerate(F)] for t, F in enumerate((F0, F1))]
    dev = [[to_dev(x, st.mode) for x in step] for step in host]
    bp = BatchedProjector(st.rm, 4)
    bp.reset()
    s0 = [v.clone() for v in bp.step_frames(dev[0])]
    m0 = [bp.memory_cache(b)[-1].clone() for b in range(3)]
    s1 = [v.clone() for v in bp.step_frames(dev[1])]
    torch.cuda.synchronize()
    lib = capi.lib()
    assert [lib.mavlm_video_steps(bp._engine.ctx, b) for b in range(4)] == [2, 2, 1, 0]
    with pytest.raises(capi.MavlmError):
        bp.step_frames(dev[0])                                                        # three clips after a step of two
    for b in range(3):
        chunks = [dev[0][b]] + ([dev[1][b]] if b < 2 else [])
        st.rm.memory_cache = []
        n0 = len(st.rm.frame_attn_scores)
        for c in chunks:
            st.rm(c)
        torch.cuda.synchronize()
        want = [m.clone() for m in st.rm.memory_cache]
        wsc = [s.clone() for s in st.rm.frame_attn_scores[n0:]]
        mine = bp.memory_cache(b)
        assert len(mine) == len(want) == len(chunks)
        assert torch.equal(mine[0], m0[b])                                            # (the first memory stays in its ring slot)
        err = O.rel_l2(to_np(torch.cat(list(mine))), to_np(torch.cat(want)))
        got_sc = [s0[b]] + ([s1[b]] if b < 2 else [])
        serr = max(O.rel_l2(to_np(x), to_np(y)) for x, y in zip(got_sc, wsc))

        def run(acc):
            with O.accumulate_in(acc):
                orm = O.RecurrentMemory(st.cfg, st.w, st.mode)
                orm.reset()
                for t in range(len(chunks)):
                    O.ROW_BATCH = (b, 3 if t == 0 else 2)
                    try:
                        orm.step(host[t][b])
                    finally:
                        O.ROW_BATCH = (0, 1)
                return np.concatenate(orm.memory_cache, axis=0).reshape(-1, st.D), orm.frame_attn_scores
        ref, rsc = run(np.float32)
        ref64, _ = run(np.float64)
        floor = O.rel_l2(ref64, ref)
        oerr = O.rel_l2(to_np(torch.cat(list(mine)).flatten(0, 1)), ref)
        print(f"video {b}: memories vs single-video engine {err:.2e}, scores {serr:.2e}; vs oracle {oerr:.2e} (floor {floor:.2e})")
        assert err < ROW_BATCH_ROWS and serr < ROW_BATCH_SCORES and oerr < chain_tol(floor)
        assert max(O.rel_l2(to_np(x), y) for x, y in zip(got_sc, rsc)) < ROW_BATCH_SCORES


# ---- 7. the emit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wf", [True, False])
@pytest.mark.parametrize("layout", arch.LAYOUTS)
def test_clip_emit_blocks_equal_the_single_video_blocks(layout, wf):
    """the clips of case 3, handed over shortest first, emitted into a sentinel-filled buffer at rows that follow no stride: every
    block is the single-video `video_memory_tokens` block of that clip, bit for bit (no unit is cut at this shape: case 3)"""
    res = _case3()
    st = res["st"]
    caller = [2, 0, 1]
    vids, idxs = [res["vids"][i] for i in caller], [res["idxs"][i] for i in caller]
    rows = [arch.video_token_rows(v.shape[0], 2, P, wf, 32, 32, 2, layout=layout) for v in vids]
    assert len(set(rows)) == (3 if wf else 1)
    gaps, dst, at = [3, 11, 6], [0] * 3, 0
    for j in (1, 2, 0):
        at += gaps[j]
        dst[j] = at
        at += rows[j]
    out_rows = at + 5
    buf = torch.full((out_rows, st.D), SENTINEL, device="cuda", dtype=torch.int16).view(vids[0].dtype)
    nl = None if layout == "no_token" else st.nl
    _, info = arch.video_memory_tokens_clips(st.model, res["bp"], vids, idxs, st.mp, st.fp, nl, wf, out=buf, layout=layout, dst_rows=dst)
    torch.cuda.synchronize()
    assert info["block_rows"] == rows and [caller[i] for i in info["order"]] == [0, 1, 2]
    got = bits(buf)
    untouched = np.ones(out_rows, bool)
    for j, v in enumerate(caller):
        untouched[dst[j]:dst[j] + rows[j]] = False
        want, _, _ = _single_clip(st, res["vids"][v], res["idxs"][v], layout, wf)
        assert want.shape[0] == rows[j]
        assert torch.equal(buf[dst[j]:dst[j] + rows[j]], want), f"{layout} clip {v}: block differs from the single-video block"
    assert (got[untouched] == SENTINEL).all(), "rows outside the blocks were written"
    # the list form: the same blocks in the caller's order
    toks, _ = arch.video_memory_tokens_clips(st.model, res["bp"], vids, idxs, st.mp, st.fp, nl, wf, layout=layout)
    torch.cuda.synchronize()
    for j in range(3):
        assert torch.equal(toks[j], buf[dst[j]:dst[j] + rows[j]])


def test_clip_emit_refusals_on_a_stepped_context():
    res = _case3()
    st, bp = res["st"], res["bp"]
    bp.reset()
    bp.step_frames(res["xs"])
    eng = bp._engine
    frames = list(res["frames"])
    rows = [arch.video_token_rows(f, 2, P, True, 32, 32, 2, layout="grid") for f in frames]
    assert rows[0] > rows[1] > rows[2]
    total = sum(rows)
    buf = torch.full((total + 4, st.D), SENTINEL, device="cuda", dtype=torch.int16).view(res["vids"][0].dtype)
    xp = (capi.vp * 3)(*[x.data_ptr() for x in res["xs"]])
    fine = torch.zeros((3, 4), dtype=torch.long)
    for b, f in enumerate(frames):
        fine[b, :f] = arch.fine_frame_indices(f, 32)
    fine = fine.cuda()
    out = (ctypes.c_int64 * 3)()

    def emit(dst, out_rows=total + 4):
        rc = capi.lib().mavlm_fuse_emit_layout_frames_to(eng.ctx, 3, xp, fine.data_ptr(), 4, _i32(frames), st.mp.data_ptr(), 10,
                                                         st.fp.data_ptr(), 9, st.nl.data_ptr(), 1, capi.LAYOUTS["grid"], buf.data_ptr(),
                                                         out_rows, _i64(dst), out, ops.stream_ptr())
        torch.cuda.synchronize()
        return rc

    assert emit([rows[2], 0, rows[1] + rows[2]]) == capi.E_ARG           # clip 1 at row 0 runs into clip 0 (its OWN length counts)
    assert emit([0, rows[0] - 1, rows[0] + rows[1]]) == capi.E_ARG         # clip 0 runs into clip 1
    assert emit([0, rows[0], rows[0] + rows[1] + 5]) == capi.E_ARG         # a block past out_rows
    assert emit([0, rows[0], rows[0] + rows[1]], out_rows=total - 1) == capi.E_ARG
    assert (bits(buf) == SENTINEL).all(), "something was written before a refusal"
    assert emit([rows[2] + 1, rows[2] + 1 + rows[0], 0]) == 0 and list(out) == rows      # the shortest block first


# ---- 8. wide heads ------------------------------------------------------------------------------------------------------------------------
def test_clips_wide_heads():
    """D = 3584 (8 heads of 448), M = 1, clips of 1 and 3 frames on an engine of 2: one plain-grid launch of the wide forward per
    video, the per-video column sums; the stacked GEMMs around them.  Against the single-video engine."""
    from test_gpu_path import make_projector
    cfg = O.PathConfig(hidden=3584, heads=8, mem_tokens=1, depth=2)
    proj = make_projector(cfg, O.make_weights(cfg, seed=77))
    segs = [to_dev(O.bf16_round(O.hash_normal_like((f, P, 3584), 9800 + b))) for b, f in enumerate((3, 1))]
    bp = BatchedProjector(proj, 2)
    bp.reset()
    views = bp.step_frames(segs)
    torch.cuda.synchronize()
    for b, seg in enumerate(segs):
        proj.memory_cache = []
        cache, scores = proj(seg)
        torch.cuda.synchronize()
        err = O.rel_l2(to_np(bp.memory_cache(b)[-1]), to_np(cache[-1]))
        serr = O.rel_l2(to_np(views[b]), to_np(scores[-1]))
        print(f"wide heads, clip {b} ({seg.shape[0]} frames): memory vs single-video engine {err:.2e}, frame scores {serr:.2e}")
        assert tuple(views[b].shape) == (seg.shape[0],)
        assert err < ROW_BATCH_ROWS and serr < ROW_BATCH_SCORES
        assert abs(float(views[b].float().sum()) - 8) < 2e-2 * 8                           # sum_f score_f = H * M


# ---- 9. the entry point -----------------------------------------------------------------------------------------------------------------------
FRAMES9 = [9, 5, 5, 3]                        # clips 0, 1, 2 one group on the engine of 4 (2 * 5 >= 9); 2 * 3 < 9: video 3 runs alone


@pytest.mark.parametrize("side", ["right", "left"])
def test_entry_point_clip_group(side):
    from test_gpu_video_batch import _host as lm_host, _video, _samples, _call, _pad_together, PROMPTS5, IMG
    lm, model, hf, _, _ = lm_host()
    hf.tokenizer_padding_side = side
    rm = model.recurrent_memory_transformer
    prompts = PROMPTS5[:4]
    videos = [_video(f, v) for v, f in enumerate(FRAMES9)]
    assert arch.plan_clip_batches(FRAMES9) == ([(4, [0, 1, 2])], [3])
    ids, mask, labels, pos = _samples(prompts)
    lib = capi.lib()
    singles = []
    for s in range(4):
        n = len(prompts[s])
        one = _call(lm, ids[s:s + 1, :n], mask[s:s + 1, :n], labels[s:s + 1, :n], pos[s:s + 1, :n], [videos[s]])
        singles.append(tuple(t.clone() if torch.is_tensor(t) else t for t in one))
    off = _call(lm, ids, mask, labels, pos, videos)
    off = tuple(t.clone() if torch.is_tensor(t) else t for t in off)
    lm.enable_clip_row_batches()
    out = _call(lm, ids, mask, labels, pos, videos)
    torch.cuda.synchronize()
    eng4 = rm.row_batcher(4)._engine
    assert lib.mavlm_steps(eng4.ctx) == 1 and [lib.mavlm_video_steps(eng4.ctx, b) for b in range(4)] == [1, 1, 1, 0]
    w_emb, w_lab, w_mask, w_pos, starts = _pad_together(singles, side == "left")
    assert torch.equal(out[5], w_lab) and torch.equal(out[2], w_mask) and torch.equal(out[1], w_pos)
    emb = out[4]
    assert emb.shape == w_emb.shape and emb.dtype == w_emb.dtype
    same = torch.ones(emb.shape[:2], dtype=torch.bool, device="cuda")
    for v in range(3):
        p = prompts[v].index(IMG)
        mem = slice(starts[v] + p + 10, starts[v] + p + 10 + 2 * P)
        err = O.rel_l2(to_np(emb[v, mem]), to_np(w_emb[v, mem]))
        plain = _plan(2 * P, FRAMES9[v] * P, 8)                      # does the single video cut a unit at its key count?
        print(f"{side} clip {v} ({FRAMES9[v]} frames): fused memory rows, clip batch vs single-sample call rel-L2 {err:.3e}; "
              f"single-video plan {plain}")
        assert err < ROW_BATCH_ROWS
        if not (plain[1] == 0 and plain[3] == 1):
            same[v, mem] = False                                     # (another schedule on the single video: the tolerance gate only)
    assert torch.equal(emb[same], w_emb[same]), "text / prompt / newline / fine-frame rows, uncut memory rows or the single's block differ"
    again = _call(lm, ids, mask, labels, pos, videos)
    assert torch.equal(again[4], emb) and torch.equal(again[5], out[5])
    lm.enable_clip_row_batches(False)
    back = _call(lm, ids, mask, labels, pos, videos)
    torch.cuda.synchronize()
    assert torch.equal(back[4], off[4]) and torch.equal(back[5], off[5]) and torch.equal(back[2], off[2])
