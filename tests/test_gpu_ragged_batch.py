"""-m gpu: ragged row batches - a row-batched context that steps a shrinking PREFIX of its videos (`mavlm_step_batch_active`),
the per-video step counts (`mavlm_video_steps`), the ragged emit (`mavlm_fuse_emit_layout_ragged_to`) and the entry-point switch
(`enable_ragged_row_batches`).  Through the C ABI like the other row-batch tests.

Default shape: D = 256 (2 heads of 128), M = 2, P = 196, chunks of 4 frames (784 keys), FIFO of 2 - the longest video wraps it.
Gates: `tests/test_gpu_batch.py` compares a row batch with the single-video engine under rel-L2 < 6e-3 (fused rows,
test_row_batch_checkpoint_shape_vs_oracle) and < 5e-3 (frame scores); those two figures are literals inside that file's test
bodies and are restated here as ROW_BATCH_ROWS / ROW_BATCH_SCORES, its TOL and `chain_tol` are imported."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd import _ops as ops
from memory_augmented_vlm_amd.model import llava_arch as arch
from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
from oracle import memory_path as O
from gpu_util import to_dev, to_np
from test_gpu_batch import _host, _prompts, TOL
from test_gpu_layouts import SENTINEL, bits
from test_gpu_path import chain_tol
from test_gpu_attention_maps import TOL as MAPS_TOL

pytestmark = pytest.mark.gpu
ROW_BATCH_ROWS, ROW_BATCH_SCORES = 6e-3, 5e-3           # tests/test_gpu_batch.py (see the module docstring)
P, CHUNK, CAP, FINE = 196, 4, 2, 3


@pytest.fixture(autouse=True)
def _inference_path():
    with torch.no_grad():
        yield


@functools.lru_cache(maxsize=None)
def _setup(mode="bf16", hidden=256, heads=2, M=2, seed=71):
    cfg = O.PathConfig(hidden=hidden, heads=heads, mem_tokens=M, depth=2, cache_cap=CAP, chunk=CHUNK, fine_frames=FINE)
    w = O.make_weights(cfg, seed=seed)
    model = _host(cfg, w, mode, cap=CAP)
    mp, fp = _prompts(hidden, mode)
    return types.SimpleNamespace(cfg=cfg, w=w, model=model, rm=model.recurrent_memory_transformer, mp=mp, fp=fp, mode=mode,
                                 D=hidden, nl=model.image_newline.detach())


def _videos(st, chunks, seed, amp=1.0):
    """(host arrays on the 16-bit grid, device tensors, frame indices) of videos of `chunks` chunks each"""
    r = O.rounder(st.mode)
    xs = [r(O.hash_normal_like((c * CHUNK, P, st.D), seed + b) + amp * O.hash_normal_like((c * CHUNK, 1, st.D), seed + 50 + b))
          for b, c in enumerate(chunks)]
    return xs, [to_dev(x, st.mode) for x in xs], [torch.arange(c * CHUNK) * 2 + b for b, c in enumerate(chunks)]


def _pe(st, vid, idx):
    return st.model.positional_encoding(vid, arch._device_indices(idx, vid.device), indices_checked=True)


def _run_prefix(st, bp, xs, chunks, record=False, after_step=None):
    """steps the videos (PE-added frames `xs`, longest first) on `bp` as a shrinking prefix; returns per step
    (n_active, scores clone, [newest memory clone per active video])"""
    bp.record_attention_maps = record
    bp.reset()
    out = []
    for i in range(chunks[0]):
        segs = [x[i * CHUNK:(i + 1) * CHUNK] for x, c in zip(xs, chunks) if c > i]
        sc = bp.step(segs)
        out.append((len(segs), sc.clone(), [bp.memory_cache(b)[-1].clone() for b in range(len(segs))]))
        if after_step is not None:
            after_step(i, len(segs))
    torch.cuda.synchronize()
    return out


def _single(st, vid, idx, layout="one_token", with_frames=True, record=False):
    """the single-video engine on one video: (block, memories, frame scores, attention maps, info)"""
    rm = st.rm
    rm.record_attention_maps = record
    n0 = len(rm.frame_attn_scores)
    tok, info = arch.video_memory_tokens(st.model, vid, idx, st.mp, st.fp, st.nl, with_frames, chunk=CHUNK, fine_frames=FINE,
                                         layout=layout)
    torch.cuda.synchronize()
    maps = list(rm.attention_maps) if record else []
    rm.record_attention_maps = False
    return tok.clone(), [m.clone() for m in rm.memory_cache], [s.clone() for s in rm.frame_attn_scores[n0:]], maps, info


# ---- 1. a constant prefix is the smaller engine, bit for bit (the launch contract) ----------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("B,k", [(4, 3), (8, 2)])
def test_constant_prefix_equals_the_smaller_engine(B, k, mode):
    st = _setup(mode)
    chunks = [4] * k
    _, vids, idxs = _videos(st, chunks, 7100)
    xs = [_pe(st, v, i) for v, i in zip(vids, idxs)]
    big, small = BatchedProjector(st.rm, B), BatchedProjector(st.rm, k)
    a = _run_prefix(st, big, xs, chunks)
    b = _run_prefix(st, small, xs, chunks)
    lib = capi.lib()
    assert lib.mavlm_steps(big._engine.ctx) == 4
    assert [lib.mavlm_video_steps(big._engine.ctx, v) for v in range(B)] == [4] * k + [0] * (B - k)
    for t, ((na, sa, ma), (nb, sb, mb)) in enumerate(zip(a, b)):
        assert na == nb == k and tuple(sa.shape) == (k, CHUNK)
        assert torch.equal(sa, sb), f"step {t}: frame scores"
        for v in range(k):
            assert torch.equal(ma[v], mb[v]), f"step {t} video {v}: memory"
    for v in range(k):
        for x, y in zip(big.memory_cache(v), small.memory_cache(v)):
            assert torch.equal(x, y)
    assert not torch.equal(big.memory_cache(0)[-1], big.memory_cache(1)[-1])
    for layout in ("one_token", "grid"):
        want, _ = arch.video_memory_tokens_batched(st.model, small, vids, idxs, st.mp, st.fp, st.nl, chunk=CHUNK, fine_frames=FINE,
                                                   layout=layout)
        got, info = arch.video_memory_tokens_batched(st.model, big, vids, idxs, st.mp, st.fp, st.nl, chunk=CHUNK, fine_frames=FINE,
                                                     layout=layout, ragged=True)
        torch.cuda.synchronize()
        assert info["order"] == list(range(k))
        for v in range(k):
            assert torch.equal(got[v], want[v]), f"{layout} video {v}: block"
    # the prefix never grows, and a full step after a smaller one is refused too: nothing is enqueued (the ring keeps its bits)
    keep = big._engine.mem_ring.view(torch.int16).clone()        # (raw bits: the rows of the unused videos were never written)
    segs = [x[:CHUNK] for x in xs] + [xs[0][:CHUNK]] * (B - k)
    ptrs = (capi.vp * B)(*[s.data_ptr() for s in segs])
    if k + 1 <= B:
        assert lib.mavlm_step_batch_active(big._engine.ctx, ptrs, k + 1, CHUNK, None, 0, ops.stream_ptr()) == capi.E_STATE
    assert lib.mavlm_step_batch(big._engine.ctx, ptrs, CHUNK, None, 0, ops.stream_ptr()) == capi.E_STATE
    with pytest.raises(capi.MavlmError):
        big.step(segs[:k + 1])
    torch.cuda.synchronize()
    assert torch.equal(big._engine.mem_ring.view(torch.int16), keep) and lib.mavlm_steps(big._engine.ctx) == 4


# ---- 2. the shrinking prefix ----------------------------------------------------------------------------------------------------------
CHUNKS2 = [4, 2, 1]                      # n_active = 3, 2, 1, 1


@functools.lru_cache(maxsize=None)
def _case2(mode="bf16", hidden=256, heads=2, chunks=tuple(CHUNKS2), seed=7200, alt=False):
    """the run of case 2 (shared by the cases that read it): the ragged batch on an engine of 4 with the attention maps recorded,
    ring snapshots, and each video on the single-video engine.  `alt`: the shortest video holds other frames with rows of 1e4."""
    st = _setup(mode, hidden, heads)
    chunks = list(chunks)
    host, vids, idxs = _videos(st, chunks, seed)
    if alt:
        x = np.array(O.rounder(st.mode)(O.hash_normal_like(host[-1].shape, seed + 900)))
        x[0, :7] = 1e4
        x[-1, 100:103] = -1e4
        host[-1], vids[-1] = x, to_dev(x, st.mode)
    xs = [_pe(st, v, i) for v, i in zip(vids, idxs)]
    bp = BatchedProjector(st.rm, 4)
    snaps = {}

    def after(i, n):
        if i == chunks[-1] - 1:          # right after the shortest video's last step: its rows in every slot and in evo_kv_ring
            torch.cuda.synchronize()
            snaps["ring"] = bp._engine.mem_ring[:, len(chunks) - 1].clone()
            snaps["evo"] = bp._engine.evo_kv[len(chunks) - 1].clone()

    steps = _run_prefix(st, bp, xs, chunks, record=True, after_step=after)
    maps = list(bp.attention_maps)
    bp.record_attention_maps = False
    eng = bp._engine
    lib = capi.lib()
    res = types.SimpleNamespace(st=st, chunks=chunks, host=host, vids=vids, idxs=idxs, xs=xs, bp=bp, steps=steps, maps=maps,
                                snaps=snaps, ring_end=eng.mem_ring[:, len(chunks) - 1].clone(),
                                evo_end=eng.evo_kv[len(chunks) - 1].clone(),
                                vsteps=[lib.mavlm_video_steps(eng.ctx, b) for b in range(4)], ctx_steps=lib.mavlm_steps(eng.ctx),
                                mems=[[m.clone() for m in bp.memory_cache(b)] for b in range(len(chunks))])
    return res


def _scores_of(res, b):
    return [sc[b] for n, sc, _ in res.steps if n > b]


def _check_vs_single_and_oracle(res, bitwise=False, oracle=True):
    st, chunks = res.st, res.chunks
    assert [n for n, _, _ in res.steps] == [sum(c > i for c in chunks) for i in range(chunks[0])]
    assert res.vsteps == chunks + [0] * (4 - len(chunks)) and res.ctx_steps == chunks[0]
    for b, c in enumerate(chunks):
        tok, mems, scores, smaps, _ = _single(st, res.vids[b], res.idxs[b], record=(b == 0))
        assert len(res.mems[b]) == len(mems) == min(c, CAP) and len(_scores_of(res, b)) == len(scores) == c
        got, want = torch.cat(res.mems[b]).flatten(0, 1), torch.cat(mems).flatten(0, 1)
        err = O.rel_l2(to_np(got), to_np(want))
        serr = max(O.rel_l2(to_np(x), to_np(y)) for x, y in zip(_scores_of(res, b), scores))
        print(f"video {b} ({c} chunks): memories vs single-video engine {err:.2e}, frame scores {serr:.2e}")
        assert err < ROW_BATCH_ROWS and serr < ROW_BATCH_SCORES
        if bitwise:
            assert torch.equal(got, want), f"video {b}: memories differ from the single-video engine where no unit is cut"
        if b == 0 and smaps:
            # attention maps: active videos only; the first step (same inputs on both engines) under the step-map gate
            for (n, _, _), am in zip(res.steps, res.maps):
                assert am.formation.shape[0] == n and (am.evolution is None or am.evolution.shape[0] == n)
                assert float((am.formation.double().sum(-1) - P).abs().max() / P) < 1e-3
            merr = O.rel_l2(to_np(res.maps[0].formation[0]), to_np(smaps[0].formation))
            print(f"video 0, first step: attention maps vs single-video engine {merr:.2e}")
            assert merr < MAPS_TOL
        if not oracle:
            continue
        # the oracle in emulation mode, its schedule mirrored per step (video b of the n videos active in that step)
        def run(acc):
            with O.accumulate_in(acc):
                xp = O.pe_add(res.host[b], res.idxs[b].numpy(), st.w["positional_encoding.frame_embed"], st.mode)
                rm = O.RecurrentMemory(st.cfg, st.w, st.mode)
                rm.reset()
                for i in range(c):
                    O.ROW_BATCH = (b, res.steps[i][0])
                    try:
                        rm.step(xp[i * CHUNK:(i + 1) * CHUNK])
                    finally:
                        O.ROW_BATCH = (0, 1)
                return np.concatenate(rm.memory_cache, axis=0).reshape(-1, st.D), rm.frame_attn_scores
        ref, rsc = run(np.float32)
        ref64, _ = run(np.float64)
        floor = O.rel_l2(ref64, ref)
        oerr = O.rel_l2(to_np(got), ref)
        print(f"video {b}: memories vs oracle {oerr:.2e} (floor {floor:.2e})")
        assert oerr < chain_tol(floor)
        assert max(O.rel_l2(to_np(x), y) for x, y in zip(_scores_of(res, b), rsc)) < ROW_BATCH_SCORES


def test_shrinking_prefix_vs_single_engine_and_oracle():
    _check_vs_single_and_oracle(_case2())


def test_shrinking_prefix_bitwise_where_no_unit_is_cut():
    """D = 256, M = 2: R = 392 query rows, 784 chunk keys, at most 2 x 392 evolution keys.  The precondition - no attention plan
    involved cuts a unit (no stream-K, no split-KV) at 1, 2 and 3 videos and on the single video - is asserted through
    mavlm_attention_plan; there the schedules coincide and the memories equal the single-video engine's bit for bit."""
    info = (capi.i32 * 4)()
    R, H = 2 * P, 2
    for S in (CHUNK * P, R, 2 * R):
        for nb in (1, 2, 3):
            capi.check(capi.lib().mavlm_attention_plan(R, S, H * nb, info), "plan")
            assert info[1] == 0 and (nb > 1 or info[3] <= 1), f"S={S} nb={nb}: plan {list(info)} cuts a unit"
    _check_vs_single_and_oracle(_case2(), bitwise=True, oracle=False)


# ---- 3. nothing leaks between videos; finished rows are left alone ---------------------------------------------------------------------
def test_no_leak_between_videos_and_finished_rows_stay():
    a, b = _case2(), _case2(alt=True)
    for r in (a, b):
        # (raw bits: rows of slots the video never wrote are whatever the allocation held, NaN patterns included)
        assert (bits(r.snaps["ring"]) == bits(r.ring_end)).all(), "the finished video's ring rows changed after its last step"
        assert (bits(r.snaps["evo"]) == bits(r.evo_end)).all(), "the finished video's evolution K/V rows changed after its last step"
    assert not torch.equal(a.mems[2][0], b.mems[2][0])
    assert torch.isfinite(b.mems[2][0].float()).all()
    for v in (0, 1):
        for x, y in zip(a.mems[v], b.mems[v]):
            assert torch.equal(x, y), f"video {v}: memory moved with another video's frames"
        for x, y in zip(_scores_of(a, v), _scores_of(b, v)):
            assert torch.equal(x, y), f"video {v}: frame scores moved with another video's frames"
    blocks = []
    for r in (a, b):
        toks, _ = arch.video_memory_tokens_batched(r.st.model, r.bp, r.vids, r.idxs, r.st.mp, r.st.fp, r.st.nl, chunk=CHUNK,
                                                   fine_frames=FINE, layout="grid", ragged=True)
        torch.cuda.synchronize()
        blocks.append([t.clone() for t in toks])
    for v in (0, 1):
        assert torch.equal(blocks[0][v], blocks[1][v]), f"video {v}: block moved with another video's frames"
    assert not torch.equal(blocks[0][2], blocks[1][2])


# ---- 4. the ragged emit -----------------------------------------------------------------------------------------------------------------
def _emit_case(res, layout, wf, caller_order, tile=0):
    """the ragged emit of the case-2 videos (handed over in `caller_order`) into a sentinel-filled buffer at rows that follow no
    stride, against the single-video engine fed the same ring memories.  `tile`: the GEMM tile hook, set around the whole ragged
    call (which steps the videos again: a forced tile also takes the split contractions out of the steps, so the ring memories
    compared are those of THIS call, read back from the engine) and around the single-video emit it is compared with."""
    st = res.st
    k = len(res.chunks)
    vids, idxs = [res.vids[i] for i in caller_order], [res.idxs[i] for i in caller_order]
    rows = [arch.video_token_rows(v.shape[0], 2, P, wf, CHUNK, FINE, CAP, layout=layout) for v in vids]
    gaps = [3, 11, 6]
    dst, at = [0] * k, 0
    for j in (2, 0, 1):                          # blocks in another order than the videos, unequal gaps
        at += gaps[j]
        dst[j] = at
        at += rows[j]
    out_rows = at + 5
    buf = torch.full((out_rows, st.D), SENTINEL, device="cuda", dtype=torch.int16).view(vids[0].dtype)
    lib = capi.lib()
    capi.check(lib.mavlm_set_gemm_tile(tile), "tile")
    try:
        _, info = arch.video_memory_tokens_batched(st.model, res.bp, vids, idxs, st.mp, st.fp, st.nl, wf, chunk=CHUNK,
                                                   fine_frames=FINE, out=buf, layout=layout, dst_rows=dst, ragged=True)
        torch.cuda.synchronize()
    finally:
        lib.mavlm_set_gemm_tile(0)
    assert info["block_rows"] == rows and [caller_order[i] for i in info["order"]] == [0, 1, 2]
    ring = [[m.clone() for m in res.bp.memory_cache(v)] for v in range(k)]       # (the engine's order is the videos' own: longest first)
    assert [len(r) for r in ring] == [min(c, CAP) for c in res.chunks]
    got = bits(buf)
    untouched = np.ones(out_rows, bool)
    for j, v in enumerate(caller_order):
        untouched[dst[j]:dst[j] + rows[j]] = False
        blk = buf[dst[j]:dst[j] + rows[j]]
        assert not (got[dst[j]:dst[j] + rows[j]] == SENTINEL).all(axis=1).any(), f"video {v}: a row of the block was never written"
        # the single-video engine fed this video's ring memories: its own steps, then its ring overwritten with the batch's rows
        tok, mems, _, _, sinfo = _single(st, res.vids[v], res.idxs[v], layout, wf)
        assert len(st.rm.memory_cache) == len(ring[v])
        for m_single, m_batch in zip(st.rm.memory_cache, ring[v]):
            m_single.copy_(m_batch)
        eng = st.rm.engine(blk.device, blk.dtype)
        n_fine = sinfo["fine_idx"].numel()
        want = torch.empty_like(tok)
        w = ctypes.c_int64(0)
        capi.check(lib.mavlm_set_gemm_tile(tile), "tile")
        try:
            rc = lib.mavlm_fuse_emit_layout(eng.ctx, sinfo["pe_frames"].data_ptr(),
                                            arch._device_indices(sinfo["fine_idx"], blk.device).data_ptr(), n_fine, st.mp.data_ptr(), 10,
                                            st.fp.data_ptr(), 9, None if layout == "no_token" else st.nl.data_ptr(), 1 if wf else 0,
                                            capi.LAYOUTS[layout], want.data_ptr(), want.shape[0], ctypes.byref(w), ops.stream_ptr())
            torch.cuda.synchronize()
        finally:
            lib.mavlm_set_gemm_tile(0)
        capi.check(rc, "mavlm_fuse_emit_layout")
        assert w.value == rows[j] == tok.shape[0]
        a, b_ = sinfo["memory_rows"]
        period = arch.layout_period(layout, P)
        feat = torch.ones(rows[j], dtype=torch.bool, device="cuda")
        feat[:a] = False
        feat[b_:] = False
        if period:
            feat[a + period:b_:period + 1] = False                # the newlines inside the memory block
        err = O.rel_l2(to_np(blk[feat]), to_np(want[feat]))
        assert err < ROW_BATCH_ROWS, (layout, wf, v, err)
        # (no unit is cut at this shape, test_shrinking_prefix_bitwise_where_no_unit_is_cut: the fused rows are the same bits)
        assert torch.equal(blk[feat], want[feat]), f"{layout} video {v}: fused rows differ from the single-video emit"
        assert torch.equal(blk[~feat], want[~feat]), f"{layout} video {v}: prompt / newline / fine-frame rows differ"
        assert torch.equal(blk[~feat], tok[~feat])
    assert (got[untouched] == SENTINEL).all(), "rows outside the blocks were written"


@pytest.mark.parametrize("wf", [True, False])
@pytest.mark.parametrize("layout", arch.LAYOUTS)
def test_ragged_emit_blocks(layout, wf):
    _emit_case(_case2(), layout, wf, [1, 2, 0])


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("tile", [256, 257, 129])
def test_ragged_emit_writer_routes(tile, mode):
    """the fuser's second GEMM of a ragged emit always carries the row map (a row-batched output): the 256-row kernel, the
    persistent kernel's map on a small grid (forced, as the layout tests do) and the 128 x 256 kernel; two blocks' form in both
    dtypes.  (The scratch + spread_rows route belongs to single-video contexts: a ragged emit never reaches it.)"""
    _emit_case(_case2(mode), "grid", True, [2, 0, 1], tile)


def test_ragged_emit_refusals_on_a_stepped_context():
    res = _case2()
    st, eng = res.st, res.bp._engine
    rows = [arch.video_token_rows(c * CHUNK, 2, P, True, CHUNK, FINE, CAP, layout="grid") for c in res.chunks]
    assert rows[0] == rows[1] > rows[2]
    total = sum(rows)
    buf = torch.full((total + 4, st.D), SENTINEL, device="cuda", dtype=torch.int16).view(res.vids[0].dtype)
    xp = (capi.vp * 3)(*[x.data_ptr() for x in res.xs])
    fine = arch._device_indices(torch.cat([arch.fine_frame_indices(c * CHUNK, FINE) for c in res.chunks]), "cuda")
    out = (ctypes.c_int64 * 3)()

    def emit(dst, out_rows=total + 4, n=3):
        rc = capi.lib().mavlm_fuse_emit_layout_ragged_to(eng.ctx, n, xp, fine.data_ptr(), FINE, st.mp.data_ptr(), 10, st.fp.data_ptr(),
                                                         9, st.nl.data_ptr(), 1, capi.LAYOUTS["grid"], buf.data_ptr(), out_rows,
                                                         (ctypes.c_int64 * len(dst))(*dst), out, ops.stream_ptr())
        torch.cuda.synchronize()
        return rc

    # the shortest block is shorter: a destination that is fine for IT overlaps when a longer block is put there
    assert emit([0, rows[0], rows[0] + rows[1] - 1]) == capi.E_ARG
    assert emit([rows[2], 0, rows[0] + rows[2]]) == capi.E_ARG                 # video 1 at 0 runs into video 0 (its own length counts)
    assert emit([0, rows[0], rows[0] + rows[1] + 5]) == capi.E_ARG             # past the end
    assert (bits(buf) == SENTINEL).all(), "something was written before a refusal"
    assert emit([rows[2] + 1, rows[2] + 1 + rows[0], 0]) == 0 and list(out) == rows       # video 2's short block first
    # the equal-length exports refuse a context whose videos hold different numbers of steps
    r = ctypes.c_int64(0)
    rc = capi.lib().mavlm_fuse_emit_layout_batch(eng.ctx, (capi.vp * 4)(*([res.xs[0].data_ptr()] * 4)), fine.data_ptr(), FINE,
                                                 st.mp.data_ptr(), 10, st.fp.data_ptr(), 9, st.nl.data_ptr(), 1, capi.LAYOUTS["grid"],
                                                 buf.data_ptr(), rows[0], ctypes.byref(r), ops.stream_ptr())
    assert rc == capi.E_STATE


# ---- 5. wide heads ----------------------------------------------------------------------------------------------------------------------
def test_shrinking_prefix_wide_heads():
    """2 heads of 448 (D = 896), lengths 3, 2 and 1: the per-video attention launches of attention_hd.hip over the active prefix"""
    _check_vs_single_and_oracle(_case2("bf16", 896, 2, (3, 2, 1), 7500))


# ---- 6. the checkpoint shape --------------------------------------------------------------------------------------------------------------
def test_checkpoint_shape_three_videos_on_an_engine_of_four():
    """D = 1024, 8 heads, M = 8, chunks of 32: videos of 96, 64 and 64 frames on the size-4 engine, blocks in one_token"""
    cfg = O.PathConfig(hidden=1024, heads=8, mem_tokens=8, depth=2)
    model = _host(cfg, O.make_weights(cfg, seed=62), "bf16")
    rm = model.recurrent_memory_transformer
    mp, fp = _prompts(1024)
    lens = [64, 96, 64]
    vids = [to_dev(O.bf16_round(O.hash_normal_like((t, P, 1024), 7600 + b))) for b, t in enumerate(lens)]
    idxs = [torch.arange(t) + b for b, t in enumerate(lens)]
    bp = rm.row_batcher(4)
    toks, info = arch.video_memory_tokens_batched(model, bp, vids, idxs, mp, fp, model.image_newline, ragged=True)
    torch.cuda.synchronize()
    assert info["order"] == [1, 0, 2] and info["num_memories"] == [2, 3, 2]
    lib = capi.lib()
    assert [lib.mavlm_video_steps(bp._engine.ctx, b) for b in range(4)] == [3, 2, 2, 0]
    toks = [t.clone() for t in toks]
    for b in range(3):
        n0 = len(rm.frame_attn_scores)
        single, sinfo = arch.video_memory_tokens(model, vids[b], idxs[b], mp, fp, model.image_newline)
        a, b_ = sinfo["memory_rows"]
        assert toks[b].shape == single.shape
        err = O.rel_l2(to_np(toks[b][a:b_]), to_np(single[a:b_]))
        print(f"checkpoint shape, video {b} ({lens[b]} frames): fused rows vs single-video engine {err:.2e}")
        assert err < ROW_BATCH_ROWS
        assert torch.equal(toks[b][:a], single[:a]) and torch.equal(toks[b][b_:], single[b_:])
        pos = info["order"].index(b)
        mine = [sc[pos] for sc in info["frame_scores"] if sc.shape[0] > pos]
        assert len(mine) == lens[b] // 32
        for x, y in zip(mine, rm.frame_attn_scores[n0:]):
            assert O.rel_l2(to_np(x), to_np(y)) < ROW_BATCH_SCORES


# ---- 7. the entry point -------------------------------------------------------------------------------------------------------------------
FRAMES7 = [40, 100, 70, 130, 20]               # sampled 64, 96, 64, 128, 20: videos 0-3 one ragged group of four, video 4 a single


@pytest.mark.parametrize("side", ["right", "left"])
def test_entry_point_ragged_group(side):
    from test_gpu_video_batch import _host as lm_host, _video, _samples, _call, _pad_together, PROMPTS5, IMG
    lm, model, hf, _, _ = lm_host()
    hf.tokenizer_padding_side = side
    rm = model.recurrent_memory_transformer
    videos = [_video(f, v) for v, f in enumerate(FRAMES7)]
    assert [arch.sample_frame_count(f) for f in FRAMES7] == [64, 96, 64, 128, 20]
    ids, mask, labels, pos = _samples(PROMPTS5)
    lib = capi.lib()
    singles = []
    for s in range(5):
        n = len(PROMPTS5[s])
        one = _call(lm, ids[s:s + 1, :n], mask[s:s + 1, :n], labels[s:s + 1, :n], pos[s:s + 1, :n], [videos[s]])
        singles.append(tuple(t.clone() if torch.is_tensor(t) else t for t in one))
    off = _call(lm, ids, mask, labels, pos, videos)
    off = tuple(t.clone() if torch.is_tensor(t) else t for t in off)
    lm.enable_ragged_row_batches()
    out = _call(lm, ids, mask, labels, pos, videos)
    torch.cuda.synchronize()
    eng4 = rm.row_batcher(4)._engine
    assert lib.mavlm_steps(eng4.ctx) == 4
    assert [lib.mavlm_video_steps(eng4.ctx, b) for b in range(4)] == [4, 3, 2, 2]          # videos 3, 1, 0, 2
    own = rm.engine(out[4].device, out[4].dtype)
    assert lib.mavlm_steps(own.ctx) == 1                                                   # only video 4 (20 frames: one chunk)
    assert set(rm.__dict__["_row_batchers"]) <= {2, 4}
    w_emb, w_lab, w_mask, w_pos, starts = _pad_together(singles, side == "left")
    assert torch.equal(out[5], w_lab) and torch.equal(out[2], w_mask) and torch.equal(out[1], w_pos)
    emb = out[4]
    assert emb.shape == w_emb.shape and emb.dtype == w_emb.dtype
    same = torch.ones(emb.shape[:2], dtype=torch.bool, device="cuda")
    for v in range(4):
        p = PROMPTS5[v].index(IMG)
        n = arch.sample_frame_count(FRAMES7[v]) // 32
        mem = slice(starts[v] + p + 10, starts[v] + p + 10 + n * 2 * P)
        same[v, mem] = False
        err = O.rel_l2(to_np(emb[v, mem]), to_np(w_emb[v, mem]))
        print(f"{side} video {v}: fused memory rows, ragged row batch vs single-sample call rel-L2 {err:.3e}")
        assert err < ROW_BATCH_ROWS                                    # (the bound of tests/test_gpu_video_batch.py for this comparison)
    assert torch.equal(emb[same], w_emb[same]), "text / prompt / newline / fine-frame rows or the single video's block differ"
    again = _call(lm, ids, mask, labels, pos, videos)
    assert torch.equal(again[4], emb) and torch.equal(again[5], out[5])
    lm.enable_ragged_row_batches(False)
    back = _call(lm, ids, mask, labels, pos, videos)
    torch.cuda.synchronize()
    assert torch.equal(back[4], off[4]) and torch.equal(back[5], off[5]) and torch.equal(back[2], off[2])
