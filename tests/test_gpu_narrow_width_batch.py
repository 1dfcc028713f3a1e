"""-m gpu: row-batched token emits at hidden sizes that are multiples of 128 but not of 256 (896 = LLaVA-OneVision-0.5B; 384 and
128 as the smallest shapes).  There the fuser's second GEMM has N = hidden, which the 256-column-tile kernels do not take: it
scatters its rows through the row-mapped form of the 128 x 128 kernel (gemm.hip: row batch, per-video bases, newline gap).

Reference of every block: the single-video engine whose ring was overwritten with the batch's memory rows, then
`mavlm_fuse_emit_layout` - the method of tests/test_gpu_ragged_batch.py::_emit_case.  With `mavlm_set_gemm_tile(128)` around both
calls no contraction splits and both sides run the 128 x 128 kernel on the same tiles: every row is bit-identical.  Without the
hook the literal rows are bit-identical and the fused rows stay under ROW_BATCH_ROWS = 6e-3 rel-L2, the project's gate for a row
batch against the single-video engine (tests/test_gpu_batch.py)."""
import ctypes
import functools
import itertools
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
from gpu_util import to_np
from test_gpu_layouts import SENTINEL, bits, frames, make_host, prompts
import test_gpu_video_batch as vb
from test_gpu_video_batch import _emit, _scattered, _pad_together
from test_gpu_ragged_batch import _case2, _emit_case, ROW_BATCH_ROWS

pytestmark = pytest.mark.gpu
P = 196
IMG = arch.IMAGE_TOKEN_INDEX
MARGIN = 4                 # sentinel rows behind every block of the constant-stride export


@pytest.fixture(autouse=True)
def _inference_path():
    with torch.no_grad():
        yield


# ---- the state: a row-batched context after its steps, and each video's blocks from the single-video engine -----------------------
@functools.lru_cache(maxsize=None)
def _state(D, M, B, T, chunk, mode):
    model, _ = make_host(D, M, mode, seed=21)
    mp, fp = prompts(D, mode)
    vids = [frames(T, D, 5100 + b, mode) for b in range(B)]
    bp = BatchedProjector(model.recurrent_memory_transformer, B)
    _, info = arch.video_memory_tokens_batched(model, bp, vids, torch.arange(T), mp, fp, model.image_newline, chunk=chunk)
    torch.cuda.synchronize()
    eng = bp.engine(vids[0].device, vids[0].dtype)
    return types.SimpleNamespace(model=model, bp=bp, eng=eng, vids=vids, xs=info["pe_frames"], mp=mp, fp=fp,
                                 fine=arch._device_indices(info["fine_idx"], vids[0].device),
                                 nl=model.image_newline.detach().contiguous(), n=info["num_memories"], B=B, T=T, D=D, M=M,
                                 chunk=chunk, mems=[[m.clone() for m in bp.memory_cache(b)] for b in range(B)],
                                 scores=[s.clone() for s in info["frame_scores"]])


@functools.lru_cache(maxsize=None)
def _single_refs(D, M, B, T, chunk, mode, layouts, tiles):
    """want[(video, layout, with_frames, tile)]: the single-video emit of the batch's memory rows; plus each video's own
    single-video memories and frame scores.  Computed once per shape and left unchanged."""
    st = _state(D, M, B, T, chunk, mode)
    rm = st.model.recurrent_memory_transformer
    lib = capi.lib()
    want, mems, scores = {}, [], []
    for v in range(B):
        n0 = len(rm.frame_attn_scores)
        _, sinfo = arch.video_memory_tokens(st.model, st.vids[v], torch.arange(T), st.mp, st.fp, st.nl, True, chunk=chunk)
        torch.cuda.synchronize()
        mems.append([m.clone() for m in rm.memory_cache])
        scores.append([s.clone() for s in rm.frame_attn_scores[n0:]])
        assert len(rm.memory_cache) == len(st.mems[v]) == st.n
        for m_single, m_batch in zip(rm.memory_cache, st.mems[v]):
            m_single.copy_(m_batch)
        eng = rm.engine(st.vids[v].device, st.vids[v].dtype)
        fine = arch._device_indices(sinfo["fine_idx"], st.vids[v].device)
        for layout, wf, tile in itertools.product(layouts, (True, False), tiles):
            rows = arch.video_token_rows(T, M, with_frames=wf, layout=layout, chunk=chunk)
            out = torch.full((rows, D), SENTINEL, device="cuda", dtype=torch.int16).view(st.vids[v].dtype)
            w = ctypes.c_int64(0)
            capi.check(lib.mavlm_set_gemm_tile(tile), "tile")
            try:
                rc = lib.mavlm_fuse_emit_layout(eng.ctx, sinfo["pe_frames"].data_ptr(), fine.data_ptr(), fine.numel(), st.mp.data_ptr(),
                                                st.mp.shape[0], st.fp.data_ptr(), st.fp.shape[0],
                                                None if layout == "no_token" else st.nl.data_ptr(), 1 if wf else 0,
                                                capi.LAYOUTS[layout], out.data_ptr(), rows, ctypes.byref(w), ops.stream_ptr())
                torch.cuda.synchronize()
            finally:
                lib.mavlm_set_gemm_tile(0)
            capi.check(rc, "mavlm_fuse_emit_layout")
            assert w.value == rows
            want[(v, layout, wf, tile)] = out
    return want, mems, scores


def _fused_mask(st, layout, rows):
    """True on the fused memory rows of a block (the rows the second fuser GEMM writes)"""
    feat_rows = st.n * st.M * P
    period = arch.layout_period(layout, P)
    a = st.mp.shape[0]
    b_ = a + feat_rows + (feat_rows // period if period else 0)
    feat = np.zeros(rows, bool)
    feat[a:b_] = True
    if period:
        feat[a + period:b_:period + 1] = False
    assert feat.sum() == feat_rows
    return feat


def _check_block(st, want, blk, v, layout, wf, tile, label):
    w = bits(want[(v, layout, wf, tile)])
    assert blk.shape == w.shape
    assert not (blk == SENTINEL).all(axis=1).any(), f"{label} video {v}: a row of the block was never written"
    feat = _fused_mask(st, layout, blk.shape[0])
    bad = np.flatnonzero((blk[~feat] != w[~feat]).any(axis=1))
    assert bad.size == 0, f"{label} video {v}: {bad.size} prompt / newline / fine-frame rows differ, first {bad[:5]}"
    dt = st.vids[0].dtype
    got_f = torch.from_numpy(np.ascontiguousarray(blk[feat])).view(dt).float().numpy()
    want_f = torch.from_numpy(np.ascontiguousarray(w[feat])).view(dt).float().numpy()
    err = O.rel_l2(got_f, want_f)
    print(f"{label} video {v} tile {tile}: fused rows vs single-video emit rel-L2 {err:.3e}")
    assert err < ROW_BATCH_ROWS, (label, v, tile, err)
    if tile == 128:
        bad = np.flatnonzero((blk[feat] != w[feat]).any(axis=1))
        assert bad.size == 0, f"{label} video {v}: {bad.size} fused rows differ on the same tiles, first {bad[:5]}"


def _check_both_exports(st, want, layout, wf, tiles):
    """the constant-stride export and the per-video destinations, each into a sentinel-filled buffer; returns the two buffers'
    blocks of the last tile"""
    rows = arch.video_token_rows(st.T, st.M, with_frames=wf, layout=layout, chunk=st.chunk)
    dt = st.vids[0].dtype
    lib = capi.lib()
    out = None
    for tile in tiles:
        cap = rows + MARGIN
        ref = torch.full((st.B, cap, st.D), SENTINEL, device="cuda", dtype=torch.int16).view(dt)
        dst, out_rows = _scattered(st.B, rows)
        buf = torch.full((out_rows, st.D), SENTINEL, device="cuda", dtype=torch.int16).view(dt)
        capi.check(lib.mavlm_set_gemm_tile(tile), "tile")
        try:
            rc0, n0 = _emit(st, layout, wf, ref.data_ptr(), cap)
            rc1, n1 = _emit(st, layout, wf, buf.data_ptr(), out_rows, dst)
        finally:
            lib.mavlm_set_gemm_tile(0)
        capi.check(rc0, "mavlm_fuse_emit_layout_batch")
        capi.check(rc1, "mavlm_fuse_emit_layout_batch_to")
        assert n0 == n1 == rows
        r, g = bits(ref), bits(buf)
        assert (r[:, rows:] == SENTINEL).all(), "constant stride: rows behind a block were written"
        untouched = np.ones(out_rows, bool)
        for v in range(st.B):
            untouched[dst[v]:dst[v] + rows] = False
            _check_block(st, want, r[v, :rows], v, layout, wf, tile, f"{layout} wf={wf} constant stride")
            _check_block(st, want, g[dst[v]:dst[v] + rows], v, layout, wf, tile, f"{layout} wf={wf} per-video rows")
            assert (g[dst[v]:dst[v] + rows] == r[v, :rows]).all(), f"video {v}: the two exports differ"
        assert (g[untouched] == SENTINEL).all(), "rows outside the blocks were written"
        out = (r, g, dst, rows)
    return out


# ---- 1. the writer, smallest shapes ---------------------------------------------------------------------------------------------------
SMALL = (384, 2, 3, 20, 10)              # hidden 384 (three 128-column tiles, 8 heads of 48), M = 2, B = 3, 20 frames in chunks of 10


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("wf", [True, False])
@pytest.mark.parametrize("layout", arch.LAYOUTS)
def test_row_mapped_writer_smallest_shapes(layout, wf, mode):
    """392 rows per video, 1176 stacked rows per cached memory = 9 x 128 + 24: almost every 128-row tile spans two videos and
    the last tile is ragged - its rows m >= M would wrap into another video's block if they were stored."""
    st = _state(*SMALL, mode)
    assert st.n == 2 and st.fine.numel() == 20
    want, _, _ = _single_refs(*SMALL, mode, tuple(arch.LAYOUTS), (128, 0))
    _check_both_exports(st, want, layout, wf, (128, 0))


def test_row_mapped_writer_single_column_tile():
    shape = (128, 2, 3, 20, 10)
    st = _state(*shape, "bf16")
    want, _, _ = _single_refs(*shape, "bf16", ("grid",), (128, 0))
    _check_both_exports(st, want, "grid", True, (128, 0))


# ---- 2. the ragged emit ---------------------------------------------------------------------------------------------------------------
RAGGED_HEADS = 8                         # hidden 384: 8 heads of 48


@pytest.mark.parametrize("wf", [True, False])
@pytest.mark.parametrize("layout", arch.LAYOUTS)
def test_ragged_emit_blocks_narrow_width(layout, wf):
    """chunk counts 4, 2, 1: blocks of different lengths, ring slots held by 3, 2 and 1 videos"""
    _emit_case(_case2(hidden=384, heads=RAGGED_HEADS), layout, wf, [1, 2, 0], tile=128)


def test_ragged_emit_narrow_width_own_dispatch():
    _emit_case(_case2(hidden=384, heads=RAGGED_HEADS), "grid", True, [1, 2, 0], tile=0)


# ---- 3. the checkpoint shape ----------------------------------------------------------------------------------------------------------
CKPT = (896, 8, 2, 40, 32)               # hidden 896, 8 heads of 112, M = 8, B = 2, 40 frames in chunks of 32 + 8


@pytest.mark.parametrize("layout", ["one_token", "grid"])
def test_checkpoint_shape_blocks(layout):
    st = _state(*CKPT, "bf16")
    assert st.n == 2
    want, _, _ = _single_refs(*CKPT, "bf16", ("one_token", "grid"), (0,))
    _check_both_exports(st, want, layout, True, (0,))          # (the two exports bit for bit, each block against the single-video engine)


def test_checkpoint_shape_memories_and_frame_scores():
    """the suite's first row-batched steps with heads of 112"""
    st = _state(*CKPT, "bf16")
    _, mems, scores = _single_refs(*CKPT, "bf16", ("one_token", "grid"), (0,))
    assert len(st.scores) == 2
    for v in range(st.B):
        err = O.rel_l2(to_np(torch.cat(st.mems[v]).flatten(0, 1)), to_np(torch.cat(mems[v]).flatten(0, 1)))
        assert len(scores[v]) == len(st.scores)
        serr = max(O.rel_l2(to_np(sb[v]), to_np(ss)) for sb, ss in zip(st.scores, scores[v]))
        print(f"hidden 896 video {v}: memories vs single-video engine {err:.3e}, frame scores {serr:.3e}")
        assert err < ROW_BATCH_ROWS and serr < ROW_BATCH_ROWS


# ---- 4. the entry point ---------------------------------------------------------------------------------------------------------------
PROMPTS3 = [[101, IMG, 102], [111, 112, 113, 114], [IMG, 121]]           # sample 1 is text only


def _entry_point(monkeypatch, side, frame_counts, ragged):
    monkeypatch.setattr(vb, "CFG", O.PathConfig(hidden=384, heads=8, mem_tokens=2, depth=2))
    lm, model, hf, _, _ = vb._host()
    assert model.embed_tokens.weight.shape[1] == 384
    hf.tokenizer_padding_side = side
    videos = [vb._video(f, v) for v, f in enumerate(frame_counts)]
    sampled = [arch.sample_frame_count(f) for f in frame_counts]
    ids, mask, labels, pos = vb._samples(PROMPTS3)
    singles = []
    for s, vid in ((0, videos[0]), (2, videos[1])):
        n = len(PROMPTS3[s])
        one = vb._call(lm, ids[s:s + 1, :n], mask[s:s + 1, :n], labels[s:s + 1, :n], pos[s:s + 1, :n], [vid])
        singles.append(tuple(t.clone() if torch.is_tensor(t) else t for t in one))
    # the text-only sample by itself: its embedded ids, its labels, mask and positions as they are
    text = (None, pos[1:2, :4].to(singles[0][1].dtype), mask[1:2, :4].to(singles[0][2].dtype), None,
            model.embed_tokens(ids[1:2, :4]).to(singles[0][4].dtype), labels[1:2, :4].to(singles[0][5].dtype))
    singles.insert(1, text)
    if ragged:
        lm.enable_ragged_row_batches()
    before = lm.draws
    out = vb._call(lm, ids, mask, labels, pos, videos)
    torch.cuda.synchronize()
    assert lm.draws == before + 1                                   # one draw per forward
    w_emb, w_lab, w_mask, w_pos, starts = _pad_together(singles, side == "left")
    assert torch.equal(out[5], w_lab) and torch.equal(out[2], w_mask) and torch.equal(out[1], w_pos)
    emb = out[4]
    assert emb.shape == w_emb.shape and emb.dtype == w_emb.dtype
    same = torch.ones(emb.shape[:2], dtype=torch.bool, device="cuda")
    for s, t in ((0, sampled[0]), (2, sampled[1])):
        p = PROMPTS3[s].index(IMG)
        n = t // 32
        mem = slice(starts[s] + p + 10, starts[s] + p + 10 + n * 2 * P)
        same[s, mem] = False
        err = O.rel_l2(to_np(emb[s, mem]), to_np(w_emb[s, mem]))
        print(f"{side} ragged={ragged} sample {s}: fused memory rows, row batch vs single-sample call rel-L2 {err:.3e}")
        assert err < 6e-3                                           # (the gate of tests/test_gpu_video_batch.py for this comparison)
    assert torch.equal(emb[same], w_emb[same]), "text / prompt / newline / fine-frame rows differ"
    batchers = model.recurrent_memory_transformer.__dict__["_row_batchers"].values()          # the row batch ran: no single-video passes
    assert [capi.lib().mavlm_steps(b._engine.ctx) for b in batchers if b._engine is not None] == [max(sampled) // 32]


@pytest.mark.parametrize("side", ["right", "left"])
def test_entry_point_two_videos_and_a_text_sample(monkeypatch, side):
    _entry_point(monkeypatch, side, [40, 50], ragged=False)             # both sampled to 64 frames


@pytest.mark.parametrize("side", ["right", "left"])
def test_entry_point_ragged_row_batch(monkeypatch, side):
    assert [arch.sample_frame_count(f) for f in (40, 100)] == [64, 96]
    _entry_point(monkeypatch, side, [40, 100], ragged=True)


# ---- 5. the offset range ----------------------------------------------------------------------------------------------------------------
def test_destination_beyond_the_32_bit_reach_is_refused_before_anything_is_written():
    """the row-mapped form addresses its output with 32-bit byte offsets: a block that ends 4 GiB into `out` is refused on the host
    (MAVLM_E_SHAPE), before the first launch.  `out_rows` and `dst_row` only claim the size: the buffer is small and stays untouched."""
    st = _state(*SMALL, "bf16")
    rows = arch.video_token_rows(st.T, st.M, layout="grid", chunk=st.chunk)
    ok_dst, ok_rows = _scattered(st.B, rows)
    buf = torch.full((ok_rows, st.D), SENTINEL, device="cuda", dtype=torch.int16).view(torch.bfloat16)
    far = (1 << 32) // (st.D * 2)                                   # first row that starts 4 GiB into the buffer
    for dst in ([0, rows + 3, far], [far - rows // 2, 0, rows + 3]):
        rc, _ = _emit(st, "grid", True, buf.data_ptr(), far + 2 * rows, dst)
        assert rc == capi.E_SHAPE, dst
        assert (bits(buf) == SENTINEL).all(), "something was written before the refusal"
    rc, _ = _emit(st, "grid", True, buf.data_ptr(), far // 2 + rows)                 # constant stride: video 2 would start there
    assert rc == capi.E_SHAPE and (bits(buf) == SENTINEL).all()
    # the ragged export makes the same check
    out = (ctypes.c_int64 * 3)()
    xp = (capi.vp * 3)(*[x.data_ptr() for x in st.xs])
    fine = st.fine.repeat(3)
    rc = capi.lib().mavlm_fuse_emit_layout_ragged_to(st.eng.ctx, 3, xp, fine.data_ptr(), st.fine.numel(), st.mp.data_ptr(), 10,
                                                     st.fp.data_ptr(), 9, st.nl.data_ptr(), 1, capi.LAYOUTS["grid"], buf.data_ptr(),
                                                     far + 2 * rows, (ctypes.c_int64 * 3)(0, rows + 3, far), out, ops.stream_ptr())
    torch.cuda.synchronize()
    assert rc == capi.E_SHAPE and (bits(buf) == SENTINEL).all()
    # ... and a destination inside the reach still works afterwards
    rc, n = _emit(st, "grid", True, buf.data_ptr(), ok_rows, ok_dst)
    assert rc == 0 and n == rows
