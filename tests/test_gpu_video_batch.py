"""-m gpu: several videos per forward.  The export that takes one destination row per video (`mavlm_fuse_emit_layout_batch_to`)
against the constant-stride export on the same context and state, bit for bit; `prepare_inputs_labels_for_multimodal` with a
padded batch of samples against the single-sample calls; one dropout draw per forward; the training route against the float64
oracle; `LlavaQwenForCausalLM.forward / generate` with two samples.  No test reads anything outside the repository."""
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
from oracle import torch_path as TP
from gpu_util import to_dev, to_np, DT
from test_gpu_layouts import SENTINEL, bits, frames, make_host, prompts
from test_gpu_path import _tiny_host

pytestmark = pytest.mark.gpu
P = 196
IMG = arch.IMAGE_TOKEN_INDEX


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch_state(D, M, B, T, chunk, mode):
    """a row-batched context after its chunk steps (the state both exports read), with what the emit calls take"""
    model, _ = make_host(D, M, mode, seed=21)
    mp, fp = prompts(D, mode)
    vids = [frames(T, D, 5100 + b, mode) for b in range(B)]
    bp = BatchedProjector(model.recurrent_memory_transformer, B)
    with torch.no_grad():
        _, info = arch.video_memory_tokens_batched(model, bp, vids, torch.arange(T), mp, fp, model.image_newline, chunk=chunk)
    torch.cuda.synchronize()
    eng = bp.engine(vids[0].device, vids[0].dtype)
    fine = arch._device_indices(info["fine_idx"], vids[0].device)
    return types.SimpleNamespace(model=model, bp=bp, eng=eng, xs=info["pe_frames"], fine=fine, mp=mp, fp=fp,
                                 nl=model.image_newline.detach().contiguous(), n=info["num_memories"], B=B, T=T, D=D, M=M, chunk=chunk)


def _emit(st, layout, wf, out_ptr, cap_rows, dst=None, ctx=None):
    """(return code, rows) of mavlm_fuse_emit_layout_batch (dst None) / mavlm_fuse_emit_layout_batch_to on the state"""
    xp = (capi.vp * st.B)(*[x.data_ptr() for x in st.xs])
    rows = ctypes.c_int64(-1)
    head = (ctx if ctx is not None else st.eng.ctx, xp, st.fine.data_ptr(), st.fine.numel(), st.mp.data_ptr(), st.mp.shape[0],
            st.fp.data_ptr(), st.fp.shape[0], None if layout == "no_token" else st.nl.data_ptr(), 1 if wf else 0, capi.LAYOUTS[layout],
            out_ptr, cap_rows)
    if dst is None:
        rc = capi.lib().mavlm_fuse_emit_layout_batch(*head, ctypes.byref(rows), ops.stream_ptr())
    else:
        rc = capi.lib().mavlm_fuse_emit_layout_batch_to(*head, (ctypes.c_int64 * len(dst))(*dst), ctypes.byref(rows), ops.stream_ptr())
    torch.cuda.synchronize()
    return rc, rows.value


def _scattered(B, rows):
    """destinations in reverse video order with unequal gaps: video B-1 first; (dst_row, out_rows)"""
    gaps = [3, 7, 20, 1, 13, 2, 9, 5][:B]
    dst, at = [0] * B, 0
    for k, b in enumerate(reversed(range(B))):
        at += gaps[k]
        dst[b] = at
        at += rows
    return dst, at + 9


def _check_scattered(st, layout, wf):
    rows = arch.video_token_rows(st.T, st.M, with_frames=wf, layout=layout, chunk=st.chunk)
    dt = st.xs[0].dtype
    ref = torch.full((st.B, rows, st.D), SENTINEL, device="cuda", dtype=torch.int16).view(dt)
    rc, n = _emit(st, layout, wf, ref.data_ptr(), rows)
    assert rc == 0 and n == rows
    dst, out_rows = _scattered(st.B, rows)
    buf = torch.full((out_rows, st.D), SENTINEL, device="cuda", dtype=torch.int16).view(dt)
    rc, n = _emit(st, layout, wf, buf.data_ptr(), out_rows, dst)
    assert rc == 0 and n == rows
    got, want = bits(buf), bits(ref)
    untouched = np.ones(out_rows, bool)
    for b in range(st.B):
        blk = got[dst[b]:dst[b] + rows]
        bad = np.flatnonzero((blk != want[b]).any(axis=1))
        assert bad.size == 0, f"video {b}: {bad.size} rows differ from the constant-stride export, first {bad[:5]}"
        assert not (blk == SENTINEL).all(axis=1).any(), f"video {b}: a row of the block was never written"
        untouched[dst[b]:dst[b] + rows] = False
    assert (got[untouched] == SENTINEL).all(), "rows outside the blocks were written"
    return buf, dst, out_rows, rows


@pytest.mark.parametrize("tile", [129, 256, 257])
@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("wf", [True, False])
@pytest.mark.parametrize("layout", arch.LAYOUTS)
def test_per_video_destinations_equal_the_constant_stride_export(layout, wf, mode, tile):
    """hidden 256 (one column tile), 8 heads, M = 2, B = 3: 392 rows per video, so the 128- / 224- / 256-row tiles of the fuser's
    second GEMM (2352 stacked rows) span two videos; two cached memories, 20 fine frames.  Each 256-column-tile kernel is forced
    in turn (129: 128x256, 256: plain, 257: persistent)."""
    st = _batch_state(256, 2, 3, 20, 10, mode)
    assert st.n == 2 and st.fine.numel() == 20
    assert capi.lib().mavlm_set_gemm_tile(tile) == 0
    try:
        _check_scattered(st, layout, wf)
    finally:
        capi.lib().mavlm_set_gemm_tile(0)


@pytest.mark.parametrize("layout", ["one_token", "grid"])
def test_per_video_destinations_checkpoint_shape(layout):
    """hidden 1024, M = 8 (1568 rows per video), B = 2, 40 frames in chunks of 32 + 8: the kernels the shape takes by itself"""
    st = _batch_state(1024, 8, 2, 40, 32, "bf16")
    assert st.n == 2
    _check_scattered(st, layout, True)


def test_per_video_destinations_refusals():
    st = _batch_state(256, 2, 3, 20, 10, "bf16")
    rows = arch.video_token_rows(st.T, st.M, layout="grid", chunk=10)
    dst, out_rows = _scattered(st.B, rows)
    buf = torch.full((out_rows + 1, st.D), SENTINEL, device="cuda", dtype=torch.int16).view(torch.bfloat16)
    cases = {"overlap": ([dst[0], dst[0] - rows + 1, dst[2]], buf.data_ptr()),
             "same row": ([dst[0], dst[0], dst[2]], buf.data_ptr()),
             "past the end": ([out_rows - rows + 1, dst[1], dst[2]], buf.data_ptr()),
             "negative": ([dst[0], dst[1], -1], buf.data_ptr()),
             "misaligned": (dst, buf.data_ptr() + 2)}
    for name, (d, ptr) in cases.items():
        rc, _ = _emit(st, "grid", True, ptr, out_rows, d)
        assert rc == capi.E_ARG, name
        assert (bits(buf) == SENTINEL).all(), f"{name}: something was written before the refusal"
    # a single-video context has no per-video destinations
    with torch.no_grad():
        arch.video_memory_tokens(st.model, frames(st.T, st.D, 5200), torch.arange(st.T), st.mp, st.fp, st.model.image_newline, chunk=10)
    one = st.model.recurrent_memory_transformer.engine(st.xs[0].device, st.xs[0].dtype)
    xp = (capi.vp * 1)(st.xs[0].data_ptr())
    r = ctypes.c_int64(0)
    rc = capi.lib().mavlm_fuse_emit_layout_batch_to(one.ctx, xp, st.fine.data_ptr(), st.fine.numel(), st.mp.data_ptr(), 10,
                                                    st.fp.data_ptr(), 9, st.nl.data_ptr(), 1, capi.LAYOUTS["grid"], buf.data_ptr(),
                                                    out_rows, (ctypes.c_int64 * 1)(0), ctypes.byref(r), ops.stream_ptr())
    torch.cuda.synchronize()
    assert rc == capi.E_STATE and (bits(buf) == SENTINEL).all()
    # ... and the valid call still works afterwards
    rc, n = _emit(st, "grid", True, buf.data_ptr(), out_rows, dst)
    assert rc == 0 and n == rows


# ---- the toy host of the entry-point tests -----------------------------------------------------------------------------------------
CFG = O.PathConfig(hidden=256, heads=8, mem_tokens=2, depth=2)
SIDE, TABLE_FRAMES = 27, 128
TEXT_IDS = list(range(100, 140))


def _weights():
    return O.make_weights(CFG, seed=31)


def _host(seed=0):
    """hidden 256, 8 heads, M = 2, depth 2, bf16 (oracle weights); a toy tower of 27 x 27 patches (a table lookup by frame id),
    so the HIP bilinear pool runs; `get_synced_dropout_decision` counts its calls and returns `lm.draw`"""
    w = _weights()
    model, hf = _tiny_host(CFG, w)
    rows = sorted(set(O.MEM_PROMPT_IDS + O.FRAME_PROMPT_IDS + TEXT_IDS))
    emb = np.zeros((48900, CFG.hidden), np.float32)
    emb[rows] = O.bf16_round(O.hash_normal_like((len(rows), CFG.hidden), 81, 0.02))
    with torch.no_grad():
        model.embed_tokens.weight.copy_(to_dev(emb))
        model.image_newline.copy_(to_dev(w["image_newline"]))
    table = to_dev(O.hash_normal_like((TABLE_FRAMES, 1, CFG.hidden), 92)).repeat(1, SIDE * SIDE, 1).contiguous()
    table += to_dev(O.hash_normal_like((1, SIDE * SIDE, CFG.hidden), 93))

    class Tower(torch.nn.Module):
        num_patches_per_side = SIDE

        def forward(self, images):
            return table[images.reshape(-1).long()]

    model.vision_tower = Tower()
    model.mm_projector = torch.nn.Identity()

    class LM(arch.LlavaMetaForCausalLM, torch.nn.Module):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.config = hf
            self.model = model
            self.draws, self.draw = 0, False

        def get_model(self):
            return self.model

        def get_synced_dropout_decision(self, prob=0.5):
            self.draws += 1
            return self.draw

        @property
        def device(self):
            return torch.device("cuda")

    return LM().eval(), model, hf, w, emb


def _video(n_frames, v):
    """frame ids into the tower's table: video v walks the table with a stride and an offset of its own"""
    ids = (torch.arange(n_frames) * (2 * v + 1) + 5 * v) % TABLE_FRAMES
    return ids.to(torch.float32).reshape(n_frames, 1, 1, 1).cuda()


def _samples(prompts_, pad_id=0):
    """right-padded ids / mask / labels / position ids of prompts of different lengths"""
    L = max(len(p) for p in prompts_)
    ids = torch.tensor([p + [pad_id] * (L - len(p)) for p in prompts_], device="cuda")
    mask = torch.tensor([[1] * len(p) + [0] * (L - len(p)) for p in prompts_], device="cuda")
    labels = torch.where((ids == IMG) | (mask == 0), torch.tensor(arch.IGNORE_INDEX, device="cuda"), ids)
    pos = torch.arange(L, device="cuda")[None].expand(len(prompts_), -1).contiguous()
    return ids, mask, labels, pos


def _call(lm, ids, mask, labels, pos, videos):
    return lm.prepare_inputs_labels_for_multimodal(ids, pos, mask, None, labels, videos, modalities=["video"] * len(videos))


def _pad_together(singles, left):
    """what padding single-sample results together gives: (emb, labels, mask, pos) - the issue's definition of the result"""
    L = max(s[4].shape[1] for s in singles)
    B, D = len(singles), singles[0][4].shape[2]
    emb = torch.zeros((B, L, D), device="cuda", dtype=singles[0][4].dtype)
    lab = torch.full((B, L), arch.IGNORE_INDEX, device="cuda", dtype=singles[0][5].dtype)
    mask = torch.zeros((B, L), device="cuda", dtype=singles[0][2].dtype)
    pos = torch.zeros((B, L), device="cuda", dtype=singles[0][1].dtype)
    starts = []
    for b, s in enumerate(singles):
        n = s[4].shape[1]
        sl = slice(L - n, L) if left else slice(0, n)
        starts.append(sl.start)
        emb[b, sl], lab[b, sl], mask[b, sl], pos[b, sl] = s[4][0], s[5][0], s[2][0], s[1][0]
    return emb, lab, mask, pos, starts


# ---- 2. the entry point, inference -------------------------------------------------------------------------------------------------
FRAMES5 = [40, 50, 40, 100, 20]                  # sampled to 64, 64, 64, 96, 20: one row batch of 2 (videos 0, 1) and three singles
PROMPTS5 = [[IMG, 101, 102, 103], [111, 112, IMG, 113, 114, 115, 116], [121, 122, 123, IMG], [131, IMG], [104, 105, 106, IMG, 107]]


@pytest.mark.parametrize("layout", ["one_token", "grid"])
@pytest.mark.parametrize("side", ["right", "left"])
def test_entry_point_batch_of_five_equals_single_sample_calls(side, layout):
    lm, model, hf, _, _ = _host()
    hf.tokenizer_padding_side = side
    hf.mm_newline_position = layout
    assert arch.token_layout(hf) == layout
    videos = [_video(f, v) for v, f in enumerate(FRAMES5)]
    assert [arch.sample_frame_count(f) for f in FRAMES5] == [64, 64, 64, 96, 20]
    assert not torch.equal(arch.sample_frame_indices(40), arch.sample_frame_indices(50))          # per-video frame indices
    ids, mask, labels, pos = _samples(PROMPTS5)
    with torch.no_grad():
        singles = []
        for s in range(5):
            n = len(PROMPTS5[s])
            singles.append(_call(lm, ids[s:s + 1, :n], mask[s:s + 1, :n], labels[s:s + 1, :n], pos[s:s + 1, :n], [videos[s]]))
            singles[-1] = tuple(t.clone() if torch.is_tensor(t) else t for t in singles[-1])
        before = lm.draws
        out = _call(lm, ids, mask, labels, pos, videos)
        assert lm.draws == before + 1                                                             # one draw per forward
        again = _call(lm, ids, mask, labels, pos, videos)
        after = _call(lm, ids[:1, :4], mask[:1, :4], labels[:1, :4], pos[:1, :4], [videos[0]])
        # the row-batched group called directly (the model's own size-2 engine, per-video indices)
        mp = model.embed_tokens(torch.tensor(arch.MEMORY_PROMPT_IDS, device="cuda"))
        fp = model.embed_tokens(torch.tensor(arch.FRAME_PROMPT_IDS, device="cuda"))
        pooled = [lm.get_2dPool(lm.encode_images(videos[v][arch.sample_frame_indices(FRAMES5[v]).cuda()])) for v in (0, 1)]
        direct = arch.video_memory_tokens_batched(model, model.recurrent_memory_transformer.row_batcher(2), pooled,
                                                  [arch.sample_frame_indices(FRAMES5[v]) for v in (0, 1)], mp, fp,
                                                  model.image_newline, layout=layout)
    torch.cuda.synchronize()
    assert out[0] is None and out[3] is None
    w_emb, w_lab, w_mask, w_pos, starts = _pad_together(singles, side == "left")
    assert torch.equal(out[5], w_lab) and out[5].dtype == w_lab.dtype
    assert torch.equal(out[2], w_mask) and out[2].dtype == w_mask.dtype
    assert torch.equal(out[1], w_pos) and out[1].dtype == w_pos.dtype
    emb = out[4]
    assert emb.shape == w_emb.shape and emb.dtype == w_emb.dtype
    # rows of the fused memory tokens of the two row-batched videos: the row batch's bits, within the row-batch gate of the
    # single-video engine (tests/test_gpu_batch.py); every other row of the buffer: the single-sample calls' bits
    same = torch.ones(emb.shape[:2], dtype=torch.bool, device="cuda")
    a, b = direct[1]["memory_rows"]
    for v in (0, 1):
        p = PROMPTS5[v].index(IMG)
        blk = slice(starts[v] + p, starts[v] + p + direct[0].shape[1])
        assert torch.equal(emb[v, blk], direct[0][v]), f"video {v}: not the row batch's bits"
        mem = slice(blk.start + a, blk.start + b)
        same[v, mem] = False
        err = O.rel_l2(to_np(emb[v, mem]), to_np(w_emb[v, mem]))
        print(f"{side} {layout} video {v}: fused memory rows, row batch vs single-sample call rel-L2 {err:.3e}")
        assert err < 6e-3
    assert torch.equal(emb[same], w_emb[same]), "text / prompt / newline / fine-frame rows or a single video's block differ"
    if layout == "grid":                                            # (newlines sit INSIDE the memory rows there: check them too)
        nl = model.image_newline.detach()
        for v in (0, 1):
            p = PROMPTS5[v].index(IMG)
            r0 = starts[v] + p + a
            assert torch.equal(emb[v, r0 + 14], nl) and torch.equal(emb[v, r0 + 29], nl)
    assert torch.equal(again[4], emb) and torch.equal(again[5], out[5])                            # the same bits again
    assert torch.equal(after[4], singles[0][4])                                                   # V == 1 before and after


def test_entry_point_text_only_sample_truncation_and_graph_cache():
    """a text-only sample beside the videos; a tokenizer_model_max_length that cuts a sample (general path: the same rows, cut);
    `enable_memory_graphs` steps aside for V >= 2 and keeps serving V == 1"""
    lm, model, hf, _, _ = _host()
    prompts_ = [[101, IMG, 102], [111, 112, 113, 114], [IMG, 121]]
    videos = [_video(40, 0), _video(50, 1)]
    ids, mask, labels, pos = _samples(prompts_)
    with torch.no_grad():
        out = _call(lm, ids, mask, labels, pos, videos)
        rows = arch.video_token_rows(64, 2)
        assert out[4].shape[1] == rows + 2 and int(out[2][1].sum()) == 4
        assert torch.equal(out[4][1, :4], model.embed_tokens(ids[1, :4])) and not out[4][1, 4:].any()
        hf.tokenizer_model_max_length = rows - 5
        cut = _call(lm, ids, mask, labels, pos, videos)
        hf.tokenizer_model_max_length = 32768
        n = rows - 5
        assert cut[4].shape[1] == n and torch.equal(cut[4], out[4][:, :n]) and torch.equal(cut[5], out[5][:, :n])
        lm.enable_memory_graphs(2)
        one = [_call(lm, ids[:1, :3], mask[:1, :3], labels[:1, :3], pos[:1, :3], videos[:1])[4].clone() for _ in range(3)]
        assert len(lm._mem_graphs) == 1                             # (third call: a replay)
        both = _call(lm, ids, mask, labels, pos, videos)
        assert len(lm._mem_graphs) == 1 and torch.equal(both[4], out[4])
        assert torch.equal(one[0], one[2])


# ---- 3. one draw -------------------------------------------------------------------------------------------------------------------
def test_one_dropout_draw_per_forward_applies_to_every_video():
    lm, model, hf, _, _ = _host()
    hf.dropout_frames = True
    prompts_ = [[101, IMG, 102], [IMG, 111, 112, 113], [121, 122, IMG]]
    videos = [_video(40, 0), _video(40, 1), _video(20, 2)]
    ids, mask, labels, pos = _samples(prompts_)
    full = [arch.video_token_rows(t, 2) for t in (64, 64, 20)]
    short = [arch.video_token_rows(t, 2, with_frames=False) for t in (64, 64, 20)]
    with torch.no_grad():
        lm.draw = True                                              # inference: the draw is made, and ignored
        out = _call(lm, ids, mask, labels, pos, videos)
        assert lm.draws == 1 and [int(m.sum()) for m in out[2]] == [len(p) - 1 + r for p, r in zip(prompts_, full)]
        lm.train()                                                  # training mode without a gradient consumer: blocks emitted in place
        out = _call(lm, ids, mask, labels, pos, videos)
        assert lm.draws == 2 and [int(m.sum()) for m in out[2]] == [len(p) - 1 + r for p, r in zip(prompts_, short)]
        nograd = out[4].clone()
    out = _call(lm, ids, mask, labels, pos, videos)                 # under autograd: the training route
    assert lm.draws == 3 and out[4].requires_grad
    assert [int(m.sum()) for m in out[2]] == [len(p) - 1 + r for p, r in zip(prompts_, short)]
    fp0 = model.embed_tokens(torch.tensor(arch.FRAME_PROMPT_IDS[:1], device="cuda"))[0]
    for s, p in enumerate(prompts_):                                # no frame prompt anywhere in a block
        at = p.index(IMG)
        assert not (out[4][s, at:at + short[s]] == fp0).all(dim=1).any()
    assert O.rel_l2(to_np(out[4]), to_np(nograd)) < 2e-3             # (training forward: one extra rounding in the fuser)
    lm.draw = False
    out = _call(lm, ids, mask, labels, pos, videos)
    assert lm.draws == 4 and [int(m.sum()) for m in out[2]] == [len(p) - 1 + r for p, r in zip(prompts_, full)]
    model.recurrent_memory_transformer.memory_cache = []


# ---- 4. training -------------------------------------------------------------------------------------------------------------------
FRAMES3 = [40, 50, 20]                            # sampled 64, 64, 20: a row batch of 2 and a single
PROMPTS3 = [[101, IMG, 102], [IMG, 111, 112, 113], [121, 122, IMG]]


def test_training_batch_vs_float64_oracle_and_single_sample_passes():
    """Gates of tests/test_gpu_batch_train.py: every parameter gradient within 6e-2 (bf16) of the float64 autograd of
    oracle/torch_path.py summed over the videos, k_proj.bias (true gradient 0) <= 2e-3 of the largest gradient norm, and the
    batched error <= 1.5 x the error of three single-sample passes accumulated by autograd.

    Measured figures: see the printed lines (run with -s)."""
    lm, model, hf, w, emb_np = _host()
    lm.train()
    model.embed_tokens.weight.requires_grad_(False)
    videos = [_video(f, v) for v, f in enumerate(FRAMES3)]
    ids, mask, labels, pos = _samples(PROMPTS3)
    idxs = [arch.sample_frame_indices(f) for f in FRAMES3]
    with torch.no_grad():
        pooled = [lm.get_2dPool(lm.encode_images(videos[v][idxs[v].cuda()])) for v in range(3)]
    rows = [arch.video_token_rows(t, 2) for t in (64, 64, 20)]
    L = max(len(p) - 1 + r for p, r in zip(PROMPTS3, rows))
    cot_np = O.bf16_round(O.hash_normal_like((3, L, CFG.hidden), 8400, 0.05))
    cot = torch.from_numpy(cot_np).cuda()
    params = dict(model.named_parameters())

    # three single-sample passes, gradients accumulated by autograd
    model.zero_grad(set_to_none=True)
    single_loss = 0.0
    for s in range(3):
        n = len(PROMPTS3[s])
        o = _call(lm, ids[s:s + 1, :n], mask[s:s + 1, :n], labels[s:s + 1, :n], pos[s:s + 1, :n], [videos[s]])
        l1 = (o[4][0].float() * cot[s, :o[4].shape[1]]).sum()
        l1.backward()
        single_loss += float(l1.detach())
    single = {k: to_np(p.grad) for k, p in params.items() if p.grad is not None}

    # one batched pass
    model.zero_grad(set_to_none=True)
    out = _call(lm, ids, mask, labels, pos, videos)
    emb = out[4]
    assert emb.requires_grad and emb.shape == (3, L, CFG.hidden)
    loss = (emb.float() * cot).sum()
    loss.backward()
    batched = {k: to_np(p.grad) for k, p in params.items() if p.grad is not None}
    # forward: the grouped videos' blocks are video_memory_tokens_batched_train's bits
    mp = model.embed_tokens(torch.tensor(arch.MEMORY_PROMPT_IDS, device="cuda"))
    fp = model.embed_tokens(torch.tensor(arch.FRAME_PROMPT_IDS, device="cuda"))
    toks, _ = arch.video_memory_tokens_batched_train(model, model.recurrent_memory_transformer.row_batcher(2), pooled[:2], idxs[:2],
                                                     mp, fp, model.image_newline)
    for v in (0, 1):
        at = PROMPTS3[v].index(IMG)
        assert torch.equal(emb[v, at:at + rows[v]].detach(), toks[v].detach()), v
    model.recurrent_memory_transformer.row_batcher(2).reset()
    model.recurrent_memory_transformer.memory_cache = []

    # float64 oracle of the same three blocks
    p64 = TP.params_from(w)
    e64 = torch.from_numpy(emb_np).double()
    nl = p64["image_newline"].reshape(1, -1)
    t_loss = 0.0
    for v in range(3):
        x = to_np(pooled[v])
        T = x.shape[0]
        xpe = O.pe_add(x, idxs[v].numpy(), w["positional_encoding.frame_embed"], "bf16")
        bounds = O.uniform_segment_variant(T, 32)
        cache = TP.run_steps(p64, CFG, [xpe[bounds[i]:bounds[i + 1]] for i in range(len(bounds) - 1)])
        fine = torch.from_numpy(xpe[O.fine_frame_indices(T)]).double() + p64["token_type_embedding.weight"][1]
        blk = torch.cat([e64[list(O.MEM_PROMPT_IDS)], TP.fuse(p64, cache), nl, e64[list(O.FRAME_PROMPT_IDS)],
                         fine.reshape(-1, CFG.hidden), nl])
        at = PROMPTS3[v].index(IMG)
        t_loss = t_loss + (blk * torch.from_numpy(cot_np[v, at:at + rows[v]]).double()).sum()
    ref = TP.grads(p64, t_loss)

    print(f"loss (blocks + text rows) batched {float(loss.detach()):.5f} single-sample {single_loss:.5f}")
    scale = max(np.linalg.norm(v) for v in ref.values())
    fails, checked = [], 0
    for name, r in ref.items():
        if name not in batched:
            continue
        g = batched[name]
        assert np.isfinite(g).all(), name
        if name.endswith("k_proj.bias"):                          # true gradient is 0 (softmax shift invariance)
            print(f"{name}: |g| / largest norm batched {np.linalg.norm(g) / scale:.2e} single {np.linalg.norm(single[name]) / scale:.2e}")
            if np.linalg.norm(g) > 2e-3 * scale:
                fails.append((name, "k_proj.bias", np.linalg.norm(g) / scale))
            continue
        eb, es = O.rel_l2(g, r), O.rel_l2(single[name], r)
        print(f"{name}: rel-L2 vs float64 batched {eb:.3e} single-sample {es:.3e} ratio {eb / max(es, 1e-30):.2f}")
        checked += 1
        if not eb < 6e-2:
            fails.append((name, "gate", eb))
        if not eb <= 1.5 * es:
            fails.append((name, "1.5 x single", eb, es))
    assert checked >= len(ref) - 4, (checked, len(ref))
    for name in ("image_newline", "token_type_embedding.weight"):
        assert batched[name].any(), name
    assert not fails, fails


# ---- 5. the wrapper ----------------------------------------------------------------------------------------------------------------
def test_wrapper_forward_and_generate_with_two_samples():
    from test_gpu_llava_qwen import VOCAB, build
    m = build(256, 1, 4, 2, 512, mem_tokens=2)
    torch.manual_seed(13)
    videos = [torch.randn(20, 3, 54, 54, device="cuda", dtype=torch.bfloat16) for _ in range(2)]
    prompts_ = [[7, 8, IMG, 9, 10, 11], [21, IMG, 22]]
    ids, mask, labels, pos = _samples(prompts_)
    rows = arch.video_token_rows(20, 2)
    L = 5 + rows
    seen = {}

    def grab(_mod, args, kwargs):
        if kwargs.get("inputs_embeds") is not None and kwargs["inputs_embeds"].shape[1] > 1:
            seen["emb"] = kwargs["inputs_embeds"].detach().clone()
            seen["pos"], seen["mask"] = kwargs.get("position_ids"), kwargs.get("attention_mask")
    h = m.model.register_forward_pre_hook(grab, with_kwargs=True)
    try:
        with torch.no_grad():
            want = arch.LlavaMetaForCausalLM.prepare_inputs_labels_for_multimodal(m, ids, pos, mask, None, labels, videos,
                                                                                  ["video", "video"])
            n0 = m.multimodal_prefills
            out = m(input_ids=ids, labels=labels, images=videos, modalities=["video", "video"], attention_mask=mask, position_ids=pos)
        assert m.multimodal_prefills == n0 + 1
        assert out.logits.shape == (2, L, VOCAB) and torch.isfinite(out.loss)
        assert torch.equal(seen["emb"], want[4]) and torch.equal(seen["mask"], want[2]) and torch.equal(seen["pos"], want[1])
        assert want[4].shape == (2, L, 256) and int(want[2][1].sum()) == 2 + rows and not want[4][1, 2 + rows:].any()
        # generate: left-padded prompts, one pass of the memory path for the prefill of both samples
        m.config.tokenizer_padding_side = "left"
        Lp = ids.shape[1]
        lids = torch.stack([torch.cat([ids[s, len(p):], ids[s, :len(p)]]) for s, p in enumerate(prompts_)])
        lmask = torch.stack([torch.cat([mask[s, len(p):], mask[s, :len(p)]]) for s, p in enumerate(prompts_)])
        assert lids.shape == (2, Lp) and int(lmask[1, 0]) == 0 and int(lmask[1, -1]) == 1
        with torch.no_grad():
            wantl = arch.LlavaMetaForCausalLM.prepare_inputs_labels_for_multimodal(m, lids, None, lmask, None, None, videos,
                                                                                   ["video", "video"])
            n0 = m.multimodal_prefills
            new = m.generate(lids, images=videos, modalities=["video", "video"], attention_mask=lmask, max_new_tokens=2,
                             do_sample=False, pad_token_id=0)
        assert m.multimodal_prefills == n0 + 1
        assert new.shape == (2, 2)
        assert torch.equal(seen["emb"], wantl[4]) and torch.equal(seen["mask"], wantl[2])
        assert not wantl[4][1, :L - (2 + rows)].any() and int(wantl[2][1, :L - (2 + rows)].sum()) == 0      # padding on the left
        assert torch.equal(wantl[4][0], want[4][0])                  # (the longest sample has no padding on either side)
    finally:
        h.remove()
