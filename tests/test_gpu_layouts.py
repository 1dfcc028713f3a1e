"""-m gpu: the video token layouts (newline per grid row, per frame, one, none; llava_arch.py:567-634 of the reference) through
the C ABI.  A layout is the values of the "one_token" block at other rows with copies of `image_newline` in between, so the gate
is bit equality with `relayout` of the same call's "one_token" block - the numpy function tests/test_layouts_cpu.py pins to the
reference's own outputs (g11_layouts.npz) - plus one run against the oracle that does not depend on the "one_token" run.

The bit tests need no oracle: weights are drawn on the device (N(0, 1 / fan_in)), each shape's "one_token" block is computed
once and every expectation derives from it."""
import types

import numpy as np
import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd.model import llava_arch as arch
from memory_augmented_vlm_amd.model.memory_module.MemoryController import BatchedProjector
from oracle import memory_path as O
from conftest import load_golden
from gpu_util import to_dev, to_np, load_oracle_weights, DT
from test_layouts_cpu import EXPECTED, PERIOD, relayout_tokens
from test_gpu_path import chain_tol

pytestmark = pytest.mark.gpu
P = 196
OTHERS = ("no_token", "frame", "grid")
SENTINEL = 0x7B7B          # a finite 16-bit pattern no kernel output of these tests takes on a whole row
PAD = 5                    # sentinel rows on either side of a block


def bits(t):
    """raw 16-bit patterns of a tensor as numpy int16 (bit equality, whatever the dtype)"""
    return t.detach().contiguous().view(torch.int16).cpu().numpy()


def make_host(D, M, mode="bf16", seed=0):
    """LlavaMetaModel on the device with weights drawn there: matrices N(0, 1 / fan_in), LayerNorm gains around 1, everything
    else N(0, 0.02^2); `image_newline` without a zero element."""
    class Base(torch.nn.Module):
        def __init__(self, config):
            super().__init__()
            self.embed_tokens = torch.nn.Embedding(64, config.hidden_size)

    class Model(arch.LlavaMetaModel, Base):
        pass

    hf = types.SimpleNamespace(hidden_size=D, num_memory_tokens=M, mm_patch_merge_type="spatial_unpad",
                               mm_newline_position="one_token", mm_spatial_pool_mode="bilinear",
                               tokenizer_model_max_length=32768, tokenizer_padding_side="right")
    with torch.device("cuda"):
        model = Model(hf).eval()
        model.image_newline = torch.nn.Parameter(torch.zeros(D))
    g = torch.Generator(device="cuda").manual_seed(1000 + seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            r = torch.randn(p.shape, generator=g, device="cuda", dtype=torch.float32)
            leaf = name.split(".")[-1]
            if name.endswith("layernorm.weight"):
                p.copy_(1.0 + 0.1 * r)
            elif name == "image_newline":
                p.copy_(0.05 * (r.abs() + 0.1) * torch.where(r < 0, -1.0, 1.0))
            elif leaf in ("initial_memory", "memory_pos_embed"):
                p.copy_(r)
            elif p.dim() >= 2 and "embed" not in name:
                p.copy_(r / p.shape[-1] ** 0.5)
            else:
                p.copy_(0.02 * r)
    model = model.to(DT[mode])
    assert float(model.image_newline.detach().abs().min()) > 0          # a zero newline would equal an unwritten zero-filled row
    return model, hf


def prompts(D, mode="bf16", seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mp = (0.02 * torch.randn((10, D), generator=g, device="cuda")).to(DT[mode])
    fp = (0.02 * torch.randn((9, D), generator=g, device="cuda")).to(DT[mode])
    return mp, fp


def frames(T, D, seed, mode="bf16"):
    """hash-normal frames: every row is different, so a misplaced row shows"""
    return to_dev(O.hash_normal_like((T, P, D), seed), mode)


def emit(model, x, idx, mp, fp, layout, with_frames=True, newline="model"):
    """video_memory_tokens into a slice of a larger sentinel-filled buffer; returns the block after checking both margins"""
    M = model.recurrent_memory_transformer.num_memory_tokens
    rows = arch.video_token_rows(x.shape[0], M, with_frames=with_frames, layout=layout)
    buf = torch.full((rows + 2 * PAD, x.shape[2]), SENTINEL, device="cuda", dtype=torch.int16).view(x.dtype)
    nl = model.image_newline if newline == "model" else newline
    out, info = arch.video_memory_tokens(model, x, idx, mp, fp, nl, with_frames=with_frames, out=buf[PAD:PAD + rows], layout=layout)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf[PAD:].data_ptr() and out.shape[0] == rows
    b = bits(buf)
    assert (b[:PAD] == SENTINEL).all() and (b[PAD + rows:] == SENTINEL).all(), f"{layout}: rows outside the block were written"
    assert not (b[PAD:PAD + rows] == SENTINEL).all(axis=1).any(), f"{layout}: a row of the block was never written"
    return b[PAD:PAD + rows], info


def check_layouts(model, x, idx, mp, fp, label):
    M = model.recurrent_memory_transformer.num_memory_tokens
    T = x.shape[0]
    mem_rows, fine_rows = min(-(-T // 32), 10) * M * P, min(32, T) * P
    nlb = bits(model.image_newline)
    for wf in (True, False):
        one, info = emit(model, x, idx, mp, fp, "one_token", wf)
        a = 10 + mem_rows
        assert info["memory_rows"] == (10, a)
        assert (one[a] == nlb).all() and (one[-1] == nlb).all()                     # the newline rows are image_newline
        assert np.unique(one[10:a], axis=0).shape[0] == mem_rows                    # distinct rows: a swap would show
        for L in OTHERS:
            got, info = emit(model, x, idx, mp, fp, L, wf, newline=None if L == "no_token" else "model")
            want = relayout_tokens(one, mem_rows, fine_rows, L, nlb, with_frames=wf)
            assert got.shape == want.shape, (label, L, wf)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, f"{label} {L} with_frames={wf}: {bad.size} rows differ, first {bad[:5]}"
            assert info["memory_rows"][1] - 10 == mem_rows + (mem_rows // PERIOD[L] if PERIOD[L] else 0)


@pytest.mark.parametrize("D,mode,M,T", [(1024, "bf16", 8, 40), (3584, "bf16", 8, 40), (1024, "fp16", 8, 40), (896, "bf16", 8, 40),
                                        (1024, "bf16", 64, 64)])
def test_layouts_bit_identical_to_one_token_relaid(D, mode, M, T):
    """Single videos, each shape with its long video and with an 8-frame one (a single memory).  M = 8 at D = 1024 / 896: the fuser's
    second GEMM runs on the 128^2 kernel (two memories) or through the split-K reduce (one) - writers without a row map: scratch
    + copy; D = 3584 with two memories: the 128 x 256 kernel scatters the rows itself; M = 64: the persistent 256^2 kernel (two
    memories per launch) and the plain 256-column-tile kernel (one) do."""
    model, _ = make_host(D, M, mode, seed=D + M)
    mp, fp = prompts(D, mode)
    with torch.no_grad():
        check_layouts(model, frames(T, D, 4000 + D, mode), torch.arange(T), mp, fp, f"D={D} {mode} M={M} T={T}")
        check_layouts(model, frames(8, D, 4100 + D, mode), torch.arange(8) * 3, mp, fp, f"D={D} {mode} M={M} T=8")
        with pytest.raises(AttributeError, match="image_newline"):
            arch.video_memory_tokens(model, frames(2, D, 1, mode), torch.arange(2), mp, fp, None, layout="grid")
        with pytest.raises(ValueError, match="unknown token layout"):
            arch.video_memory_tokens(model, frames(2, D, 1, mode), torch.arange(2), mp, fp, model.image_newline, layout="rows")


def test_grid_layout_vs_oracle():
    """Independent of the "one_token" run: the `grid` block against relayout(O.video_tokens(...)) at D = 1024, M = 8, 40 frames,
    with the gates of test_video_tokens_vs_oracle - chain_tol on the memory rows, 1e-6 on the literal and fine rows."""
    cfg = O.PathConfig(hidden=1024, heads=8, mem_tokens=8, depth=2)
    w = O.make_weights(cfg, seed=8)
    model, _ = make_host(1024, 8)
    load_oracle_weights(model, w)
    rows = sorted(set(O.MEM_PROMPT_IDS + O.FRAME_PROMPT_IDS))
    emb = np.zeros((48900, 1024), np.float32)
    emb[rows] = O.bf16_round(O.hash_normal_like((len(rows), 1024), 81, 0.02))
    T = 40
    x = O.bf16_round(O.hash_normal_like((T, P, 1024), 82))
    idx = O.subsample_indices(45)[:T]
    toks = O.video_tokens(x, idx, cfg, w, emb, "bf16")
    with O.accumulate_in(np.float64):
        toks64 = O.video_tokens(x, idx, cfg, w, emb, "bf16")
    nl = O.bf16_round(np.asarray(w["image_newline"], np.float32))
    assert float(np.abs(nl).min()) > 0
    mem_rows, fine_rows = 2 * 1568, 32 * P
    want, want64 = (relayout_tokens(t, mem_rows, fine_rows, "grid", nl) for t in (toks, toks64))
    mp, fp = to_dev(emb[list(O.MEM_PROMPT_IDS)]), to_dev(emb[list(O.FRAME_PROMPT_IDS)])
    with torch.no_grad():
        got, info = arch.video_memory_tokens(model, to_dev(x), torch.from_numpy(idx), mp, fp, model.image_newline, layout="grid")
    g = to_np(got)
    a, b = info["memory_rows"]
    assert (a, b) == (10, 10 + mem_rows + mem_rows // 14) and g.shape == want.shape
    is_nl = (np.arange(b - a) % 15) == 14
    floor = O.rel_l2(want64[a:b][~is_nl], want[a:b][~is_nl])
    err = O.rel_l2(g[a:b][~is_nl], want[a:b][~is_nl])
    print(f"grid layout, fused memory rows: HIP vs oracle {err:.2e}, noise floor {floor:.2e}")
    assert err < chain_tol(floor)
    np.testing.assert_array_equal(g[:a], want[:a])
    np.testing.assert_array_equal(g[a:b][is_nl], want[a:b][is_nl])
    assert O.rel_l2(g[b:], want[b:]) < 1e-6


def test_row_batch_and_pool_layouts():
    """video_memory_tokens_batched (B = 2) and MemoryPathPool(batch=2): each layout, per video, equals the same call's "one_token"
    result relaid out, bit for bit (row-batch map and newline gap composed in the GEMM's output-row map)."""
    D, M, T, B = 1024, 8, 40, 2
    model, _ = make_host(D, M, seed=3)
    mp, fp = prompts(D)
    nlb = bits(model.image_newline)
    mem_rows, fine_rows = 2 * M * P, 32 * P
    vids = [frames(T, D, 4300 + i) for i in range(4)]
    idx = torch.arange(T)
    with torch.no_grad():
        bp = BatchedProjector(model.recurrent_memory_transformer, B)
        for wf in (True, False):
            one = bits(arch.video_memory_tokens_batched(model, bp, vids[:B], idx, mp, fp, model.image_newline, with_frames=wf)[0])
            for L in OTHERS:
                rows = arch.video_token_rows(T, M, with_frames=wf, layout=L)
                buf = torch.full((B * rows + 2 * PAD, D), SENTINEL, device="cuda", dtype=torch.int16).view(torch.bfloat16)
                arch.video_memory_tokens_batched(model, bp, vids[:B], idx, mp, fp, model.image_newline, with_frames=wf,
                                                 out=buf[PAD:PAD + B * rows].view(B, rows, D), layout=L)
                torch.cuda.synchronize()
                b = bits(buf)
                assert (b[:PAD] == SENTINEL).all() and (b[PAD + B * rows:] == SENTINEL).all()
                for v in range(B):
                    want = relayout_tokens(one[v], mem_rows, fine_rows, L, nlb, with_frames=wf)
                    assert np.array_equal(b[PAD + v * rows:PAD + (v + 1) * rows], want), (L, wf, v)
        pool = arch.MemoryPathPool(model, 2, batch=2)
        videos = [(v, idx) for v in vids]
        ones = [bits(t) for t in pool.run(videos, mp, fp, model.image_newline)]
        grids = pool.run(videos, mp, fp, model.image_newline, layout="grid")
        torch.cuda.synchronize()
        for i in range(4):
            assert np.array_equal(bits(grids[i]), relayout_tokens(ones[i], mem_rows, fine_rows, "grid", nlb)), i


def _outer_host():
    """the toy host of test_prepare_inputs_end_to_end_vs_oracle (fake tower -> bilinear pool -> path -> splice), device weights"""
    D, side, F0 = 1024, 27, 40
    model, hf = make_host(D, 8, seed=9)
    g = torch.Generator(device="cuda").manual_seed(91)
    with torch.no_grad():
        model.embed_tokens = torch.nn.Embedding(48900, D, device="cuda", dtype=torch.bfloat16)
        model.embed_tokens.weight.copy_(0.02 * torch.randn((48900, D), generator=g, device="cuda"))
    table = frames(F0, D, 92)[:, :1].repeat(1, side * side, 1).contiguous()
    table += to_dev(O.hash_normal_like((1, side * side, D), 93))          # (729 distinct patch rows per frame)

    class Tower(torch.nn.Module):
        num_patches_per_side = side

        def forward(self, images):
            return table[images.reshape(-1).long()]

    model.vision_tower = Tower()
    model.mm_projector = torch.nn.Identity()

    class LM(arch.LlavaMetaForCausalLM, torch.nn.Module):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.config = hf
            self.model = model

        def get_model(self):
            return self.model

        @property
        def device(self):
            return torch.device("cuda")

    ids = torch.tensor([[11, 22, arch.IMAGE_TOKEN_INDEX, 33, 44]], device="cuda")
    labels = torch.tensor([[-100, -100, -100, 33, 44]], device="cuda")
    images = [torch.arange(F0, dtype=torch.float32, device="cuda").reshape(F0, 1, 1, 1)]
    return LM().eval(), model, hf, ids, labels, images


def _set(hf, name):
    hf.mm_patch_merge_type, hf.mm_newline_position = name.split("__")[:2]


def test_prepare_inputs_layouts_and_errors():
    """The outer API for every configuration of the golden fixture: shapes, labels, mask and positions as the golden maps imply,
    embeddings = the "one_token" run relaid out (bit for bit), the in-place route = the general splice route, and the reference's
    exception types for the error cases."""
    z, meta = load_golden("g11_layouts.npz")
    lm, model, hf, ids, labels, images = _outer_host()
    am = torch.ones_like(ids)
    pos_in = torch.arange(ids.shape[1], device="cuda")[None]
    nlb = bits(model.image_newline)
    mem_rows, fine_rows = 2 * 8 * P, 32 * P                     # 40 frames -> 64 sampled: two chunks, 32 fine frames
    with torch.no_grad():
        _set(hf, meta["control"])
        one = bits(lm.prepare_inputs_labels_for_multimodal(ids, pos_in, am, None, labels, images, modalities=["video"])[4][0])
        assert one.shape[0] == int(z[f"rows_{meta['control']}_70"])            # (70 input frames sample 64 as well)
        for name in meta["configs"]:
            _set(hf, name)
            L = EXPECTED[name]
            none_ids, pos, mask, pkv, emb, labs = lm.prepare_inputs_labels_for_multimodal(ids, pos_in, am, None, labels, images,
                                                                                          modalities=["video"])
            n = int(z[f"rows_{name}_70"])
            assert none_ids is None and pkv is None and tuple(emb.shape) == (1, n, 1024), name
            np.testing.assert_array_equal(labs[0].cpu().numpy(), z[f"labels_{name}_70"])
            np.testing.assert_array_equal(mask[0].cpu().numpy().astype(bool), z[f"mask_{name}_70"])
            np.testing.assert_array_equal(pos[0].cpu().numpy(), z[f"pos_{name}_70"])
            want = np.concatenate([one[:2], relayout_tokens(one[2:-2], mem_rows, fine_rows, L, nlb), one[-2:]])
            assert np.array_equal(bits(emb[0]), want), name
            # the golden map, applied to the "one_token" run
            m = z[f"map_{name}_70"]
            assert np.array_equal(bits(emb[0]), np.where((m < 0)[:, None], nlb[None, :], one[np.maximum(m, 0)])), name
            # general route (a truncating tokenizer_model_max_length keeps _direct_emit out): same bits, cut
            hf.tokenizer_model_max_length = n - 3
            gen = lm.prepare_inputs_labels_for_multimodal(ids, pos_in, am, None, labels, images, modalities=["video"])
            hf.tokenizer_model_max_length = 32768
            assert torch.equal(gen[4], emb[:, :n - 3]) and torch.equal(gen[5], labs[:, :n - 3]) and gen[4].shape[1] == n - 3
            # ... and uncut: splice_into_text over the tokens of video_memory_tokens
            pooled = lm.get_2dPool(lm.encode_images(images[0][arch.sample_frame_indices(40).cuda()]))
            toks, _ = arch.video_memory_tokens(model, pooled, arch.sample_frame_indices(40),
                                               model.embed_tokens(torch.tensor(arch.MEMORY_PROMPT_IDS, device="cuda")),
                                               model.embed_tokens(torch.tensor(arch.FRAME_PROMPT_IDS, device="cuda")),
                                               model.image_newline, layout=L)
            gen = arch.splice_into_text(lm, model, [toks], ids, pos_in, am, None, labels)
            assert torch.equal(gen[4], emb) and torch.equal(gen[5], labs) and torch.equal(gen[2], mask) and torch.equal(gen[1], pos)
        # error cases: the exception types the reference raised
        errs = {"ValueError": ValueError, "AttributeError": AttributeError}
        for case, tname in meta["errors"].items():
            _set(hf, case)
            saved = model.image_newline
            if case.endswith("nonewline"):
                del model.image_newline
            try:
                with pytest.raises(errs[tname]):
                    lm.prepare_inputs_labels_for_multimodal(ids, pos_in, am, None, labels, images, modalities=["video"])
            finally:
                model.image_newline = saved
        # a layout that inserts nothing works without image_newline
        _set(hf, "spatial__one_token")
        saved = model.image_newline
        del model.image_newline
        try:
            emb = lm.prepare_inputs_labels_for_multimodal(ids, pos_in, am, None, labels, images, modalities=["video"])[4]
        finally:
            model.image_newline = saved
        assert np.array_equal(bits(emb[0]), np.concatenate([one[:2], relayout_tokens(one[2:-2], mem_rows, fine_rows, "no_token", nlb),
                                                            one[-2:]]))
        _set(hf, "spatial_unpad__grid")
        hf.add_faster_video = True
        with pytest.raises(NotImplementedError, match="add_faster_video"):
            lm.prepare_inputs_labels_for_multimodal(ids, pos_in, am, None, labels, images, modalities=["video"])


def test_graphs_keep_layouts_apart():
    """GraphedVideoMemory(layout="grid") replays to the eager grid block; with enable_memory_graphs(2) one video shape served
    alternately as "one_token" and "grid" never returns the other layout's block."""
    lm, model, hf, ids, labels, images = _outer_host()
    am = torch.ones_like(ids)
    D, T = 1024, 40
    mp, fp = prompts(D)
    idx = torch.arange(T)
    with torch.no_grad():
        g = arch.GraphedVideoMemory(model, T, idx, layout="grid")
        for seed in (4500, 4501):
            x = frames(T, D, seed)
            eager, _ = arch.video_memory_tokens(model, x, idx, mp, fp, model.image_newline, layout="grid")
            out = g(x, mp, fp, model.image_newline)
            torch.cuda.synchronize()
            assert out.shape == eager.shape == (arch.video_token_rows(T, 8, layout="grid"), D) and torch.equal(out, eager)
        want = {}
        for name in ("spatial_unpad__one_token", "spatial_unpad__grid"):
            _set(hf, name)
            want[name] = lm.prepare_inputs_labels_for_multimodal(ids, None, am, None, labels, images, modalities=["video"])[4].clone()
        assert want["spatial_unpad__one_token"].shape[1] + 14 * (16 + 32) - 2 == want["spatial_unpad__grid"].shape[1]
        lm.enable_memory_graphs(2)
        for rep in range(4):
            for name in ("spatial_unpad__one_token", "spatial_unpad__grid"):
                _set(hf, name)
                got = lm.prepare_inputs_labels_for_multimodal(ids, None, am, None, labels, images, modalities=["video"])[4]
                assert got.shape == want[name].shape and torch.equal(got, want[name]), (rep, name)
        assert len(lm._mem_graphs) == 2 and sorted(g_.layout for g_ in lm._mem_graphs.values()) == ["grid", "one_token"]


def test_training_tail_layouts_and_newline_gradient():
    """`larimar_model` setting (fuser, token-type embedding and image_newline train, the recurrent transformer is frozen): the
    `grid` / `frame` training tokens are the "one_token" training tokens relaid out bit for bit; image_newline.grad is the float64
    sum of the upstream gradient over the newline rows within 3 x 2^-8 (one 16-bit rounding where the newline enters the memory
    block, one where it enters the fine block, one for their sum; 2^-8 = half an ulp of bf16); the fuser parameters get exactly
    the gradients of the "one_token" run (the loss ignores the row order: the same upstream rows reach the same kernels)."""
    D, M, T = 1024, 8, 40
    model, _ = make_host(D, M, seed=11)
    model.train()
    for n_, p_ in model.named_parameters():
        p_.requires_grad_(not n_.startswith("recurrent_memory_transformer") and not n_.startswith("embed_tokens"))
    mp, fp = prompts(D)
    x, idx = frames(T, D, 4600), torch.arange(T)
    mem_rows, fine_rows = 2 * M * P, 32 * P
    runs = {}
    for L in ("one_token", "grid", "frame"):
        model.zero_grad(set_to_none=True)
        toks, info = arch.video_memory_tokens(model, x, idx, mp, fp, model.image_newline, layout=L)
        assert toks.requires_grad and model.recurrent_memory_transformer._cache_mode == "engine"
        toks.float().square().sum().backward()
        torch.cuda.synchronize()
        runs[L] = (bits(toks), toks.detach().double(), {n_: p_.grad.clone() for n_, p_ in model.named_parameters() if p_.requires_grad})
        assert all(g_ is not None for g_ in runs[L][2].values())
    one = runs["one_token"][0]
    nlb = bits(model.image_newline)
    for L in ("grid", "frame"):
        got, tok64, grads = runs[L]
        assert np.array_equal(got, relayout_tokens(one, mem_rows, fine_rows, L, nlb)), L
        is_nl = relayout_tokens(np.arange(one.shape[0], dtype=np.int64).reshape(-1, 1), mem_rows, fine_rows, L, np.array([-1]))[:, 0] < 0
        assert int(is_nl.sum()) == (mem_rows + fine_rows) // PERIOD[L]
        want = (2.0 * tok64[torch.from_numpy(is_nl).cuda()]).sum(0)             # d/dt sum t^2 over the newline rows, float64
        err = float((grads["image_newline"].double() - want).norm() / want.norm())
        print(f"{L}: image_newline.grad vs float64 sum over {int(is_nl.sum())} rows: rel-L2 {err:.2e}")
        assert err <= 3 * 2.0 ** -8, (L, err)
        for n_ in grads:
            if n_.startswith("memory_fuser"):
                assert torch.equal(grads[n_], runs["one_token"][2][n_]), (L, n_)
