"""Several videos per forward, the host side (no GPU): how videos are grouped into row batches, where everything of a padded batch
of samples lands when the blocks are emitted in place (`VideoPlacement` against `splice_into_text`, exactly), which inputs are
refused, and the binding of the export that takes one destination per video."""
import ctypes
import os
import types

import pytest
import torch

import memory_augmented_vlm_amd  # noqa: F401
from memory_augmented_vlm_amd import _capi as capi
from memory_augmented_vlm_amd.model import llava_arch as arch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = arch.IMAGE_TOKEN_INDEX
D = 16


def test_grouping_cuts_equal_lengths_into_8_4_2_and_keeps_input_order():
    counts = [64, 64, 96, 64, 20, 64, 64, 64, 64, 64, 64, 64]
    batches, singles = arch.plan_row_batches(counts)
    assert batches == [[0, 1, 3, 5, 6, 7, 8, 9], [10, 11]]          # the ten 64s: 8 + 2, non-consecutive members, input order
    assert singles == [2, 4]
    assert sorted(i for b in batches for i in b) + singles == sorted(set(range(12)) - {2, 4}) + [2, 4]
    assert arch.LlavaMetaForCausalLM.row_batch_sizes == (8, 4, 2) == arch.ROW_BATCH_SIZES
    # overridden sizes: 10 = 4 + 4 + (2 left as singles); 3 + 3 + 3 + 1
    assert arch.plan_row_batches(counts, (4,)) == ([[0, 1, 3, 5], [6, 7, 8, 9]], [2, 4, 10, 11])
    assert arch.plan_row_batches(counts, (3,)) == ([[0, 1, 3], [5, 6, 7], [8, 9, 10]], [2, 4, 11])
    assert arch.plan_row_batches([7, 7, 7, 7, 7, 7, 7]) == ([[0, 1, 2, 3], [4, 5]], [6])          # 7 = 4 + 2 + 1
    assert arch.plan_row_batches([5]) == ([], [0]) and arch.plan_row_batches([]) == ([], [])
    # results come back in input order whatever ran together
    order = [None] * 12
    for b in batches:
        for i in b:
            order[i] = ("batch", counts[i])
    for i in singles:
        order[i] = ("single", counts[i])
    assert [o[1] for o in order] == counts
    with pytest.raises(ValueError):
        arch.plan_row_batches(counts, (32,))                          # the batched emit takes 16 videos per launch


class _Emb(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.embed_tokens = torch.nn.Embedding(100, D)
        with torch.no_grad():
            self.embed_tokens.weight.copy_(torch.randn((100, D), generator=g))


def _lm(side, max_tok):
    return types.SimpleNamespace(config=types.SimpleNamespace(tokenizer_padding_side=side, tokenizer_model_max_length=max_tok),
                                 training=False)


def _batch():
    """five samples, right-padded with 0 behind an attention mask: image token first / in the middle / last, a text-only
    sample (position 3: `splice_into_text` advances its feature index over it), prompts of different lengths"""
    rows = [[IMG, 11, 12, 13], [21, 22, IMG, 23, 24, 25, 26], [31, 32, 33, IMG], [41, 42, 43, 44, 45], [51, IMG, 52]]
    L = max(len(r) for r in rows)
    ids = torch.tensor([r + [0] * (L - len(r)) for r in rows])
    mask = torch.tensor([[1] * len(r) + [0] * (L - len(r)) for r in rows])
    labels = torch.where(ids == IMG, torch.tensor(arch.IGNORE_INDEX), ids + 1000)
    return rows, ids, mask, labels


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("with_optional", [True, False])
def test_placement_plan_equals_splice_into_text(side, with_optional):
    rows, ids, mask, labels = _batch()
    g = torch.Generator().manual_seed(5)
    block_rows = [7, 3, 12, 5]                                       # the four videos, in the order of the samples that hold them
    feats = [torch.randn((r, D), generator=g) for r in block_rows]
    model, lm = _Emb(), _lm(side, 64)
    pos_in = torch.arange(ids.shape[1])[None].expand(ids.shape[0], -1)
    plan = arch.VideoPlacement([r for r in rows], block_rows, left=side == "left", max_tok=64)
    assert not plan.general and plan.video_of == [0, 1, 2, -1, 3] and plan.image_at == [0, 2, 3, -1, 1]
    am, po, la = (mask, pos_in, labels) if with_optional else (None, None, None)
    if am is None:                                                    # (without a mask every position counts: no padding ids)
        ids = torch.tensor([r + [60] * (ids.shape[1] - len(r)) for r in rows])
        plan = arch.VideoPlacement(ids, block_rows, left=side == "left", max_tok=64)
    with torch.no_grad():
        want = arch.splice_into_text(lm, model, arch.features_per_sample(plan.video_of, feats), ids, po, am, None, la)
    w_pos, w_mask, w_emb, w_lab = want[1], want[2], want[4], want[5]
    B, L = w_emb.shape[:2]
    assert plan.Lmax == L and len(plan.lengths) == B
    # the buffer the in-place route fills: padding zeroed, text rows from the segments, block v at row dst_row[v] of [B * L, D]
    emb = torch.full((B, L, D), float("nan"))
    for s, lo, hi in plan.padding:
        emb[s, lo:hi] = 0
    id_list = [ids[s][mask[s].bool()] if am is not None else ids[s] for s in range(B)]
    with torch.no_grad():
        for s, lo, hi, row in plan.segments:
            emb[s, row:row + hi - lo] = model.embed_tokens(id_list[s][lo:hi])
    flat = emb.view(B * L, D)
    for v, f in enumerate(feats):
        assert torch.isnan(flat[plan.dst_row[v]:plan.dst_row[v] + f.shape[0]]).all()       # blocks overlap nothing
        flat[plan.dst_row[v]:plan.dst_row[v] + f.shape[0]] = f
    assert torch.equal(emb, w_emb)
    lab_list = None if la is None else [labels[s][mask[s].bool()] for s in range(B)]
    g_lab, g_mask, g_pos = plan.labels_mask_positions(lab_list, am, po)
    for got, ref in ((g_lab, w_lab), (g_mask, w_mask), (g_pos, w_pos)):
        assert (got is None) == (ref is None)
        if ref is not None:
            assert got.dtype == ref.dtype and torch.equal(got, ref)
    if side == "left":
        assert all(st + n == L for st, n in zip(plan.starts, plan.lengths))
    else:
        assert plan.starts == [0] * B


def test_placement_plan_reports_the_general_path_when_a_sample_is_cut():
    rows, ids, mask, labels = _batch()
    block_rows = [7, 3, 12, 5]
    plan = arch.VideoPlacement(rows, block_rows, left=False, max_tok=14)       # sample 2 has 3 + 12 = 15 rows
    assert plan.general and plan.lengths == [10, 9, 14, 5, 7] and plan.Lmax == 14
    assert not arch.VideoPlacement(rows, block_rows, left=False, max_tok=15).general
    assert arch.VideoPlacement(rows, block_rows, left=False, max_tok=None).Lmax == 15
    # the cut sequence itself is `splice_into_text`'s: same padded length
    g = torch.Generator().manual_seed(6)
    feats = [torch.randn((r, D), generator=g) for r in block_rows]
    with torch.no_grad():
        out = arch.splice_into_text(_lm("right", 14), _Emb(), arch.features_per_sample(plan.video_of, feats), ids, None, mask, None,
                                    labels)
    assert out[4].shape[1] == plan.Lmax


def test_placement_plan_refuses_what_is_not_one_video_per_sample():
    with pytest.raises(NotImplementedError, match="one video"):
        arch.VideoPlacement([[1, IMG, 2, IMG]], [4, 4])                          # two image tokens in one sample
    with pytest.raises(NotImplementedError, match="one video per sample"):
        arch.VideoPlacement([[1, IMG, 2]], [4, 4])                               # two videos, one sample
    with pytest.raises(NotImplementedError, match="one video"):
        arch.VideoPlacement([[1, IMG], [IMG, 3], [4, IMG]], [4, 4])              # three samples with a token, two videos


def _cpu_lm():
    """the toy host of tests/test_host_cpu.py (CPU tower; the memory path itself needs a GPU and is never reached here)"""
    H, NP = 32, 9

    class Tower(torch.nn.Module):
        num_patches_per_side = 3

        def forward(self, images):
            return images.flatten(1)[:, :NP * H].reshape(images.shape[0], NP, H)

    class Base(torch.nn.Module):
        def __init__(self, config):
            super().__init__()
            self.embed_tokens = torch.nn.Embedding(49000, H)

    class Inner(arch.LlavaMetaModel, Base):
        pass

    class LM(arch.LlavaMetaForCausalLM, torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.config = types.SimpleNamespace(hidden_size=H, mm_patch_merge_type="spatial_unpad", mm_newline_position="one_token",
                                                mm_spatial_pool_mode="bilinear", tokenizer_model_max_length=4096,
                                                tokenizer_padding_side="right")
            self.model = Inner(self.config)
            self.model.vision_tower = Tower()
            self.model.mm_projector = torch.nn.Identity()
            self.model.image_newline = torch.nn.Parameter(torch.zeros(H))
            self.draws = 0

        def get_model(self):
            return self.model

        def get_synced_dropout_decision(self, prob=0.5):
            self.draws += 1
            return False

        @property
        def device(self):
            return torch.device("cpu")

    torch.manual_seed(0)
    return LM().eval()


def test_entry_point_refusals_and_the_single_video_call():
    lm = _cpu_lm()
    video = torch.randn(2, 3, 10, 10)
    one = torch.tensor([[5, 6, IMG, 7]])
    two = torch.tensor([[5, 6, IMG, 7], [IMG, 8, 9, 10]])
    twice = torch.tensor([[5, IMG, 6, IMG], [7, 8, 9, 10]])
    call = lambda ids, n: lm.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [video] * n, modalities=["video"] * n)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="one video"):      # two videos for one sample (tests/test_host_cpu.py's case)
            call(one, 2)
        with pytest.raises(NotImplementedError, match="one video per sample"):
            call(twice, 2)                                               # two image tokens in one sample
        with pytest.raises(NotImplementedError, match="one video per sample"):
            call(two, 3)                                                 # three videos, two samples
        assert lm.draws == 0                                             # refused before anything is encoded or drawn
        # V == 1 is today's path: it reaches the memory path, which has no CPU fallback - with one sample and with two samples
        # sharing the video, as before
        for ids in (one, two):
            with pytest.raises(capi.MavlmError, match="not on a GPU"):
                call(ids, 1)
        assert lm.draws == 2
        # V == 2, paired: accepted by the host logic, one draw, and then the same "no CPU fallback" error from the path
        with pytest.raises(capi.MavlmError, match="GPU"):
            call(two, 2)
        assert lm.draws == 3


def test_new_export_is_bound_and_declared():
    l = capi.lib()
    assert l.mavlm_abi_version() == 3                                    # additive: the ABI version stays
    name = "mavlm_fuse_emit_layout_batch_to"
    assert name in capi.SIGNATURES and hasattr(ctypes.CDLL(l._name), name)
    res, args = capi.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == 16 and args[13] is ctypes.POINTER(ctypes.c_int64)     # dst_row: host int64[B]
    hdr = open(os.path.join(ROOT, "include", "mavlm.h")).read()
    assert "int mavlm_fuse_emit_layout_batch_to(mavlm_ctx* ctx" in hdr and "const int64_t* dst_row" in hdr
    assert "#define MAVLM_ABI_VERSION 3" in hdr
    rows = ctypes.c_int64(0)
    dst = (ctypes.c_int64 * 2)(0, 0)
    assert l.mavlm_fuse_emit_layout_batch_to(None, None, None, 0, None, 0, None, 0, None, 1, 0, None, 0, dst, ctypes.byref(rows),
                                             None) == capi.E_ARG
