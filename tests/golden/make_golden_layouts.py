#!/usr/bin/env python3
"""Golden video token layouts (g11_layouts.npz): the reference's own `prepare_inputs_labels_for_multimodal` under every
mm_patch_merge_type / mm_newline_position combination the memory branch can take (llava_arch.py:562-634).

Runs ONLY where the reference is present (as make_golden.py, whose import recipe it uses; make_golden.py is not touched).  The
toy host is the one of G6 (make_golden.py g5_g6: D = 32, weights seed 61, embedding seed 62, frame features seed 600 + F0), so
the control configuration ("spatial_unpad", "one_token") must reproduce what g6_glue.npz stores for the same video - the
generator stops if it does not.

Per video (8 and 70 input frames: one chunk with 8 fine frames / two chunks with 32 fine frames) and configuration the fixture
holds the row count, an int32 map from every output row to its row in the control output (-1 = an inserted newline row; found
by exact fp32 row equality in row order - the reference run is deterministic on the CPU), every 13th row, and the label, mask and position
vectors; for the three error cases the name of the exception type the reference raises.

The file is written with fixed zip timestamps: it regenerates bit-identically.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_layouts.py
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (loads the reference's files at run time)
from make_golden import O  # noqa: E402

D, VOCAB, SIDE = 32, 48900, 27
WSEED, EMBSEED, FEATSEED0 = 61, 62, 600
TEXT_IDS = [11, 22, 33, 44]
VIDEOS = (8, 70)
ROWSTEP = 13
CONTROL = ("spatial_unpad", "one_token")
CONFIGS = (CONTROL, ("spatial_unpad", "grid"), ("spatial_unpad", "frame"), ("spatial_unpad", "no_token"),
           ("spatial", "one_token"), ("flat", "grid"))
# (merge type, newline position, host has image_newline)
ERROR_CASES = (("spatial_unpad", "bogus", True), ("bogus", "grid", True), ("spatial", "grid", False))


def cfg_name(merge, pos):
    return f"{merge}__{pos}"


def build_host():
    """the toy host of G6 (make_golden.py g5_g6), restated"""
    LlavaMetaModel, LlavaMetaForCausalLM = G.import_glue()

    class Cfg:
        hidden_size = D
        mm_patch_merge_type = CONTROL[0]
        mm_newline_position = CONTROL[1]
        mm_spatial_pool_mode = "bilinear"
        image_aspect_ratio = "anyres_max_9"
        tokenizer_model_max_length = 32768
        tokenizer_padding_side = "right"

    class FakeTower(nn.Module):
        num_patches_per_side = SIDE

        def __init__(self):
            super().__init__()
            self.table = None

        def forward(self, images):  # images [F,1,1,1] holding the original frame id
            return self.table[images.reshape(-1).long()]

    class TinyBase(nn.Module):
        def __init__(self, config):
            super().__init__()
            self.embed_tokens = nn.Embedding(VOCAB, D)

        @property
        def device(self):
            return torch.device("cpu")

        @property
        def dtype(self):
            return torch.float32

    class TinyModel(LlavaMetaModel, TinyBase):
        pass

    class TinyLM(LlavaMetaForCausalLM, nn.Module):
        def __init__(self):
            nn.Module.__init__(self)
            self.config = Cfg()
            self.model = TinyModel(self.config)
            self.model.vision_tower = FakeTower()
            self.model.mm_projector = nn.Identity()
            self.model.image_newline = nn.Parameter(torch.zeros(D))

        def get_model(self):
            return self.model

        @property
        def device(self):
            return torch.device("cpu")

    cfg = O.PathConfig(hidden=D, heads=8, mem_tokens=8, depth=2)
    w = O.make_weights(cfg, seed=WSEED)
    lm = TinyLM().eval().float()
    sd = lm.model.state_dict()
    for k, v in w.items():
        if k in sd:
            sd[k].copy_(G.T(v))
    rows = sorted(set(O.MEM_PROMPT_IDS + O.FRAME_PROMPT_IDS + TEXT_IDS))
    emb = np.zeros((VOCAB, D), dtype=np.float32)
    emb[rows] = O.bf16_round(O.hash_normal_like((len(rows), D), EMBSEED, 0.02))
    lm.model.embed_tokens.weight.copy_(G.T(emb))
    lm.model.image_newline.copy_(G.T(w["image_newline"]))
    return lm, np.asarray(w["image_newline"], dtype=np.float32)


def run(lm, F0, merge, pos):
    lm.config.mm_patch_merge_type, lm.config.mm_newline_position = merge, pos
    feats = O.bf16_round(O.hash_normal_like((F0, SIDE * SIDE, D), FEATSEED0 + F0))
    lm.model.vision_tower.table = G.T(feats)
    images = [torch.arange(F0, dtype=torch.float32).reshape(F0, 1, 1, 1)]
    input_ids = torch.tensor([[11, 22, -200, 33, 44]])
    labels = torch.tensor([[-100, -100, -100, 33, 44]])
    am = torch.ones_like(input_ids)
    position_ids = torch.arange(input_ids.shape[1])[None]
    lm.get_model().recurrent_memory_transformer.frame_attn_scores = []
    _, p, mask, _, embeds, labs = lm.prepare_inputs_labels_for_multimodal(input_ids, position_ids, am, None, labels, images,
                                                                          modalities=["video"])
    return embeds[0].numpy(), labs[0].numpy(), mask[0].numpy(), p[0].numpy()


def row_map(out, ctl, newline):
    """int32 map out row -> control row (-1 = newline), by exact equality of the fp32 rows.  The two prompts share three token
    ids ("the", " video", ":"), so six prompt rows have a twin: a layout keeps the order of the rows, and a row with a twin goes
    to the first equal control row behind the previous match.  Every other control row is unique."""
    is_nl = np.array([r.tobytes() == newline.tobytes() for r in ctl])
    assert int(is_nl.sum()) == 2, "the control output has exactly two newline rows"
    where = {}
    for i, r in enumerate(ctl):
        if not is_nl[i]:
            where.setdefault(r.tobytes(), []).append(i)
    twins = sorted(i for v in where.values() if len(v) > 1 for i in v)
    assert len(twins) <= 6 and all(len(v) <= 2 for v in where.values()), f"unexpected equal control rows {twins}"
    m = np.full(out.shape[0], -1, dtype=np.int32)
    hits = np.zeros(ctl.shape[0], dtype=np.int64)
    prev = -1
    for i, r in enumerate(out):
        cand = where.get(r.tobytes())
        if cand is None:
            assert r.tobytes() == newline.tobytes(), f"output row {i} is neither a control row nor image_newline"
            continue
        later = [j for j in cand if j > prev]
        assert later, f"output row {i} repeats or reorders control row {cand}"
        prev = m[i] = later[0]
        hits[prev] += 1
    assert (hits[~is_nl] == 1).all(), "every control row except its newlines appears exactly once"
    return m


def save_deterministic(name, arrs):
    """np.savez_compressed with fixed zip timestamps (numpy stamps the members with the wall clock)"""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrs[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    lm, newline = build_host()
    assert float(np.abs(newline).min()) > 0.0
    g6 = np.load(os.path.join(HERE, "g6_glue.npz"))
    g6step = {8: 1, 70: 13}
    arrs = {}
    for F0 in VIDEOS:
        ctl, clab, cmask, cpos = run(lm, F0, *CONTROL)
        # the control is the G6 run of the same video
        assert ctl.shape[0] == int(g6[f"rows_{F0}"])
        assert np.array_equal(ctl[::g6step[F0]], g6[f"embeds_{F0}"]), "control differs from g6_glue.npz"
        assert np.array_equal(ctl.astype(np.float64).sum(axis=1), g6[f"rowsum_{F0}"]), "control differs from g6_glue.npz"
        for merge, pos in CONFIGS:
            out, lab, mask, p = (ctl, clab, cmask, cpos) if (merge, pos) == CONTROL else run(lm, F0, merge, pos)
            m = row_map(out, ctl, newline)
            k = f"{cfg_name(merge, pos)}_{F0}"
            arrs[f"rows_{k}"] = np.array(out.shape[0], dtype=np.int64)
            arrs[f"map_{k}"] = m
            arrs[f"embeds_{k}"] = out[::ROWSTEP].copy()
            arrs[f"labels_{k}"] = lab.astype(np.int32)
            arrs[f"mask_{k}"] = mask.astype(np.bool_)
            arrs[f"pos_{k}"] = p.astype(np.int32)
            print(f"F0 = {F0:3d}  {merge:14s} {pos:10s} rows {out.shape[0]:6d}  newline rows {int((m < 0).sum())}")
    errors = {}
    for merge, pos, has_newline in ERROR_CASES:
        host, _ = (lm, None) if has_newline else build_host()
        if not has_newline:
            del host.model.image_newline
        try:
            run(host, VIDEOS[0], merge, pos)
            raise AssertionError(f"{merge} / {pos}: the reference raised nothing")
        except (ValueError, AttributeError, NotImplementedError, IndexError, TypeError, RuntimeError) as e:
            errors[f"{cfg_name(merge, pos)}__{'newline' if has_newline else 'nonewline'}"] = type(e).__name__
            print(f"{merge} / {pos} / image_newline {has_newline}: {type(e).__name__}: {str(e)[:100]}")
    arrs["image_newline"] = newline
    arrs["meta"] = G.meta(D=D, side=SIDE, wseed=WSEED, embseed=EMBSEED, featseed0=FEATSEED0, text_ids=TEXT_IDS,
                          videos=list(VIDEOS), rowstep=ROWSTEP, control=cfg_name(*CONTROL),
                          configs=[cfg_name(*c) for c in CONFIGS], errors=errors, n_text=len(TEXT_IDS), image_pos=2)
    save_deterministic("g11_layouts.npz", arrs)


if __name__ == "__main__":
    main()
