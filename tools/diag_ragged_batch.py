"""Diagnostic (GPU box): ragged row batches through the model entry point.  Eight videos of MIXED chunk counts (2, 2, 3, 3, 4, 4,
6, 8 chunks of 32 sampled frames) at M = 8, hidden 1024 and 896, bf16, a toy tower of 27 x 27 patches (table lookup) in front of
the HIP pool:
  * `prepare_inputs_labels_for_multimodal` with `enable_ragged_row_batches()` on against off (off: equal lengths pair up, the rest
    run as single videos) - same process, interleaved, medians of 7 rounds;
  * one deliberately lopsided pair, 2 and 16 chunks, stepped as ONE ragged batch of two (the planner's half rule bypassed: the
    long video runs 14 of its 16 steps alone on the row-batch schedule) against the two videos as singles: what the
    lone-survivor stretch costs.
usage: python tools/diag_ragged_batch.py"""
import os
import sys
import time
import types
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from memory_augmented_vlm_amd import _capi as capi  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
CHUNKS, M, SIDE, ROUNDS, TABLE = (2, 2, 3, 3, 4, 4, 6, 8), 8, 27, 7, 256
V = len(CHUNKS)


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def run(hidden):
    model, arch = bench.build_model(dev, hidden=hidden, mem_tokens=M, seed=4321)
    g = torch.Generator(device="cpu").manual_seed(100)
    table = (torch.randn((TABLE, 1, hidden), generator=g) + torch.randn((1, SIDE * SIDE, hidden), generator=g)).to(dev).to(torch.bfloat16)

    class Tower(torch.nn.Module):
        num_patches_per_side = SIDE

        def forward(self, images):
            return table[images.reshape(-1).long()]

    model.vision_tower, model.mm_projector = Tower(), torch.nn.Identity()

    class LM(arch.LlavaMetaForCausalLM, torch.nn.Module):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.config = types.SimpleNamespace(hidden_size=hidden, mm_patch_merge_type="spatial_unpad", mm_newline_position="one_token",
                                                mm_spatial_pool_mode="bilinear", tokenizer_model_max_length=1 << 20,
                                                tokenizer_padding_side="left")
            self.model = model

        def get_model(self):
            return self.model

        @property
        def device(self):
            return dev

    lm = LM().eval()
    # input frame counts that the sampler turns into exactly c chunks of 32 (c * 32 input frames: every frame is kept)
    videos = [((torch.arange(32 * c) + 7 * v) % TABLE).to(torch.float32).reshape(32 * c, 1, 1, 1).to(dev) for v, c in enumerate(CHUNKS)]
    assert [arch.sample_frame_count(32 * c) for c in CHUNKS] == [32 * c for c in CHUNKS]
    lens = [6 + 3 * v for v in range(V)]
    L = max(lens)
    ids = torch.full((V, L), 17, device=dev)
    mask = torch.zeros((V, L), dtype=torch.long, device=dev)
    for v, n in enumerate(lens):
        ids[v, L - n + n // 2] = arch.IMAGE_TOKEN_INDEX
        mask[v, L - n:] = 1
    mods = ["video"] * V
    frames = 32 * sum(CHUNKS)

    def call():
        return lm.prepare_inputs_labels_for_multimodal(ids, None, mask, None, None, videos, mods)

    res = {True: [], False: []}
    with torch.no_grad():
        for on in (False, True, False, True):
            lm.enable_ragged_row_batches(on)
            call()
        for _ in range(ROUNDS):
            for on in (True, False):
                lm.enable_ragged_row_batches(on)
                res[on].append(timed(call, 3))
    lm.enable_ragged_row_batches(False)
    m_on, m_off = median(res[True]), median(res[False])
    plan = arch.plan_ragged_batches([32 * c for c in CHUNKS])
    print(f"D={hidden} M={M}: {V} videos of {CHUNKS} chunks through the entry point | ragged on {m_on * 1e3:8.4f} ms "
          f"({frames / m_on / 1e3:.1f} k frames/s) | off {m_off * 1e3:8.4f} ms ({frames / m_off / 1e3:.1f} k frames/s) | "
          f"ratio off / on {m_off / m_on:.3f}  (spread on {min(res[True]) * 1e3:.4f}-{max(res[True]) * 1e3:.4f}, off "
          f"{min(res[False]) * 1e3:.4f}-{max(res[False]) * 1e3:.4f}); groups {plan[0]}", flush=True)

    # ---- the lopsided pair: 2 and 16 chunks as one ragged batch of two (half rule bypassed) against two singles
    rm = model.recurrent_memory_transformer
    with torch.no_grad():
        mp = model.embed_tokens(torch.tensor(arch.MEMORY_PROMPT_IDS, device=dev)).contiguous()
        fp = model.embed_tokens(torch.tensor(arch.FRAME_PROMPT_IDS, device=dev)).contiguous()
        pair = []
        for v, c in enumerate((2, 16)):
            vid = ((torch.arange(32 * c) + 11 * v) % TABLE).to(torch.float32).reshape(32 * c, 1, 1, 1).to(dev)
            idx = arch.sample_frame_indices(32 * c)
            pair.append((lm.get_2dPool(lm.encode_images(vid[idx.to(dev)])), idx))
        bp = rm.row_batcher(2)

        def together():
            arch.video_memory_tokens_batched(model, bp, [p for p, _ in pair], [i for _, i in pair], mp, fp, model.image_newline,
                                             ragged=True)

        def apart():
            for p, i in pair:
                arch.video_memory_tokens(model, p, i, mp, fp, model.image_newline)

        res = {"together": [], "apart": []}
        for _ in range(2):
            together(); apart()
        for _ in range(ROUNDS):
            res["together"].append(timed(together, 3))
            res["apart"].append(timed(apart, 3))
    mt, ma = median(res["together"]), median(res["apart"])
    print(f"D={hidden} M={M}: lopsided pair (2 and 16 chunks) | one ragged batch of two {mt * 1e3:8.4f} ms | two singles "
          f"{ma * 1e3:8.4f} ms | ratio singles / batch {ma / mt:.3f}  (spread {min(res['together']) * 1e3:.4f}-"
          f"{max(res['together']) * 1e3:.4f}, {min(res['apart']) * 1e3:.4f}-{max(res['apart']) * 1e3:.4f})", flush=True)


for hidden in (1024, 896):
    try:
        run(hidden)
    except capi.MavlmError as e:          # (a width whose row-batched emit the GEMM kernels refuse is reported, not hidden)
        print(f"D={hidden} M={M}: not run - {e}", flush=True)
