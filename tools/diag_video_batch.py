"""Diagnostic (GPU box): several videos per forward through the model entry point.  8 videos of 64 frames at M = 8, hidden 1024
and 896, bf16, a toy tower of 27 x 27 patches (table lookup) in front of the HIP pool:
  * `prepare_inputs_labels_for_multimodal` with 8 samples in ONE call (one row batch of 8, blocks emitted into the padded buffer)
    against eight single-sample calls (the single-video path, `_direct_emit`) - same process, interleaved, medians of 7 rounds;
  * placement alone: `mavlm_fuse_emit_layout_batch_to` straight into the padded buffer against `mavlm_fuse_emit_layout_batch` into a
    staging buffer plus one copy per video, on the same context and state;
  * workspace bytes of the three batched engines the model caches (row batches of 8, 4 and 2).
usage: python tools/diag_video_batch.py"""
import ctypes
import os
import sys
import time
import types
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from memory_augmented_vlm_amd import _capi as capi  # noqa: E402
from memory_augmented_vlm_amd import _ops as ops  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
V, FRAMES, M, SIDE, ROUNDS = 8, 64, 8, 27, 7


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


for hidden in (1024, 896):
    model, arch = bench.build_model(dev, hidden=hidden, mem_tokens=M, seed=4321)
    g = torch.Generator(device="cpu").manual_seed(100)
    table = (torch.randn((FRAMES, 1, hidden), generator=g) + torch.randn((1, SIDE * SIDE, hidden), generator=g)).to(dev).to(torch.bfloat16)

    class Tower(torch.nn.Module):
        num_patches_per_side = SIDE

        def forward(self, images):
            return table[images.reshape(-1).long()]

    model.vision_tower, model.mm_projector = Tower(), torch.nn.Identity()

    class LM(arch.LlavaMetaForCausalLM, torch.nn.Module):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.config = types.SimpleNamespace(hidden_size=hidden, mm_patch_merge_type="spatial_unpad", mm_newline_position="one_token",
                                                mm_spatial_pool_mode="bilinear", tokenizer_model_max_length=32768,
                                                tokenizer_padding_side="left")
            self.model = model

        def get_model(self):
            return self.model

        @property
        def device(self):
            return dev

    lm = LM().eval()
    videos = [((torch.arange(FRAMES) + 7 * v) % FRAMES).to(torch.float32).reshape(FRAMES, 1, 1, 1).to(dev) for v in range(V)]
    lens = [6 + 3 * v for v in range(V)]                      # prompts of different lengths, the image token in the middle
    L = max(lens)
    ids = torch.full((V, L), 17, device=dev)
    mask = torch.zeros((V, L), dtype=torch.long, device=dev)
    for v, n in enumerate(lens):
        ids[v, L - n + n // 2] = arch.IMAGE_TOKEN_INDEX
        mask[v, L - n:] = 1
    mods = ["video"] * V

    def batched():
        return lm.prepare_inputs_labels_for_multimodal(ids, None, mask, None, None, videos, mods)

    def singles():
        return [lm.prepare_inputs_labels_for_multimodal(ids[v:v + 1, L - lens[v]:], None, mask[v:v + 1, L - lens[v]:], None, None,
                                                        [videos[v]], ["video"]) for v in range(V)]

    res = {"batched": [], "singles": []}
    with torch.no_grad():
        for _ in range(3):
            batched(); singles()
        for _ in range(ROUNDS):
            res["batched"].append(timed(batched, 5))
            res["singles"].append(timed(singles, 5))
    mb, ms = median(res["batched"]), median(res["singles"])
    print(f"D={hidden} M={M}: {V} videos x {FRAMES} frames through the entry point | one call {mb * 1e3:8.4f} ms "
          f"({V * FRAMES / mb / 1e3:.1f} k frames/s) | {V} single-sample calls {ms * 1e3:8.4f} ms ({V * FRAMES / ms / 1e3:.1f} k frames/s) | "
          f"ratio {ms / mb:.3f}  (spread one call {min(res['batched']) * 1e3:.4f}-{max(res['batched']) * 1e3:.4f}, singles "
          f"{min(res['singles']) * 1e3:.4f}-{max(res['singles']) * 1e3:.4f})", flush=True)

    # ---- placement alone, on the state the last batched call left in the size-8 engine
    rm = model.recurrent_memory_transformer
    bp = rm.row_batcher(V)
    eng = bp.engine(dev, torch.bfloat16)
    with torch.no_grad():
        out = batched()
        mp = model.embed_tokens(torch.tensor(arch.MEMORY_PROMPT_IDS, device=dev)).contiguous()
        fp = model.embed_tokens(torch.tensor(arch.FRAME_PROMPT_IDS, device=dev)).contiguous()
        pooled = [lm.get_2dPool(lm.encode_images(vid[arch.sample_frame_indices(FRAMES).to(dev)])) for vid in videos]
        _, info = arch.video_memory_tokens_batched(model, bp, pooled, arch.sample_frame_indices(FRAMES), mp, fp, model.image_newline)
    rows = info["block_rows"]
    Lmax = out[4].shape[1]
    buf = torch.empty((V * Lmax, hidden), device=dev, dtype=torch.bfloat16)
    stage = torch.empty((V, rows, hidden), device=dev, dtype=torch.bfloat16)
    dst = [v * Lmax + (Lmax - (lens[v] - 1 + rows)) + lens[v] // 2 for v in range(V)]
    xp = (capi.vp * V)(*[x.data_ptr() for x in info["pe_frames"]])
    fine = arch._device_indices(info["fine_idx"], dev)
    nl = model.image_newline.detach().contiguous()
    wr = ctypes.c_int64(0)
    head = (eng.ctx, xp, fine.data_ptr(), fine.numel(), mp.data_ptr(), mp.shape[0], fp.data_ptr(), fp.shape[0], nl.data_ptr(), 1,
            capi.LAYOUTS["one_token"])
    dst_c = (ctypes.c_int64 * V)(*dst)

    def direct():
        capi.check(capi.lib().mavlm_fuse_emit_layout_batch_to(*head, buf.data_ptr(), V * Lmax, dst_c, ctypes.byref(wr), ops.stream_ptr()),
                   "mavlm_fuse_emit_layout_batch_to")

    def staged():
        capi.check(capi.lib().mavlm_fuse_emit_layout_batch(*head, stage.data_ptr(), rows, ctypes.byref(wr), ops.stream_ptr()),
                   "mavlm_fuse_emit_layout_batch")
        for v in range(V):
            buf[dst[v]:dst[v] + rows].copy_(stage[v])

    res = {"direct": [], "staged": []}
    for _ in range(3):
        direct(); staged()
    for _ in range(ROUNDS):
        res["direct"].append(timed(direct, 20))
        res["staged"].append(timed(staged, 20))
    md, mst = median(res["direct"]), median(res["staged"])
    print(f"D={hidden} M={M}: emit of {V} blocks of {rows} rows | per-video destinations {md * 1e3:8.4f} ms | staging + {V} copies "
          f"{mst * 1e3:8.4f} ms | ratio {mst / md:.3f}  (spread {min(res['direct']) * 1e3:.4f}-{max(res['direct']) * 1e3:.4f}, "
          f"{min(res['staged']) * 1e3:.4f}-{max(res['staged']) * 1e3:.4f})", flush=True)
    ws = {s: int(capi.lib().mavlm_workspace_bytes(rm.row_batcher(s).engine(dev, torch.bfloat16).c)) for s in arch.ROW_BATCH_SIZES}
    print(f"D={hidden} M={M}: workspace bytes of the cached batched engines " +
          ", ".join(f"B={s}: {b} ({b / 2 ** 20:.1f} MiB)" for s, b in ws.items()), flush=True)
    del model, lm, table
