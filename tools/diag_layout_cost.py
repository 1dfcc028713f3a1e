"""Diagnostic (GPU box): cost of a video token layout - a whole 64-frame video as "grid" (one newline per row of the patch grid:
1/14 more rows, the output-row map of the fuser's second GEMM or scratch + copy) against "one_token", same process, interleaved.
Also times the extra pass alone where a shape takes the scratch-and-copy route (the "grid" block minus its literal rows is then
written twice).
usage: python tools/diag_layout_cost.py"""
import os
import sys
import time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
LAYOUTS = ("one_token", "grid")
for (hidden, frames, M) in ((1024, 64, 64), (1024, 64, 8), (3584, 64, 8)):
    bench.HIDDEN, bench.FRAMES = hidden, frames
    model, arch = bench.build_model(dev, hidden=hidden, mem_tokens=M, seed=4321)
    idx = torch.arange(frames)
    g = torch.Generator(device="cpu").manual_seed(100)
    x = torch.randn((frames, bench.PATCHES, hidden), generator=g).to(dev).to(torch.bfloat16)
    mp = torch.nn.functional.embedding(torch.tensor(arch.MEMORY_PROMPT_IDS, device=dev), model.embed_tokens.weight)
    fp = torch.nn.functional.embedding(torch.tensor(arch.FRAME_PROMPT_IDS, device=dev), model.embed_tokens.weight)
    outs = {L: torch.empty((arch.video_token_rows(frames, M, layout=L), hidden), device=dev, dtype=torch.bfloat16) for L in LAYOUTS}

    def step(L):
        return arch.video_memory_tokens(model, x, idx, mp, fp, model.image_newline, out=outs[L], layout=L)

    res = {L: [] for L in LAYOUTS}
    n = 20 if hidden == 1024 else 5
    with torch.no_grad():
        for L in LAYOUTS:
            for _ in range(3):
                step(L)
        for rnd in range(7):
            for L in LAYOUTS:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(n):
                    step(L)
                torch.cuda.synchronize(); res[L].append((time.perf_counter() - t0) / n)
    med = {L: sorted(v)[len(v) // 2] for L, v in res.items()}
    print(f"D={hidden} frames={frames} M={M}: one_token {med['one_token'] * 1e3:8.4f} ms | grid {med['grid'] * 1e3:8.4f} ms | "
          f"grid / one_token {med['grid'] / med['one_token']:.4f}  (spread one_token {min(res['one_token']) * 1e3:.4f}-"
          f"{max(res['one_token']) * 1e3:.4f}, grid {min(res['grid']) * 1e3:.4f}-{max(res['grid']) * 1e3:.4f})", flush=True)
    del model
