"""Diagnostic: cost of the attention-map pass (attention_maps.hip).

1. The pass (`ops.attention_group_mass`, groups of one memory token x one frame) against the column-sum pass
   (`ops.attention_colsum`) of the same shape - the same Q.K^T on MFMA and the same exp2 per score - interleaved in one
   process, at (R, S, H) = (1568, 6272, 8) and (12544, 6272, 8), head sizes 128 and 448.
2. A 64-frame video (two 32-frame chunks, M = 8 memory tokens) through TransformerProjector with `record_attention_maps`
   on against off, interleaved, D = 1024 and D = 3584.
Prints medians of 5 windows; recorded in DESIGN.md section 4.1, not gated anywhere."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import memory_augmented_vlm_amd  # noqa: F401,E402
from memory_augmented_vlm_amd import _ops as ops  # noqa: E402

P = 196


def timed(fn, n):
    """median over 5 windows of n calls, microseconds per call (device events)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / n)
    return sorted(ts)[2] * 1e3


def operator(R, S, H, hd):
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn((R, H * hd), generator=g, device="cuda").bfloat16()
    k = torch.randn((S, H * hd), generator=g, device="cuda").bfloat16()
    _, lse = ops.attention(q, k, k, H, want_lse=True, head_dim=hd)
    for rep in range(2):          # interleaved: A B A B
        a = timed(lambda: ops.attention_group_mass(q, k, lse, H, P, P, head_dim=hd), 20)
        b = timed(lambda: ops.attention_colsum(q, k, lse, H, head_dim=hd), 20)
        tf = 2.0 * R * S * H * hd / (a * 1e-6) / 1e12
        print(f"R={R} S={S} H={H} head_dim={hd} [{rep}]: group mass {a:.1f} us ({tf:.0f} TFLOP/s of Q.K^T), column sums {b:.1f} us, "
              f"ratio {a / b:.2f}", flush=True)


def video(D):
    from oracle import memory_path as O
    from test_gpu_path import make_projector
    cfg = O.PathConfig(hidden=D, heads=8, mem_tokens=8, depth=2)
    proj = make_projector(cfg, O.make_weights(cfg, seed=3))
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn((64, P, D), generator=g, device="cuda").bfloat16()

    def run(record):
        proj.record_attention_maps = record
        proj.memory_cache = []
        proj.frame_attn_scores = []
        proj(x[:32])
        proj(x[32:])

    with torch.no_grad():
        for rep in range(2):
            off = timed(lambda: run(False), 5)
            on = timed(lambda: run(True), 5)
            print(f"64-frame video D={D} M=8 [{rep}]: recording off {off:.0f} us, on {on:.0f} us, ratio {on / off:.3f}", flush=True)


if __name__ == "__main__":
    for hd in (128, 448):
        for R in (1568, 12544):
            operator(R, 6272, 8, hd)
    for D in (1024, 3584):
        video(D)
