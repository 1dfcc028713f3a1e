#!/usr/bin/env python3
"""Golden attention maps (g10_attention_maps.npz): the reference projector's own probabilities, grouped.

Runs ONLY where the reference is present (as make_golden.py, whose import recipe, weight loader and save helpers it uses).
Forward hooks on the reference's `Attention` modules take the probabilities `[1, H, R, S]` each forward returns and group them

    formation (every layer):  [H, M, F]      rows of one memory token x patches of one frame
    evolution:                [H, M, n_past] rows of one memory token x keys of one cached memory (torch.cat order: oldest first)

for every chunk of one video (32, 32, 7 frames) at D = 1024, H = 8, M = 8, P = 196, depth 2 - once in fp32 and once in the
reference's own bf16 run.  The fixture holds the maps, the seeds, and per map the reference's envelope
e = rel_l2(bf16 map, fp32 map), which the GPU test uses as its yardstick.

Frames = seeded normal patches + one normal offset vector per frame: plain normal frames give formation maps within a few
percent of uniform, which pin nothing.  The generator asserts a relative distance of at least 0.1 from the uniform map on every
formation map and raises the offset amplitude until it holds.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_maps.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (loads the reference's files at run time)
from make_golden import O  # noqa: E402

HIDDEN, HEADS, MEM, DEPTH, P = 1024, 8, 8, 2, 196
FRAMES = (32, 32, 7)
WSEED, SEGSEED, OFFSEED = 101, 1000, 1100
MIN_FROM_UNIFORM = 0.1


def frames_of(t, f, amp):
    """chunk t: normal patches + amp x one normal offset vector per frame, on the bf16 grid"""
    x = O.hash_normal_like((f, P, HIDDEN), SEGSEED + t) + amp * O.hash_normal_like((f, 1, HIDDEN), OFFSEED + t)
    return O.bf16_round(x)


def run(dtype, amp):
    """the reference projector over the video; returns per chunk (formation [depth, H, M, F], evolution [H, M, n] | None)"""
    cfg = O.PathConfig(hidden=HIDDEN, heads=HEADS, mem_tokens=MEM, depth=DEPTH)
    w = O.make_weights(cfg, seed=WSEED)
    m = G.ref_projector(cfg, w, dtype)
    got = {}

    def grouped(probs, kg):
        p = probs[0].float()                                   # [H, R, S]
        h, r, s = p.shape
        return p.reshape(h, r // P, P, s // kg, kg).sum(dim=(2, 4)).numpy().copy()

    def hook(name, kg):
        def f(_mod, _inp, out):
            got.setdefault(name, []).append(grouped(out[1], kg))
        return f

    m.memory_update_attention.register_forward_hook(hook("evo", MEM * P))
    for layer in m.layers:
        layer.memory_segment_fusion_attention.register_forward_hook(hook("form", P))
    m.memory_cache = []
    m.frame_attn_scores = []
    out = []
    for t, f in enumerate(FRAMES):
        got.clear()
        _, scores = m(G.T(frames_of(t, f, amp)).to(dtype))
        assert len(got["form"]) == DEPTH and len(got.get("evo", [])) == (1 if t else 0)
        out.append((np.stack(got["form"]), got["evo"][0] if t else None, scores[-1].float().numpy().copy()))
    return out


def from_uniform(a):
    u = np.full_like(a, a.sum() / a.size, dtype=np.float64)
    return O.rel_l2(a, u)


def main():
    amp = 1.0
    while True:
        ref32 = run(torch.float32, amp)
        far = [from_uniform(form[l]) for form, _, _ in ref32 for l in range(DEPTH)]
        print(f"amplitude {amp}: formation maps {min(far):.3f} .. {max(far):.3f} from uniform")
        if min(far) >= MIN_FROM_UNIFORM:
            break
        amp += 1.0
        assert amp <= 8.0, "formation maps stay uniform"
    ref16 = run(torch.bfloat16, amp)
    arrs, env_form, env_evo, far_evo = {}, [], [], []
    for t, ((f32, e32, s32), (f16, e16, _)) in enumerate(zip(ref32, ref16)):
        arrs[f"fp32_form_{t}"], arrs[f"bf16_form_{t}"] = f32.astype(np.float32), f16.astype(np.float32)
        arrs[f"fp32_scores_{t}"] = s32
        env_form.append([O.rel_l2(f16[l], f32[l]) for l in range(DEPTH)])
        if e32 is not None:
            arrs[f"fp32_evo_{t}"], arrs[f"bf16_evo_{t}"] = e32.astype(np.float32), e16.astype(np.float32)
            env_evo.append(O.rel_l2(e16, e32))
            far_evo.append(from_uniform(e32))
    print("envelope rel_l2(reference bf16, reference fp32): formation", env_form, "evolution", env_evo)
    print("evolution maps from uniform:", far_evo)
    G.save("g10_attention_maps.npz",
           meta=G.meta(hidden=HIDDEN, heads=HEADS, mem_tokens=MEM, depth=DEPTH, patches=P, frames=list(FRAMES), wseed=WSEED,
                       segseed0=SEGSEED, offseed0=OFFSEED, amplitude=amp, from_uniform_formation=far,
                       from_uniform_evolution=far_evo, envelope_formation=env_form, envelope_evolution=env_evo),
           **arrs)


if __name__ == "__main__":
    main()
