"""Diagnostic (GPU box): the frame-score forward with its (a, m) entries in LDS (attention3.hip FR = 3, the default) against the
scratch form (FR = 1, `mavlm_set_frame_entries_lds(0)`) and the plain forward, at the bench launch shape: 16 (video, head) pairs,
R = 12 544 query rows, S = 6 272 keys of 32 frames, one process, alternating blocks of launches (HIP events around a block).
Prints every block's time, the medians, both ratios to the plain launch, and the spread of the FR = 1 blocks - the yardstick:
FR = 3 counts as faster only if its ratio lies below FR = 1's by more than that spread.
usage: python tools/diag_frames_lds_ab.py [blocks=7] [launches per block=20]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import memory_augmented_vlm_amd  # noqa: F401
    from memory_augmented_vlm_amd import _capi as capi
    from memory_augmented_vlm_amd import _ops as ops
    blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    lib = capi.lib()
    H, R, S, P = 16, 12544, 6272, 196
    info = (capi.i32 * 4)()
    capi.check(lib.mavlm_attention_plan(R, S, H, info), "plan")
    print(f"plan: {info[0]} waves, {info[1]} workgroups, {info[2]} cut levels", flush=True)
    W = H * 128
    torch.manual_seed(0)
    q = (torch.randn(R, W, device="cuda") * 0.5).bfloat16()
    k = (torch.randn(S, W, device="cuda") * 0.5).bfloat16()
    v = torch.randn(S, W, device="cuda").bfloat16()

    def frames(on):
        def f():
            lib.mavlm_set_frame_entries_lds(on)
            ops.attention_frames(q, k, v, H, P)
        return f

    cands = [("plain", lambda: ops.attention(q, k, v, H)), ("FR=1", frames(0)), ("FR=3", frames(1))]
    lib.mavlm_set_frame_entries_lds(0)
    r1 = ops.attention_frames(q, k, v, H, P, want_lse=True)
    lib.mavlm_set_frame_entries_lds(1)
    r3 = ops.attention_frames(q, k, v, H, P, want_lse=True)
    print("FR = 3 == FR = 1 (ctx, lse2, scores):", all(torch.equal(x, y) for x, y in zip(r1, r3)), flush=True)
    t0 = time.time()
    while time.time() - t0 < 0.5:                          # clocks up before the first measured block
        for _, f in cands:
            for _ in range(5):
                f()
        torch.cuda.synchronize()
    times = {name: [] for name, _ in cands}
    for blk in range(blocks):
        for name, f in cands:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / n * 1e3)
        print(f"block {blk}: " + "  ".join(f"{name} {times[name][-1]:7.1f} us" for name, _ in cands), flush=True)
    lib.mavlm_set_frame_entries_lds(1)
    med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
    ratios = {name: [x / p for x, p in zip(times[name], times["plain"])] for name in ("FR=1", "FR=3")}
    for name in ("plain", "FR=1", "FR=3"):
        print(f"{name:6s} median {med[name]:7.1f} us  min {min(times[name]):7.1f}  max {max(times[name]):7.1f}")
    for name in ("FR=1", "FR=3"):
        rs = sorted(ratios[name])
        print(f"{name} / plain per block: median {rs[len(rs) // 2]:.4f}  min {rs[0]:.4f}  max {rs[-1]:.4f}")
    spread = max(ratios["FR=1"]) - min(ratios["FR=1"])
    gain = sorted(ratios["FR=1"])[blocks // 2] - sorted(ratios["FR=3"])[blocks // 2]
    print(f"FR=1 ratio - FR=3 ratio (medians): {gain:+.4f}; spread of the FR=1 blocks: {spread:.4f} -> "
          f"{'FR=3 is faster' if gain > spread else 'not distinguishable / not faster'}")


if __name__ == "__main__":
    main()
