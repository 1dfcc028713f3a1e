"""Diagnostic (GPU box): clip row batches at the LLaVA-OneVision-7B width (hidden 3584, 8 heads of 448) with and without the
variable-length forward (`mavlm_set_attention_hd_varlen`, off by default).  Four clips of 31, 27, 23 and 19 frames, M = 8, bf16,
through `run_video_groups` - the model builder and the clips of tools/diag_clip_batch.py.  Three legs:
    single    clips=False: every clip a single video (no two lengths are equal) - code that exists without clip row batches
    clips     clips=True, switch off: one plain-grid launch of the forward per video and formation layer
    clips+vl  clips=True, switch on: one variable-length launch per formation layer
All legs are warmed up, then alternated in one process with device synchronisation around every timed window; medians and
min - max over the rounds, and the launches per pass by kernel kind (the library's HIP-event brackets), go to
profiles/clip_batch_wide.txt.  A difference between two legs counts only if it exceeds the spread of both.
usage: python tools/diag_clip_wide.py [output file]"""
import ctypes
import os
import sys
import time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from memory_augmented_vlm_amd import _capi as capi  # noqa: E402
from memory_augmented_vlm_amd import _ops as ops  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "clip_batch_wide.txt")
HIDDEN, FRAMES = 3584, (31, 27, 23, 19)
M, P, ROUNDS, REPS = 8, 196, 7, 3
LEGS = (("single", False, False), ("clips", True, False), ("clips+vl", True, True))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median(v):
    return sorted(v)[len(v) // 2]


def launches(fn):
    lib, nk = capi.lib(), len(capi.KERNEL_KINDS)
    ms, ln = (ctypes.c_double * nk)(), (ctypes.c_int64 * nk)()
    fl, by = (ctypes.c_double * nk)(), (ctypes.c_double * nk)()
    lib.mavlm_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        capi.check(lib.mavlm_prof_read(ms, ln, fl, by, nk), "mavlm_prof_read")
    finally:
        lib.mavlm_prof_enable(0)
    return {name: int(ln[i]) for i, name in enumerate(capi.KERNEL_KINDS) if ln[i]}


def disjoint(a, b):
    return max(a) < min(b) or max(b) < min(a)


def run(dev):
    model, arch = bench.build_model(dev, hidden=HIDDEN, mem_tokens=M, seed=4321)
    g = torch.Generator(device="cpu").manual_seed(100)
    vids = [(torch.randn((f, P, HIDDEN), generator=g).to(dev).to(torch.bfloat16), torch.arange(f) * 2 + b) for b, f in enumerate(FRAMES)]
    with torch.no_grad():
        mp = model.embed_tokens(torch.tensor(arch.MEMORY_PROMPT_IDS, device=dev)).contiguous()
        fp = model.embed_tokens(torch.tensor(arch.FRAME_PROMPT_IDS, device=dev)).contiguous()

        def leg(clips, vl):
            def f():
                ops.set_attention_hd_varlen(vl)
                try:
                    arch.run_video_groups(model, vids, mp, fp, model.image_newline, clips=clips)
                finally:
                    ops.set_attention_hd_varlen(False)
            return f

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / REPS

        for _ in range(2):                                   # warm-up of all legs (engines, workspaces, index caches)
            for _, clips, vl in LEGS:
                leg(clips, vl)()
        res = {name: [] for name, _, _ in LEGS}
        for _ in range(ROUNDS):
            for name, clips, vl in reversed(LEGS):
                res[name].append(timed(leg(clips, vl)))
        count = {name: launches(leg(clips, vl)) for name, clips, vl in LEGS}
    tot = sum(FRAMES)
    say(f"D={HIDDEN} M={M}: {len(FRAMES)} clips of {FRAMES} frames | groups {arch.plan_clip_batches(list(FRAMES))}")
    for name, _, _ in LEGS:
        m = median(res[name])
        say(f"    {name:9s} {m * 1e3:8.4f} ms median ({tot / m / 1e3:.1f} k frames/s; min - max {min(res[name]) * 1e3:.4f} - "
            f"{max(res[name]) * 1e3:.4f}) | launches per pass {sum(count[name].values())} = {count[name]}")
    for a, b in (("clips+vl", "clips"), ("clips+vl", "single"), ("clips", "single")):
        ma, mb = median(res[a]), median(res[b])
        verdict = ("faster" if ma < mb else "slower") if disjoint(res[a], res[b]) else "no difference beyond the spread of the two legs"
        say(f"    {a} against {b}: {mb / ma:.3f} x ({verdict})")


def main():
    if not torch.cuda.is_available():
        lines.append("tools/diag_clip_wide.py: NOT MEASURED (no GPU in this run)")
    else:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        say(f"tools/diag_clip_wide.py: medians of {ROUNDS} alternated rounds of {REPS} passes, bf16, {torch.cuda.get_device_name(0)}")
        run(dev)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
